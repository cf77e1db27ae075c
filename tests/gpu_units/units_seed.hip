// tests/gpu_units/units_seed.hip -- TEST INFRASTRUCTURE: host-callable wrappers around the seeding front end
// (k_seed.hip and the rank / LF / suffix-array helpers of dev_common.h), so that tests/test_units_seed.py can compare
// them with the oracle's FM-index one function at a time.  Built in two flavours like units.hip (hipcc for gfx950, g++
// against the emulation); never part of libbwamem_hip.so.
//
// Return codes: 0 = done, -1 = a runtime call failed, -2 = refused: an argument would make a kernel touch memory outside
// what the wrapper allocated (checked on the host; nothing is launched), -3 = an output array of the caller is too small.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../gatk-bwamem-jni_amd/csrc/k_seed.hip"
#include "../../gatk-bwamem-jni_amd/csrc/index_io.h"

namespace {
struct DBuf {
    void* p = nullptr;
    DBuf() {}
    DBuf(const DBuf&) = delete;
    ~DBuf() { if (p) (void)hipFree(p); }
    bool alloc(size_t n, int fill = 0) { return hipMalloc(&p, n + 64) == hipSuccess && hipMemset(p, fill, n + 64) == hipSuccess; }   // 64 bytes of slack
    bool up(const void* src, size_t n) { return alloc(n) && (n == 0 || hipMemcpy(p, src, n, hipMemcpyHostToDevice) == hipSuccess); }
    bool down(void* dst, size_t n) const { return n == 0 || hipMemcpy(dst, p, n, hipMemcpyDeviceToHost) == hipSuccess; }
    template <typename T> T* as() const { return (T*)p; }
};
bool ran() { return hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess; }

struct UIndex {
    std::vector<uint8_t> img;
    HostIndex h;
    DevIndex d;
    DBuf occ, sa_lo, sa_hi, pac, ann_off, ann_len;
    size_t n_kept = 0;
    int32_t densify_err = -1;
};
}

// ------------------------------------------------------------------------------------------ wrapper kernels
__global__ void k_unit_sa_lookup(DevIndex ix, const uint64_t* ks, int64_t n, int64_t* out, unsigned long long* n_lf_total)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t n_lf = 0;
    if (i < n) out[i] = (int64_t)sa_lookup(ix, ks[i], n_lf);
    count_add(n_lf_total, (unsigned long long)n_lf);
}
__global__ void k_unit_lf(DevIndex ix, const uint64_t* ks, int64_t n, uint64_t* out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = lf_step(ix, ks[i]);
}
__global__ void k_unit_extend_sm(DevIndex ix, const uint64_t* x0, const uint64_t* x1, const uint64_t* size, const int32_t* c, const int32_t* is_back, int64_t n, uint64_t* out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t o0, o1, os;
    extend_sm(ix, x0[i], x1[i], size[i], c[i], is_back[i] != 0, o0, o1, os);
    out[3 * i] = o0; out[3 * i + 1] = o1; out[3 * i + 2] = os;
}
// CandStack as k_seed lays it out: n pushes per lane ([entry][lane] arrays; the ring spills), two pushes the global area has no
// room for, every entry read back, every entry overwritten from the top down (what the backward phase does), read back again
__global__ void __launch_bounds__(64) k_unit_candstack(int K, int narrow, int spill_cap, int n, const uint64_t* x0, const uint64_t* sz, const int32_t* en,
                                                       const uint64_t* x0b, const uint64_t* szb, const int32_t* enb, uint4* spill, uint64_t* out, int32_t* ok)
{
    HIP_DYNAMIC_SHARED(uint32_t, lds)
    const int lane = threadIdx.x;
    CandStack V;
    V.narrow = narrow != 0;
    V.v0 = lds + lane; V.v1 = V.v0 + K * 64; V.v2 = V.v1 + K * 64; V.K = K;
    V.v2n = (uint16_t*)(lds + 2 * K * 64) + lane;
    V.spill = spill + lane; V.spill_cap = spill_cap;
    for (int e = 0; e < n + 2; ++e) {
        const int s = (e < n ? e : n - 1) * 64 + lane;
        ok[e * 64 + lane] = V.push(e, x0[s], sz[s], en[s]) ? 1 : 0;
    }
    for (int ph = 0; ph < 2; ++ph) {
        for (int e = 0; e < n; ++e) {
            uint64_t a, b; int c;
            V.get(e, n, a, b, c);
            uint64_t* o = out + ((size_t)(ph * n + e) * 64 + lane) * 3;
            o[0] = a; o[1] = b; o[2] = (uint64_t)(int64_t)c;
        }
        if (ph == 0) for (int e = n - 1; e >= 0; --e) V.put(e, n, x0b[e * 64 + lane], szb[e * 64 + lane], enb[e * 64 + lane]);
    }
}

// ------------------------------------------------------------------------------------------ 1. the index on the device
// an image as upload_index (pipeline.cpp) puts it on the device: launch_build_occ64 + launch_sa_densify with every
// sa_intv-th rank kept (a power of two up to the image's own spacing)
extern "C" void useed_index_close(void* hv) { delete (UIndex*)hv; }
extern "C" void* useed_index_open(const char* path, int sa_intv)
{
    UIndex* u = new UIndex;
    bool ok = false;
    do {
        FILE* f = fopen(path, "rb");
        if (!f) break;
        fseek(f, 0, SEEK_END); const long sz = ftell(f); fseek(f, 0, SEEK_SET);
        u->img.resize(sz > 0 ? (size_t)sz : 0);
        const bool rd = sz > 0 && fread(u->img.data(), 1, (size_t)sz, f) == (size_t)sz;
        fclose(f);
        if (!rd || !parse_index_image(u->img.data(), u->img.size(), u->h)) break;
        const HostIndex& h = u->h;
        if (h.seq_len >= (1ull << 37) || sa_intv < 1 || (sa_intv & (sa_intv - 1)) || sa_intv > h.sa_intv) break;
        const uint64_t n_blocks = (h.seq_len + 63) / 64 + 1;
        {
            DBuf tmp;
            const size_t bwt_bytes = ((size_t)h.bwt_size * 4 + 255) & ~(size_t)63;
            if (!tmp.alloc(bwt_bytes) || !u->occ.alloc((size_t)n_blocks * 32 + 64)) break;
            if (hipMemcpy(tmp.p, h.bwt, (size_t)h.bwt_size * 4, hipMemcpyHostToDevice) != hipSuccess) break;
            launch_build_occ64(0, tmp.as<uint32_t>(), n_blocks, u->occ.as<uint4>());
            if (!ran()) break;
        }
        const int n = (int)h.contigs.size();
        std::vector<int64_t> off((size_t)n); std::vector<int32_t> len((size_t)n);
        for (int i = 0; i < n; ++i) { off[i] = h.contigs[i].offset; len[i] = h.contigs[i].len; }
        if (!u->pac.up(h.pac, (size_t)(h.l_pac / 4 + 1)) || !u->ann_off.up(off.data(), (size_t)n * 8) || !u->ann_len.up(len.data(), (size_t)n * 4)) break;
        DevIndex& d = u->d;
        memset(&d, 0, sizeof d);
        d.occ = u->occ.as<uint4>(); d.pac = u->pac.as<uint8_t>(); d.ann_offset = u->ann_off.as<int64_t>(); d.ann_len = u->ann_len.as<int32_t>();
        d.primary = h.primary; for (int i = 0; i < 5; ++i) d.L2[i] = h.L2[i];
        d.seq_len = h.seq_len; d.l_pac = h.l_pac; d.n_seqs = n;
        { int v = 0; d.n_cu = hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, 0) == hipSuccess && v > 0 ? v : 256; }
        d.sa_intv = sa_intv; d.sa_shift = 0;
        while ((1 << d.sa_shift) < sa_intv) ++d.sa_shift;
        u->n_kept = (size_t)(h.seq_len >> d.sa_shift) + 1;
        DBuf src, flag;
        if (!u->sa_lo.alloc(u->n_kept * 4 + 64, 0xee) || !u->sa_hi.alloc(u->n_kept + 64, 0xee) || !src.up(h.sa, (size_t)h.n_sa * 8) || !flag.alloc(64)) break;
        d.sa_lo = u->sa_lo.as<uint32_t>(); d.sa_hi = u->sa_hi.as<uint8_t>();
        launch_sa_densify(0, d, src.as<uint64_t>(), h.n_sa, h.sa_intv, u->sa_lo.as<uint32_t>(), u->sa_hi.as<uint8_t>(), flag.as<int32_t>());
        if (!ran() || !flag.down(&u->densify_err, 4)) break;
        ok = true;
    } while (0);
    if (!ok) { delete u; return nullptr; }
    return u;
}
// primary, L2[0..4], seq_len, kept SA entries, kept spacing, the densification's error flag, l_pac, n_seqs
extern "C" void useed_index_info(void* hv, uint64_t* out12)
{
    const UIndex* u = (const UIndex*)hv;
    out12[0] = u->d.primary; for (int i = 0; i < 5; ++i) out12[1 + i] = u->d.L2[i];
    out12[6] = u->d.seq_len; out12[7] = u->n_kept; out12[8] = (uint64_t)u->d.sa_intv; out12[9] = (uint64_t)(int64_t)u->densify_err;
    out12[10] = (uint64_t)u->d.l_pac; out12[11] = (uint64_t)u->d.n_seqs;
}
extern "C" int useed_index_sa_raw(void* hv, uint32_t* lo, uint8_t* hi)
{
    const UIndex* u = (const UIndex*)hv;
    return u->sa_lo.down(lo, u->n_kept * 4) && u->sa_hi.down(hi, u->n_kept) ? 0 : -1;
}

static int run_sa_lookup(const DevIndex& ix, int64_t n, const uint64_t* ks, int64_t* out, uint64_t* n_lf)
{
    DBuf dk, dout, dn;
    if (!dk.up(ks, (size_t)n * 8) || !dout.alloc((size_t)n * 8) || !dn.alloc(8)) return -1;
    if (n > 0) hipLaunchKernelGGL(k_unit_sa_lookup, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, ix, dk.as<uint64_t>(), n, dout.as<int64_t>(), dn.as<unsigned long long>());
    return ran() && dout.down(out, (size_t)n * 8) && dn.down(n_lf, 8) ? 0 : -1;
}
static int run_lf(const DevIndex& ix, int64_t n, const uint64_t* ks, uint64_t* out)
{
    DBuf dk, dout;
    if (!dk.up(ks, (size_t)n * 8) || !dout.alloc((size_t)n * 8)) return -1;
    if (n > 0) hipLaunchKernelGGL(k_unit_lf, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, ix, dk.as<uint64_t>(), n, dout.as<uint64_t>());
    return ran() && dout.down(out, (size_t)n * 8) ? 0 : -1;
}
static int run_extend(const DevIndex& ix, int64_t n, const uint64_t* x0, const uint64_t* x1, const uint64_t* size, const int32_t* c, const int32_t* is_back, uint64_t* out)
{
    DBuf d0, d1, ds, dc, db, dout;
    if (!d0.up(x0, (size_t)n * 8) || !d1.up(x1, (size_t)n * 8) || !ds.up(size, (size_t)n * 8) || !dc.up(c, (size_t)n * 4) || !db.up(is_back, (size_t)n * 4) || !dout.alloc((size_t)n * 24)) return -1;
    if (n > 0) hipLaunchKernelGGL(k_unit_extend_sm, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, ix, d0.as<uint64_t>(), d1.as<uint64_t>(), ds.as<uint64_t>(), dc.as<int32_t>(), db.as<int32_t>(), n, dout.as<uint64_t>());
    return ran() && dout.down(out, (size_t)n * 24) ? 0 : -1;
}
// the stored blocks (sentinel skipped) the rank step of (x0, x1, size) reads; false when the arguments are outside extend_sm's contract
static bool extend_blocks(uint64_t primary, uint64_t seq_len, uint64_t x0, uint64_t x1, uint64_t size, int c, int is_back, uint64_t& bk, uint64_t& bl)
{
    const uint64_t xa = is_back ? x0 : x1;
    if (c < 0 || c > 3 || xa < 1 || size > seq_len || xa - 1 + size > seq_len) return false;
    const uint64_t k = xa - 1, l = xa - 1 + size;
    bk = (k - (k >= primary)) >> 6; bl = (l - (l >= primary)) >> 6;
    return true;
}

extern "C" int useed_sa_lookup(void* hv, int64_t n, const uint64_t* ks, int64_t* out, uint64_t* n_lf)
{
    const UIndex* u = (const UIndex*)hv;
    for (int64_t i = 0; i < n; ++i) if (ks[i] < 1 || ks[i] > u->d.seq_len) return -2;
    return run_sa_lookup(u->d, n, ks, out, n_lf);
}
extern "C" int useed_lf(void* hv, int64_t n, const uint64_t* ks, uint64_t* out)
{
    const UIndex* u = (const UIndex*)hv;
    for (int64_t i = 0; i < n; ++i) if (ks[i] > u->d.seq_len) return -2;
    return run_lf(u->d, n, ks, out);
}
// ---- 2. the rank step; out[3i..] = o0, o1, osz
extern "C" int useed_extend(void* hv, int64_t n, const uint64_t* x0, const uint64_t* x1, const uint64_t* size, const int32_t* c, const int32_t* is_back, uint64_t* out)
{
    const UIndex* u = (const UIndex*)hv;
    uint64_t bk, bl;
    for (int64_t i = 0; i < n; ++i) if (!extend_blocks(u->d.primary, u->d.seq_len, x0[i], x1[i], size[i], c[i], is_back[i], bk, bl)) return -2;
    return run_extend(u->d, n, x0, x1, size, c, is_back, out);
}

// ---- 3. the same arithmetic beyond 2^32 on a window: `table` holds n_blocks device-layout blocks (8 words each) that stand for
// blocks B0 .. B0 + n_blocks - 1 of an index with the given primary, L2 and seq_len
extern "C" int useed_window(const uint32_t* table, uint64_t n_blocks, uint64_t B0, uint64_t primary, const uint64_t* L2, uint64_t seq_len,
                            int64_t n_ext, const uint64_t* x0, const uint64_t* x1, const uint64_t* size, const int32_t* c, const int32_t* is_back, uint64_t* out_ext,
                            int64_t n_lf, const uint64_t* ks, uint64_t* out_lf)
{
    if (n_blocks < 1 || B0 > (1ull << 40) || n_blocks > (1ull << 20)) return -2;
    for (int64_t i = 0; i < n_ext; ++i) {
        uint64_t bk, bl;
        if (!extend_blocks(primary, seq_len, x0[i], x1[i], size[i], c[i], is_back[i], bk, bl)) return -2;
        if (bk < B0 || bk >= B0 + n_blocks || bl < B0 || bl >= B0 + n_blocks) return -2;
    }
    for (int64_t i = 0; i < n_lf; ++i) {
        if (ks[i] > seq_len) return -2;
        if (ks[i] == primary) continue;
        const uint64_t b = (ks[i] - (ks[i] > primary)) >> 6;
        if (b < B0 || b >= B0 + n_blocks) return -2;
    }
    DBuf dt;
    if (!dt.up(table, (size_t)n_blocks * 32)) return -1;
    DevIndex ix; memset(&ix, 0, sizeof ix);
    ix.occ = (const uint4*)((uintptr_t)dt.p - (uintptr_t)32 * B0);
    ix.primary = primary; for (int i = 0; i < 5; ++i) ix.L2[i] = L2[i];
    ix.seq_len = seq_len; ix.sa_intv = 1;
    int rc = run_extend(ix, n_ext, x0, x1, size, c, is_back, out_ext);
    return rc ? rc : run_lf(ix, n_lf, ks, out_lf);
}
// sa_lookup on a dense table given as its two planes
extern "C" int useed_sa_synth(int64_t n_entries, const uint32_t* lo, const uint8_t* hi, int64_t n, const uint64_t* ks, int64_t* out, uint64_t* n_lf)
{
    for (int64_t i = 0; i < n; ++i) if (ks[i] >= (uint64_t)n_entries) return -2;
    DBuf dl, dh;
    if (!dl.up(lo, (size_t)n_entries * 4) || !dh.up(hi, (size_t)n_entries)) return -1;
    DevIndex ix; memset(&ix, 0, sizeof ix);
    ix.sa_lo = dl.as<uint32_t>(); ix.sa_hi = dh.as<uint8_t>(); ix.sa_intv = 1; ix.sa_shift = 0; ix.seq_len = (uint64_t)n_entries - 1;
    return run_sa_lookup(ix, n, ks, out, n_lf);
}
// CandStack round trips: arrays are [n][64]; out = [2][n][64][3] (after the pushes, after the puts); ok = [n + 2][64] push results
extern "C" int useed_candstack(int K, int narrow, int n, const uint64_t* x0, const uint64_t* sz, const int32_t* en, const uint64_t* x0b, const uint64_t* szb, const int32_t* enb, uint64_t* out, int32_t* ok)
{
    if (K < 1 || K > 64 || (K & (K - 1)) || n <= K || n > 4096) return -2;
    const uint64_t vmax = narrow ? (1ull << 35) : (1ull << 37);
    const int emax = narrow ? 1023 : (1 << 17);
    for (int i = 0; i < n * 64; ++i)
        if (x0[i] >= vmax || sz[i] >= vmax || x0b[i] >= vmax || szb[i] >= vmax || en[i] < 0 || en[i] >= emax || enb[i] < 0 || enb[i] >= emax) return -2;
    const int spill_cap = n - K;
    const size_t m = (size_t)n * 64;
    DBuf d0, d1, d2, e0, e1, e2, sp, dout, dok;
    if (!d0.up(x0, m * 8) || !d1.up(sz, m * 8) || !d2.up(en, m * 4) || !e0.up(x0b, m * 8) || !e1.up(szb, m * 8) || !e2.up(enb, m * 4)
        || !sp.alloc((size_t)spill_cap * 64 * 16, 0xab) || !dout.alloc(2 * m * 24) || !dok.alloc((m + 128) * 4, 0xff)) return -1;
    const size_t lds = (size_t)(narrow ? 5 * K * 32 : 3 * K * 64) * 4;
    hipLaunchKernelGGL(k_unit_candstack, dim3(1), dim3(64), lds, 0, K, narrow, spill_cap, n, d0.as<uint64_t>(), d1.as<uint64_t>(), d2.as<int32_t>(),
                       e0.as<uint64_t>(), e1.as<uint64_t>(), e2.as<int32_t>(), sp.as<uint4>(), dout.as<uint64_t>(), dok.as<int32_t>());
    return ran() && dout.down(out, 2 * m * 24) && dok.down(ok, (m + 128) * 4) ? 0 : -1;
}

// ------------------------------------------------------------------------------------------ 4. k_seed + k_seed_fin + scan + k_sa
// request: n_reads NUL-terminated ASCII reads back to back, seq_off[n_reads + 1] their offsets.  mode 0: k_seed<LDSQ> launched
// here with the given K, refill_min, narrow and grid; mode 1: through launch_seed (production's geometry; K, refill_min, narrow and
// grid are ignored).  intv = [n_reads][intv_cap][3] (x0, size, info), iso = [n_reads][intv_cap], seeds: seeds_cap entries.
extern "C" int useed_seed(void* hv, const MemOpt* opt, int n_reads, const uint8_t* request, const int64_t* seq_off, int mode, int K, int refill_min, int narrow, int grid,
                          int intv_cap, int smem_cap, int32_t* n_intv, uint64_t* intv, int32_t* iso, int32_t* n_seeds, int32_t* l_rep, int64_t* seed_off,
                          int64_t seeds_cap, int64_t* rbeg, int32_t* qbeg, int32_t* slen, int32_t* rid, int32_t* err, uint64_t* cnt3)
{
    const UIndex* u = (const UIndex*)hv;
    if (n_reads < 1 || intv_cap < 1 || smem_cap < 1) return -2;
    int max_len = 0;
    for (int r = 0; r < n_reads; ++r) {
        const int64_t l = seq_off[r + 1] - seq_off[r] - 1;
        if (l < 0 || l >= (1 << 17)) return -2;
        max_len = l > max_len ? (int)l : max_len;
    }
    const size_t n_bytes = (size_t)seq_off[n_reads];
    const size_t qbytes = (size_t)64 * 4 * (((size_t)max_len + 7) / 8);
    const bool ldsq = qbytes <= 24576;
    size_t lds = 0;
    int groups = (n_reads + 63) / 64;
    if (mode == 0) {
        if (K < 1 || K > 64 || (K & (K - 1)) || refill_min < 1 || grid < 1 || grid > 65536) return -2;
        if (narrow && !(u->d.seq_len < (1ull << 35) && max_len < 1023)) return -2;
        lds = (size_t)(narrow ? 5 * K * 32 : 3 * K * 64) * 4 + (size_t)SEED_EL_CAP * 64 * 4 + (ldsq ? qbytes : 0) + 16;
        if (lds > (size_t)64 << 10) return -2;
        groups = grid;
    }
    const size_t nr = (size_t)n_reads;
    DBuf dseq, doff, dintv, dnintv, diso, dns, dlrep, dsoff, derr, dcnt, dsmem, dtmp;
    if (!dseq.up(request, n_bytes) || !doff.up(seq_off, (nr + 1) * 8) || !dintv.alloc(nr * intv_cap * sizeof(Intv), 0xcd) || !dnintv.alloc(nr * 4, 0xff)
        || !diso.alloc(nr * intv_cap * 4, 0xcd) || !dns.alloc(nr * 4, 0xff) || !dlrep.alloc(nr * 4, 0xff) || !dsoff.alloc((nr + 1) * 8, 0xff) || !derr.alloc(64) || !dcnt.alloc(sizeof(DevCounters))
        || !dsmem.alloc((size_t)groups * smem_cap * 64 * 16, 0xab) || !dtmp.alloc(scan_tmp_bytes(n_reads))) return -1;
    launch_encode(0, dseq.as<uint8_t>(), (int64_t)n_bytes);
    TileView tv; memset(&tv, 0, sizeof tv);
    tv.n_reads = n_reads; tv.max_len = max_len; tv.seq = dseq.as<uint8_t>(); tv.seq_off = doff.as<int64_t>();
    tv.intv_cap = intv_cap; tv.intv = dintv.as<Intv>(); tv.n_intv = dnintv.as<int32_t>();
    tv.intv_seed_off = diso.as<int32_t>(); tv.n_seeds = dns.as<int32_t>(); tv.l_rep = dlrep.as<int32_t>(); tv.seed_off = dsoff.as<int64_t>();
    tv.smem_scratch = dsmem.as<Intv>(); tv.smem_cap = smem_cap; tv.smem_groups = groups;
    tv.err = derr.as<int32_t>(); tv.cnt = dcnt.as<DevCounters>();
    if (mode == 1) launch_seed(0, u->d, *opt, tv);
    else {
        if (ldsq) hipLaunchKernelGGL(k_seed<true>, dim3(grid), dim3(64), lds, 0, u->d, *opt, tv, K, refill_min, narrow);
        else hipLaunchKernelGGL(k_seed<false>, dim3(grid), dim3(64), lds, 0, u->d, *opt, tv, K, refill_min, narrow);
        hipLaunchKernelGGL(k_seed_fin, dim3((n_reads + 255) / 256), dim3(256), 0, 0, *opt, tv);
    }
    if (!ran()) return -1;
    launch_scan(0, tv.n_seeds, tv.seed_off, n_reads, dtmp.as<int64_t>());
    int64_t n_occ = -1;
    if (!ran() || hipMemcpy(&n_occ, tv.seed_off + n_reads, 8, hipMemcpyDeviceToHost) != hipSuccess || n_occ < 0) return -1;
    if (n_occ > seeds_cap) return -3;
    DBuf dseeds, drid;
    if (!dseeds.alloc((size_t)n_occ * sizeof(Seed), 0xcd) || !drid.alloc((size_t)n_occ * 4, 0xcd)) return -1;
    tv.seeds = dseeds.as<Seed>(); tv.seed_rid = drid.as<int32_t>();
    launch_sa(0, u->d, *opt, tv, n_occ);
    if (!ran()) return -1;
    std::vector<Intv> hi(nr * intv_cap); std::vector<Seed> hs((size_t)n_occ);
    DevCounters hc;
    if (!dintv.down(hi.data(), hi.size() * sizeof(Intv)) || !dnintv.down(n_intv, nr * 4) || !diso.down(iso, nr * intv_cap * 4) || !dns.down(n_seeds, nr * 4) || !dlrep.down(l_rep, nr * 4)
        || !dsoff.down(seed_off, (nr + 1) * 8) || !dseeds.down(hs.data(), hs.size() * sizeof(Seed)) || !drid.down(rid, (size_t)n_occ * 4) || !derr.down(err, 4) || !dcnt.down(&hc, sizeof hc)) return -1;
    for (size_t i = 0; i < hi.size(); ++i) { intv[3 * i] = hi[i].x0; intv[3 * i + 1] = hi[i].size; intv[3 * i + 2] = hi[i].info; }
    for (size_t i = 0; i < hs.size(); ++i) { rbeg[i] = hs[i].rbeg; qbeg[i] = hs[i].qbeg; slen[i] = hs[i].len; }
    cnt3[0] = hc.n_ext; cnt3[1] = hc.n_lf; cnt3[2] = hc.n_sa;
    return 0;
}

// ------------------------------------------------------------------------------------------ 5. the small kernels of k_seed.hip
extern "C" int useed_scan(const int32_t* in, int n, int64_t* out)
{
    if (n < 0) return -2;
    DBuf di, dout, dtmp;
    if (!di.up(in, (size_t)n * 4) || !dout.alloc(((size_t)n + 1) * 8, 0xff) || !dtmp.alloc(scan_tmp_bytes(n))) return -1;
    launch_scan(0, di.as<int32_t>(), dout.as<int64_t>(), n, dtmp.as<int64_t>());
    return ran() && dout.down(out, ((size_t)n + 1) * 8) ? 0 : -1;
}
extern "C" int useed_order(const int32_t* n_seeds, int n, int32_t* order)
{
    if (n < 0) return -2;
    DBuf di, dbins, dout;
    if (!di.up(n_seeds, (size_t)n * 4) || !dbins.alloc(64 * 4, 0xff) || !dout.alloc((size_t)n * 4, 0xff)) return -1;
    launch_order(0, di.as<int32_t>(), n, dbins.as<int32_t>(), dout.as<int32_t>());
    return ran() && dout.down(order, (size_t)n * 4) ? 0 : -1;
}
// off: off_n entries, all of them returned (those the kernels did not write hold -1)
extern "C" int useed_nul_offsets(const uint8_t* buf, int64_t n_bytes, int64_t n_reads_max, int64_t off_n, int64_t* off, int64_t* n_found)
{
    if (n_bytes < 0 || n_reads_max < 0 || off_n < n_reads_max + 1) return -2;
    DBuf db, doff, dfound, dtmp;
    if (!db.up(buf, (size_t)n_bytes) || !doff.alloc((size_t)off_n * 8, 0xff) || !dfound.alloc(8, 0xff) || !dtmp.alloc(nul_tmp_bytes(n_bytes))) return -1;   // (the slack behind the buffer holds NULs)
    launch_nul_offsets(0, db.as<uint8_t>(), n_bytes, doff.as<int64_t>(), n_reads_max, dfound.as<int64_t>(), dtmp.p);
    return ran() && doff.down(off, (size_t)off_n * 8) && dfound.down(n_found, 8) ? 0 : -1;
}
extern "C" int useed_encode(uint8_t* buf, int64_t n)
{
    if (n < 0) return -2;
    DBuf db;
    if (!db.up(buf, (size_t)n)) return -1;
    launch_encode(0, db.as<uint8_t>(), n);
    return ran() && db.down(buf, (size_t)n) ? 0 : -1;
}
