// k_post.hip -- region post-processing and record generation, one lane per read.
//
// Replaces, for the reference call at jnibwa.c:214, upstream bwamem.c mem_sort_dedup_patch /
// mem_patch_reg (row a13), mem_mark_primary_se (a14), mem_reg2aln + bwa.c bwa_gen_cigar2 +
// ksw.c ksw_global2 (a15), mem_approx_mapq_se (a16), mem_reg2sam + bwamem_extra.c mem_gen_alt
// (a17), and the reference's own record hook fmt_BAMish / bufLen (jnibwa.c:43-124, a18).
// These stages are branchy and tiny next to seeding and extension; they stay on the device
// so a batch never round-trips through the host between kernels.
#include "dev_common.h"
#include "kernels.h"
#include "post_common.h"
#include "bgzf_deflate.h"
#include "bgzf_inflate.h"
#include "bam_sort.h"
#include "fastq_parse.h"

// WAVE_PER_READ = false: one lane per read.  true (tiles of long reads): one wavefront per read -- sixty-four times the waves
// in flight for this latency-bound stage -- with lane 0 doing the updates and the banded global alignments of region
// patching spread across the lanes (sort_dedup_patch_wave / global_score_wave; rings in dynamic LDS).
template <bool WAVE_PER_READ>
__global__ void __launch_bounds__(64, WAVE_PER_READ ? 3 : 6) k_post1(DevIndex ix, MemOpt opt, TileView tv, int ring)
{
    HIP_DYNAMIC_SHARED(int32_t, smem)
    const int r = WAVE_PER_READ ? (int)blockIdx.x : (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (r >= tv.n_reads) return;
    const bool writer = !WAVE_PER_READ || threadIdx.x == 0;
    WaveDp wd; wd.eh_h = smem; wd.eh_e = smem + ring; wd.tmpM = smem + 2 * ring; wd.rm = ring - 1; wd.lane = (int)threadIdx.x; wd.no_pk = (tv.debug & 0x10000) != 0;
    PostScratch S = post_scratch_for(tv, r);
    const uint8_t* query = tv.seq + tv.seq_off[r];
    AlnReg* a = tv.regs + tv.seed_off[r];
    {   // regions must be sane before any loop is sized from them: fail the call loudly instead of spinning
        const int l_query = (int)(tv.seq_off[r + 1] - tv.seq_off[r] - 1);
        const int n0 = tv.n_regs[r];
        bool bad = n0 < 0 || n0 > tv.seed_off[r + 1] - tv.seed_off[r];
        for (int i = 0; !bad && i < n0; ++i)
            bad = a[i].qb < 0 || a[i].qe < a[i].qb || a[i].qe > l_query || a[i].rb < 0 || a[i].re < a[i].rb || a[i].re > ix.l_pac << 1
               || a[i].re - a[i].rb > 4 * (int64_t)l_query + 1024 || a[i].rid < 0 || a[i].rid >= ix.n_seqs;
        if (bad) {
            if (writer && !(atomicOr(tv.err, ERR_BAD_REG) & ERR_BAD_REG)) { tv.err[1] = r; tv.err[2] = n0; if (n0 > 0) { tv.err[3] = a[0].qb; tv.err[4] = a[0].qe; tv.err[5] = (int)a[0].rb; tv.err[6] = (int)a[0].re; tv.err[7] = a[0].score; } }
            if (WAVE_PER_READ) __syncthreads();
            if (writer) tv.n_regs[r] = 0;
            return;
        }
    }
    if (tv.debug & 0xff) printf("[k] post1 read %d n=%d\n", r, tv.n_regs[r]);
    const int n_in = tv.n_regs[r];
    if (WAVE_PER_READ) __syncthreads();                              // every lane has read the count before lane 0 replaces it
    SortKey* keys = (tv.debug & 0x400) ? nullptr : sort_keys_for(tv, r);          // BWAMEM_HIP_DEBUGK=1024: sort the regions themselves (tests)
    int n = WAVE_PER_READ ? sort_dedup_patch_wave(ix, opt, S, query, n_in, a, wd, keys) : sort_dedup_patch(ix, opt, S, query, n_in, a, tv.debug & 0xff, keys);
    if (tv.debug & 0xff) printf("[k] post1 read %d done n=%d\n", r, n);
    if (writer)
        for (int i = 0; i < n; ++i)
            if (a[i].rid >= 0 && ix.ann_is_alt[a[i].rid]) a[i].is_alt = 1;
    if (writer) tv.n_regs[r] = n;
    if (S.err && writer) atomicOr(tv.err, S.err);
}

// ------------------------------------------------------------------ single-end finalisation
// step 1: primary marking, and a job for every region whose record (or XA entry) needs a banded global alignment
__global__ void __launch_bounds__(64, 6) k_final_prep(DevIndex ix, MemOpt opt, TileView tv)
{
    int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= tv.n_reads) return;
    AlnReg* a = tv.regs + tv.seed_off[r];
    const int n = tv.n_regs[r];
    int32_t* zbuf = (int32_t*)(tv.srt + tv.seed_off[r]);      // >= 2 ints per region
    mark_primary_se(opt, n, a, tv.read_id0 + r, zbuf, (tv.debug & 0x400) ? nullptr : sort_keys_for(tv, r));
    if (opt.flag & MEM_F_PRIMARY5) reorder_primary5(opt.T, n, a);
    int32_t *cnt = 0, *has_alt = 0;
    if (!(opt.flag & MEM_F_ALL) && n > 0) {
        cnt = zbuf; has_alt = zbuf + n;
        if (xa_prepare(opt, n, a, cnt, has_alt) == 0) cnt = has_alt = 0;
    }
    DpJob* jobs = (DpJob*)tv.jobs;
    for (int k = 0; k < n; ++k) {
        AlnReg* p = &a[k];
        p->pad_ = 0;
        // will mem_reg2sam emit a record for it?
        bool rec = !(p->score < opt.T) && !(p->secondary >= 0 && (p->is_alt || !(opt.flag & MEM_F_ALL)))
                && !(p->secondary >= 0 && p->secondary < INT_MAX_ && (float)p->score < (float)a[p->secondary].score * opt.drop_ratio);
        // will mem_gen_alt list it in an XA tag?
        bool xa = false;
        if (cnt) {
            int pr = get_pri_idx(opt.XA_drop_ratio, a, k);
            xa = pr >= 0 && !(cnt[pr] > opt.max_XA_hits_alt || (!has_alt[pr] && cnt[pr] > opt.max_XA_hits));
        }
        if ((rec || xa) && region_needs_dp(opt, *p)) {
            // (one slot per reservation: every slot below job_cap that was handed out gets written, so an overflow leaves no
            // unwritten slot behind -- unlike the several-slot reservations of k_pe_rescue_plan / k_rescore_plan)
            int job = atomicAdd(tv.job_cnt, 1);
            if (job < tv.job_cap) { DpJob jb; jb.read = r; jb.reg = k; jobs[job] = jb; p->pad_ = job + 1; }
            else atomicOr(tv.err, ERR_JOB_CAP);
        }
    }
}

// step 3 (after k_gcigar): mem_reg2sam record selection and the reference's fmt_BAMish record writer
// (64, 6): a tile's 6 144 waves are six per SIMD; with the default register budget only four would be resident, and this stage
// waits on dependent loads most of the time
__global__ void __launch_bounds__(64, 6) k_final_se(DevIndex ix, MemOpt opt, TileView tv, JobView jv)
{
    int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= tv.n_reads) return;
    PostScratch S = post_scratch_for(tv, r);
    const uint8_t* query = tv.seq + tv.seq_off[r];
    int l_query = (int)(tv.seq_off[r + 1] - tv.seq_off[r] - 1);
    AlnReg* a = tv.regs + tv.seed_off[r];
    int n = tv.n_regs[r];
    int32_t* zbuf = (int32_t*)(tv.srt + tv.seed_off[r]);
    OutBuf ob; ob.p = tv.out + (size_t)r * tv.out_cap; ob.cap = tv.out_cap; ob.len = 0; ob.ovf = false;

    reg2sam(ix, opt, S, ob, l_query, query, n, a, zbuf, 0, (const MateInfo*)0, &jv);

    tv.out_len[r] = ob.ovf ? 0 : ob.len;
    if (ob.ovf) atomicOr(tv.err, ERR_OUT_CAP);
    if (S.err) atomicOr(tv.err, S.err);
}

// gather the per-read staging slots into one contiguous result buffer
__global__ void k_pack(TileView tv, uint8_t* dst)
{
    int r = blockIdx.x * (blockDim.x >> 3) + (threadIdx.x >> 3);   // 8 lanes per read
    int sub = threadIdx.x & 7;
    if (r >= tv.n_reads) return;
    const uint32_t* src = (const uint32_t*)(tv.out + (size_t)r * tv.out_cap);
    uint32_t* d = (uint32_t*)(dst + tv.out_off[r]);
    int nw = tv.out_len[r] >> 2;
    for (int i = sub; i < nw; i += 8) d[i] = src[i];
}

// ------------------------------------------------------------------ BAM records from the packed response (bam_encode.h)
// Three steps like k_final_se / launch_scan / k_pack: the bytes of every read's records, a scan, and the records themselves.
// step 1: one lane per read walks the read's response records and adds up the sizes of their BAM records.  TAGS: with the optional
// tags, whose sizes come from the reads' BamTagInfo (k_bam_tag_size of every tile has run, and the scan of the side texts)
template <bool TAGS>
__global__ void __launch_bounds__(64) k_bam_size(BamTile t)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= t.n_reads) return;
    const int64_t lo = t.resp_off[r], hi = t.resp_off[r + 1];
    int64_t total = 0;
    int err = 0;
    if (hi > lo) {                                                   // (an odd trailing read of a paired call has no bytes: no record)
        const uint32_t* p = (const uint32_t*)(t.resp + lo);
        const int64_t n = (hi - lo) >> 2;
        const int32_t l_read = (int32_t)(t.raw_off[r + 1] - t.raw_off[r] - 1);
        const int32_t n_aln = (int32_t)p[0];
        int64_t at = 1, sa_at = 0;
        if (n_aln < 0 || l_read < 0 || ((hi - lo) & 3)) err = BAM_ERR_PARSE;
        for (int32_t k = 0; k < n_aln && !err; ++k) {
            BamRec R;
            err = bam_parse<TAGS>(p + at, n - at, k, l_read, t.n_seqs, R);
            if (err) break;
            bam_name(t, r, R);
            if (TAGS) sa_at += bam_tags(t, r, R, sa_at);
            if (bam_layout<TAGS>(R) < 0) { err = BAM_ERR_SPAN; break; }
            total += R.total; at += R.words;
        }
        if (!err && at != n) err = BAM_ERR_PARSE;
        if (!err && total > 0x7fffffff) err = BAM_ERR_SPAN;
    }
    t.sizes[r] = err ? 0 : (int32_t)total;
    if (err) atomicOr(t.err, err);
}

// The side text of the optional tags (bam_encode.h: BamTagInfo), by the same three steps.  Step 1, one lane per read: what the read's
// text will hold.  A read whose response does not parse gets no text; k_bam_size meets the same error and flags it.
__global__ void __launch_bounds__(64) k_bam_tag_size(BamTile t)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= t.n_reads) return;
    const int64_t lo = t.resp_off[r], hi = t.resp_off[r + 1];
    BamTagInfo info; info.mate = info.l_mc = info.n_sa = info.l_sa = 0;
    int64_t l_sa = 0;
    int err = 0;
    if (hi > lo) {
        const uint32_t* p = (const uint32_t*)(t.resp + lo);
        const int64_t n = (hi - lo) >> 2;
        const int32_t l_read = (int32_t)(t.raw_off[r + 1] - t.raw_off[r] - 1);
        const int32_t n_aln = (int32_t)p[0];
        int64_t at = 1;
        if (n_aln < 0 || l_read < 0 || ((hi - lo) & 3)) err = BAM_ERR_PARSE;
        for (int32_t k = 0; k < n_aln && !err; ++k) {
            BamRec R;
            err = bam_parse<true>(p + at, n - at, k, l_read, t.n_seqs, R);
            if (err) break;
            if (bam_sa_listed(R)) { ++info.n_sa; l_sa += bam_sa_entry_len(t, R); }
            if (k == 0 && R.mapped) { info.mate = 0x100 | R.mapq; if (t.paired && (t.tags & BAM_TAG_MC)) info.l_mc = R.l_cigtxt; }
            at += R.words;
        }
        if (!err && l_sa + info.l_mc > 0x7fffffff) err = BAM_ERR_SPAN;
    }
    if (err) { info.mate = info.l_mc = info.n_sa = 0; l_sa = 0; if (err == BAM_ERR_SPAN) atomicOr(t.err, err); }
    if ((t.tags & BAM_TAG_SA) && info.n_sa >= 2) info.l_sa = (int32_t)l_sa;
    t.tag_info[t.read0 + r] = info;
    t.tag_sizes[t.read0 + r] = info.l_sa + info.l_mc;
}

// step 3, by the lane groups of k_bam_emit: the entries of the read's listed records, then record 0's CIGAR.  Nothing is written
// outside the bytes step 1 counted.
template <int G>
__global__ void __launch_bounds__(256) k_bam_tag_text(BamTile t)
{
    const int r = blockIdx.x * (256 / G) + ((int)threadIdx.x / G), sub = (int)threadIdx.x % G;
    if (r >= t.n_reads) return;
    const int64_t g = (int64_t)t.read0 + r;
    const BamTagInfo info = t.tag_info[g];
    const int64_t lo = t.resp_off[r], hi = t.resp_off[r + 1];
    if (hi <= lo || info.l_sa + info.l_mc <= 0 || t.tag_off[g + 1] - t.tag_off[g] != (int64_t)info.l_sa + info.l_mc) return;
    uint8_t* dst = t.tag_text + t.tag_off[g];
    const uint32_t* p = (const uint32_t*)(t.resp + lo);
    const int64_t n = (hi - lo) >> 2;
    const int32_t l_read = (int32_t)(t.raw_off[r + 1] - t.raw_off[r] - 1);
    const int32_t n_aln = (int32_t)p[0];
    int64_t at = 1, o = 0;
    for (int32_t k = 0; k < n_aln; ++k) {
        BamRec R;
        if (bam_parse<true>(p + at, n - at, k, l_read, t.n_seqs, R)) return;
        if (k == 0 && info.l_mc > 0 && R.mapped && R.l_cigtxt == info.l_mc) bam_put_cigar(dst + info.l_sa, R, sub, G);
        if (info.l_sa > 0 && bam_sa_listed(R)) {
            const int64_t len = bam_sa_entry_len(t, R);
            if (o + len > info.l_sa) return;
            bam_put_sa_entry(dst + o, t, R, sub, G);
            o += len;
        }
        at += R.words;
    }
}

// step 3: G lanes per read (8, or the wavefront for tiles of long reads) write the read's records.  Every lane parses the record
// (the same few words for all of them); the lanes then share out the aligned 32-bit words of the record's span in the output,
// each assembled in a register from bam_byte and stored whole.  Only the up to three bytes before the first aligned word
// and after the last are stored singly.  Q: the batch carries qualities (the instantiation without them has no load for QUAL).
// TAGS: SA / MC / MQ are asked for; their text comes from the side buffer (k_bam_tag_text) through the same word assembly.
template <int G, bool Q, bool TAGS>
__global__ void __launch_bounds__(256) k_bam_emit(BamTile t)
{
    const int r = blockIdx.x * (256 / G) + ((int)threadIdx.x / G), sub = (int)threadIdx.x % G;
    if (r >= t.n_reads) return;
    const int64_t lo = t.resp_off[r], hi = t.resp_off[r + 1];
    int64_t o = t.out_off[r];
    const int64_t o_end = t.out_off[r + 1];
    if (hi <= lo || o_end <= o) return;                              // no record (or refused by the size kernel, which flagged it)
    const uint32_t* p = (const uint32_t*)(t.resp + lo);
    const int64_t n = (hi - lo) >> 2;
    const uint8_t* raw = t.raw + t.raw_off[r];
    const uint8_t* qual = Q ? t.qual + t.raw_off[r] : nullptr;
    const int32_t l_read = (int32_t)(t.raw_off[r + 1] - t.raw_off[r] - 1);
    const int32_t n_aln = (int32_t)p[0];
    int64_t at = 1, sa_at = 0;
    for (int32_t k = 0; k < n_aln; ++k) {
        BamRec R;
        int err = bam_parse<TAGS>(p + at, n - at, k, l_read, t.n_seqs, R);
        if (!err) {
            bam_name(t, r, R);
            if (TAGS) sa_at += bam_tags(t, r, R, sa_at);
            if (bam_layout<TAGS>(R) < 0 || o + R.total > o_end) err = BAM_ERR_SPAN;                            // never outside the read's span
        }
        if (err) { if (sub == 0) atomicOr(t.err, err); return; }
        uint8_t* dst = t.out + o;
        const int32_t lead = (int32_t)((4 - (o & 3)) & 3), head = R.total < lead ? R.total : lead;
        const int32_t nw = (R.total - head) >> 2, tail = R.total - head - 4 * nw;
        if (sub < head) dst[sub] = bam_byte<TAGS>(R, raw, sub, qual);
        uint32_t* dw = (uint32_t*)(dst + head);
        for (int32_t w = sub; w < nw; w += G) {
            const int32_t i = head + 4 * w;
            dw[w] = (uint32_t)bam_byte<TAGS>(R, raw, i, qual) | (uint32_t)bam_byte<TAGS>(R, raw, i + 1, qual) << 8 | (uint32_t)bam_byte<TAGS>(R, raw, i + 2, qual) << 16 | (uint32_t)bam_byte<TAGS>(R, raw, i + 3, qual) << 24;
        }
        if (sub < tail) dst[head + 4 * nw + sub] = bam_byte<TAGS>(R, raw, head + 4 * nw + sub, qual);
        o += R.total; at += R.words;
    }
}

// the qualities handed to bwamem_hip_batch_set_qualities against the reads, one lane per read: a NUL where the read's NUL is,
// every other byte in 33..126.  err: FASTQ_NO_ERROR - the smallest offending read (0: none)
__global__ void __launch_bounds__(64) k_qual_check(const uint8_t* raw, const uint8_t* qual, const int64_t* raw_off, int n_reads, int32_t* err)
{
    const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (r >= n_reads) return;
    const int64_t lo = raw_off[r], hi = raw_off[r + 1] - 1;
    bool bad = hi < lo || qual[hi] != 0;
    for (int64_t i = lo; i < hi && !bad; ++i) bad = qual[i] < 33 || qual[i] > 126;
    if (bad) atomicMax(err, FASTQ_NO_ERROR - r);
}

// the names of the two reads of every pair must be equal (paired calls on batches with names of their own), one lane per pair
__global__ void __launch_bounds__(64) k_mate_names(const uint8_t* names, const int64_t* name_off, int n_pairs, int32_t* err)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n_pairs) return;
    const int64_t a = name_off[2 * i], b = name_off[2 * i + 1], l = b - a;
    bool bad = name_off[2 * i + 2] - b != l;
    for (int64_t k = 0; k < l && !bad; ++k) bad = names[a + k] != names[b + k];
    if (bad) atomicMax(err, FASTQ_NO_ERROR - 2 * i);
}

// ------------------------------------------------------------------ FASTQ text taken apart on the device (fastq_parse.h)
// the newlines among the lane's FASTQ_LANE_BYTES positions from p0 (one 16-byte load where the text covers them all), as a bit per
// position
static __device__ inline uint32_t fastq_lane_newlines(const uint8_t* text, int64_t n, int64_t p0)
{
    uint32_t m = 0;
    if (p0 + FASTQ_LANE_BYTES <= n) {
        const uint4 v = *(const uint4*)(text + p0);
        const uint32_t w[4] = { v.x, v.y, v.z, v.w };
        for (int k = 0; k < 4; ++k) {
            const uint32_t b = fastq_newline_bits(w[k]);
            m |= ((b >> 7 & 1) | (b >> 14 & 2) | (b >> 21 & 4) | (b >> 28 & 8)) << (4 * k);
        }
    } else
        for (int k = 0; k < FASTQ_LANE_BYTES && p0 + k <= n; ++k) m |= (uint32_t)fastq_newline_at(text, n, p0 + k) << k;
    return m;
}

// (a) the newlines of every chunk
__global__ void __launch_bounds__(FASTQ_THREADS) k_fastq_count(const uint8_t* text, int64_t n, int32_t* counts)
{
    __shared__ int s_w[FASTQ_THREADS / 64];
    const int tid = (int)threadIdx.x;
    int c = __popc(fastq_lane_newlines(text, n, (int64_t)blockIdx.x * FASTQ_CHUNK + (int64_t)tid * FASTQ_LANE_BYTES));
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((tid & 63) == 0) s_w[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) { int tot = 0; for (int w = 0; w < FASTQ_THREADS / 64; ++w) tot += s_w[w]; counts[blockIdx.x] = tot; }
}

// (c) the start of every line: the number of a newline is its chunk's base plus a workgroup scan of the lanes' counts
__global__ void __launch_bounds__(FASTQ_THREADS) k_fastq_starts(FastqText t)
{
    __shared__ int s_w[FASTQ_THREADS / 64];
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t p0 = (int64_t)blockIdx.x * FASTQ_CHUNK + (int64_t)tid * FASTQ_LANE_BYTES;
    uint32_t m = fastq_lane_newlines(t.text, t.n, p0);
    const int c = __popc(m);
    int incl = c;
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(incl, o); if (lane >= o) incl += u; }
    if (lane == 63) s_w[wv] = incl;
    __syncthreads();
    int pre = 0;
    for (int w = 0; w < wv; ++w) pre += s_w[w];
    int64_t j = t.chunk_base[blockIdx.x] + pre + incl - c + 1;       // the number of the lane's first newline
    if (blockIdx.x == 0 && tid == 0 && t.n_lines >= 0) t.start[0] = 0;
    for (; m; m &= m - 1, ++j)
        if (j <= t.n_lines) t.start[j] = p0 + (__ffsll((long long)m) - 1) + 1;       // never outside the index
}

// (d) one lane per record checks its four lines and writes the lengths of its read; the smallest offending read into the error word
__global__ void __launch_bounds__(64) k_fastq_records(FastqText t, FastqOut o)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= t.n_rec) return;
    const int64_t read = (int64_t)t.stride * i + t.phase;
    FastqRec R;
    if (fastq_record(t.text, t.start, i, R)) { o.len1[read] = R.l_seq + 1; o.l_name[read] = R.l_name; atomicMax(&o.err[1], R.l_seq); }
    else { o.len1[read] = 1; o.l_name[read] = 1; atomicMax(&o.err[0], (int32_t)(FASTQ_NO_ERROR - read)); }
}

// n bytes from src to dst by the G lanes of a group: the aligned 32-bit words of dst are assembled in a register and stored whole
// (src is at any alignment), the bytes before the first and after the last singly -- as k_bam_emit stores a record
template <int G>
static __device__ inline void fastq_copy_bytes(uint8_t* dst, const uint8_t* src, int32_t n, int sub)
{
    const int32_t lead = (int32_t)((4 - ((uintptr_t)dst & 3)) & 3), head = n < lead ? n : lead;
    const int32_t nw = (n - head) >> 2, tail = n - head - 4 * nw;
    if (sub < head) dst[sub] = src[sub];
    uint32_t* dw = (uint32_t*)(dst + head);
    for (int32_t w = sub; w < nw; w += G) {
        const uint8_t* s = src + head + 4 * w;
        dw[w] = (uint32_t)s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16 | (uint32_t)s[3] << 24;
    }
    if (sub < tail) dst[head + 4 * nw + sub] = src[head + 4 * nw + sub];
}

// (f) the lane groups of k_bam_emit: G lanes per record (8, or the wavefront for long reads) write its bases + NUL, its qualities +
// NUL at the same offset, and its name.  Runs only after every record has passed its check: the places come from the line index,
// the lengths from the scans.
template <int G>
__global__ void __launch_bounds__(256) k_fastq_copy(FastqText t, FastqOut o)
{
    const int i = blockIdx.x * (256 / G) + ((int)threadIdx.x / G), sub = (int)threadIdx.x % G;
    if (i >= t.n_rec) return;
    const int64_t read = (int64_t)t.stride * i + t.phase;
    const int64_t so = o.seq_off[read], no = o.name_off[read];
    const int64_t l_seq = o.seq_off[read + 1] - so - 1, l_name = o.name_off[read + 1] - no;
    const int64_t name = t.start[4 * (int64_t)i] + 1, seq = t.start[4 * (int64_t)i + 1], qual = t.start[4 * (int64_t)i + 3];
    if (l_seq < 0 || l_name < 0 || name + l_name > t.n || seq + l_seq > t.n || qual + l_seq > t.n) return;       // never outside the text
    fastq_copy_bytes<G>(o.seq + so, t.text + seq, (int32_t)l_seq, sub);
    fastq_copy_bytes<G>(o.qual + so, t.text + qual, (int32_t)l_seq, sub);
    fastq_copy_bytes<G>(o.names + no, t.text + name, (int32_t)l_name, sub);
    if (sub == 0) { o.seq[so + l_seq] = 0; o.qual[so + l_seq] = 0; }
}

// ------------------------------------------------------------------ BGZF members on the device (bgzf_deflate.h)
// One workgroup per member; a fixed grid walks the members, so the token scratch is one member's worth per workgroup.
//   1. CRC-32: every lane a slice, advanced over the rest of the input by x^(8 * bytes) and combined by XOR.
//   2. LZ77 in windows of BGZ_WIN positions.  Every position of a window looks up one candidate in the hash table (4-byte hash,
//      latest earlier position) and the run candidate at distance 1; the longer match wins, the run on a tie.  Only after the
//      whole window has looked, its positions enter the table by atomicMax of the position: the table then holds, per hash, the
//      last position of all earlier windows whichever lane stored last, so the matches are a function of the input alone.
//      Greedy token selection over the window: per chunk of 16 positions one lane computes where a token starting at each
//      position leaves the chunk (backwards), one lane chains the 64 chunks, then the chunks mark their token starts; a
//      wavefront scan turns the marks into token indices.  Tokens go to the workgroup's scratch in HBM, histograms to LDS.
//   3. Huffman: the used symbols are ranked by all lanes, one lane per alphabet builds the length-limited code, one lane
//      run-length-codes the lengths, builds the code-length code and adds up the exact size; stored wins if not larger.
//   4. The member -- header, block header, tokens, end of block, CRC-32, ISIZE -- is one bit stream: lanes OR their bits into a
//      staging area of LDS words at offsets from a workgroup scan, and complete words are stored to the slot as dwords.
#define BGZ_THREADS 256
#define BGZ_WIN 1024
#define BGZ_PER_LANE (BGZ_WIN / BGZ_THREADS)
#define BGZ_CHUNK 16
#define BGZ_HASH_BITS 13
#define BGZ_STAGE_DW 1544                  // a round of 1 024 tokens of at most 48 bits, and the carried word

static __device__ inline uint32_t bgz_ld32(const uint8_t* p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
static __device__ inline int bgz_hash(uint32_t v) { return (int)((v * 2654435761u) >> (32 - BGZ_HASH_BITS)); }
// number of equal leading bytes of a and b (a < b), at most maxl; b + maxl is within the member
static __device__ inline int bgz_match_len(const uint8_t* a, const uint8_t* b, int maxl)
{
    int k = 0;
    while (k + 4 <= maxl) {
        const uint32_t x = bgz_ld32(a + k) ^ bgz_ld32(b + k);
        if (x) return k + (__builtin_ctz(x) >> 3);
        k += 4;
    }
    while (k < maxl && a[k] == b[k]) ++k;
    return k;
}
// nb <= 32 bits of v at bit `bit` of the staging area: by any lane / by the one lane that writes alone
static __device__ inline void bgz_put(int* stage, uint32_t bit, uint32_t v, int nb)
{
    if (nb == 0) return;
    const uint32_t i = bit >> 5, sh = bit & 31;
    atomicOr(&stage[i], (int)(v << sh));
    if (sh + nb > 32) atomicOr(&stage[i + 1], (int)(v >> (32 - sh)));
}
static __device__ inline void bgz_put1(int* stage, uint32_t& bit, uint32_t v, int nb)
{
    const uint32_t i = bit >> 5, sh = bit & 31;
    stage[i] |= (int)(v << sh);
    if (sh + nb > 32) stage[i + 1] |= (int)(v >> (32 - sh));
    bit += nb;
}
// after a barrier behind the puts: the complete words of the staging area go to the slot, the last partial word is carried
static __device__ inline void bgz_flush(int* stage, uint32_t* out_dw, uint32_t& obits, uint32_t cb, int tid)
{
    const uint32_t total = (obits & 31) + cb, full = total >> 5;
    for (uint32_t k = tid; k < full; k += BGZ_THREADS) out_dw[(obits >> 5) + k] = (uint32_t)stage[k];
    const int carry = stage[full];
    __syncthreads();
    for (uint32_t k = tid; k <= full; k += BGZ_THREADS) stage[k] = k == 0 ? carry : 0;
    obits += cb;
    __syncthreads();
}

__global__ void __launch_bounds__(BGZ_THREADS) k_bgzf_deflate(const uint8_t* src, int64_t n_total, int n_blocks, uint8_t* slots, int32_t* sizes, uint32_t* tokens)
{
    __shared__ int s_hash[1 << BGZ_HASH_BITS];
    __shared__ uint16_t s_mlen[2][BGZ_WIN], s_mdist[2][BGZ_WIN], s_exit[BGZ_WIN];
    __shared__ uint16_t s_entry[BGZ_WIN / BGZ_CHUNK], s_cmask[BGZ_WIN / BGZ_CHUNK];
    __shared__ int s_cbase[BGZ_WIN / BGZ_CHUNK];
    __shared__ int s_hll[288], s_hd[32], s_hcl[32], s_cnt[3][16];
    __shared__ uint32_t s_tll[288], s_td[32], s_tcl[32];
    __shared__ uint8_t s_lenll[288], s_lend[32], s_lencl[32], s_seq[DFL_NLL + DFL_ND + 4];
    __shared__ uint16_t s_ordll[288], s_parll[2 * 288], s_ordd[32], s_pard[64], s_rle[DFL_NLL + DFL_ND + 4];
    __shared__ uint32_t s_wll[288], s_wd[32];
    __shared__ uint32_t s_crc[256], s_red[BGZ_THREADS];
    __shared__ int s_stage[BGZ_STAGE_DW];
    __shared__ int s_scan[BGZ_THREADS], s_gp[64];
    __shared__ int s_next, s_ntok, s_bits, s_mll, s_md, s_total, s_cb, s_dynamic, s_hlit, s_hdist, s_hclen, s_ncl, s_hbits, s_fix[2];

    const int tid = (int)threadIdx.x;
    uint32_t* toks = tokens + (size_t)blockIdx.x * BGZF_IN;
    for (int blk = (int)blockIdx.x; blk < n_blocks; blk += (int)gridDim.x) {
        const int64_t at = (int64_t)blk * BGZF_IN;
        const int n = (int)(n_total - at < BGZF_IN ? n_total - at : BGZF_IN);
        const uint8_t* in = src + at;
        uint32_t* out_dw = (uint32_t*)(slots + (size_t)blk * BGZF_SLOT);

        for (int k = tid; k < 1 << BGZ_HASH_BITS; k += BGZ_THREADS) s_hash[k] = 0;
        for (int k = tid; k < BGZ_STAGE_DW; k += BGZ_THREADS) s_stage[k] = 0;
        for (int k = tid; k < 288; k += BGZ_THREADS) { s_hll[k] = 0; s_lenll[k] = 0; }
        if (tid < 32) { s_hd[tid] = 0; s_hcl[tid] = 0; s_lend[tid] = 0; s_lencl[tid] = 0; }
        s_crc[tid] = bgz_crc_table_entry((uint32_t)tid);
        if (tid == 0) { s_next = 0; s_ntok = 0; s_bits = 0; s_mll = 0; s_md = 0; }
        __syncthreads();

        {   // ---- 1. CRC-32
            const int per = (n + BGZ_THREADS - 1) / BGZ_THREADS, lo = tid * per, hi = lo + per < n ? lo + per : n;
            uint32_t x = 0;
            if (lo < n) {
                uint32_t c = lo == 0 ? 0xffffffffu : 0u;
                for (int p = lo; p < hi; ++p) c = s_crc[(c ^ in[p]) & 0xff] ^ (c >> 8);
                x = bgz_crc_mul(c, bgz_crc_xpow8((uint32_t)(n - hi)));
            }
            s_red[tid] = x;
        }

        // ---- 2. LZ77
        for (int w0 = 0, par = 0; w0 < n; w0 += BGZ_WIN, par ^= 1) {
            const int wn = n - w0 < BGZ_WIN ? n - w0 : BGZ_WIN;
            const bool active = s_next < w0 + wn;                    // (uniform) a token starts in this window
            int hv[BGZ_PER_LANE];
#pragma unroll
            for (int j = 0; j < BGZ_PER_LANE; ++j) {
                const int i = j * BGZ_THREADS + tid, p = w0 + i;
                hv[j] = i < wn && p + 4 <= n ? bgz_hash(bgz_ld32(in + p)) : -1;
                if (!active || i >= wn) continue;
                const int maxl = n - p < DFL_MAX_MATCH ? n - p : DFL_MAX_MATCH;
                int bl = 0, bd = 0;
                if (maxl >= DFL_MIN_MATCH) {
                    if (hv[j] >= 0) {
                        const int c = s_hash[hv[j]] - 1;
                        if (c >= 0 && p - c <= DFL_MAX_DIST) { const int l = bgz_match_len(in + c, in + p, maxl); if (l >= 4) { bl = l; bd = p - c; } }
                    }
                    if (p >= 1 && in[p - 1] == in[p]) { const int l = bgz_match_len(in + p - 1, in + p, maxl); if (l >= DFL_MIN_MATCH && l >= bl) { bl = l; bd = 1; } }
                }
                s_mlen[par][i] = (uint16_t)bl; s_mdist[par][i] = (uint16_t)bd;
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < BGZ_PER_LANE; ++j)
                if (hv[j] >= 0) atomicMax(&s_hash[hv[j]], w0 + j * BGZ_THREADS + tid + 1);
            if (active && tid < BGZ_WIN / BGZ_CHUNK) {               // where a token starting at i leaves the chunk
                const int lo = tid * BGZ_CHUNK, hi = lo + BGZ_CHUNK < wn ? lo + BGZ_CHUNK : wn;
                for (int i = hi - 1; i >= lo; --i) {
                    const int l = s_mlen[par][i], nx = i + (l ? l : 1);
                    s_exit[i] = (uint16_t)(nx >= hi ? nx : s_exit[nx]);
                }
            }
            __syncthreads();
            if (active && tid == 0) {                                // the chunks a token starts in, and where
                int e = s_next - w0;
                for (int c = 0; c * BGZ_CHUNK < wn; ++c) {
                    const int hi = (c + 1) * BGZ_CHUNK < wn ? (c + 1) * BGZ_CHUNK : wn;
                    if (e < hi) { s_entry[c] = (uint16_t)e; e = s_exit[e]; } else s_entry[c] = 0xffff;
                }
                s_next = w0 + e;
            }
            __syncthreads();
            if (active && tid < BGZ_WIN / BGZ_CHUNK) {               // token starts of the chunk, and the index of its first token
                const int lo = tid * BGZ_CHUNK, hi = lo + BGZ_CHUNK < wn ? lo + BGZ_CHUNK : wn;
                const int base = s_ntok;
                uint32_t mask = 0;
                if (lo < wn) {
                    int i = s_entry[tid];
                    if (i != 0xffff) while (i < hi) { mask |= 1u << (i - lo); const int l = s_mlen[par][i]; i += l ? l : 1; }
                }
                const int cnt = __popc(mask);
                int incl = cnt;
                for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(incl, o); if (tid >= o) incl += u; }
                s_cmask[tid] = (uint16_t)mask; s_cbase[tid] = base + incl - cnt;
                if (tid == 63) s_ntok = base + incl;
            }
            __syncthreads();
            if (active) {
#pragma unroll
                for (int j = 0; j < BGZ_PER_LANE; ++j) {
                    const int i = j * BGZ_THREADS + tid, c = i / BGZ_CHUNK, b = i % BGZ_CHUNK;
                    if (i >= wn) continue;
                    const uint32_t mask = s_cmask[c];
                    if (!(mask >> b & 1)) continue;
                    const int k = s_cbase[c] + __popc(mask & ((1u << b) - 1));
                    const int l = s_mlen[par][i];
                    if (l) {
                        const int d = s_mdist[par][i];
                        toks[k] = dfl_tok_match(l, d);
                        atomicAdd(&s_hll[dfl_len_sym(l)], 1); atomicAdd(&s_hd[dfl_dist_sym(d)], 1);
                    } else {
                        const uint8_t v = in[w0 + i];
                        toks[k] = v;
                        atomicAdd(&s_hll[v], 1);
                    }
                }
            }
        }
        __syncthreads();

        // ---- 3. Huffman codes
        if (tid == 0) {
            s_hll[DFL_EOB] = 1;
            int used = 0;
            for (int s = 0; s < DFL_ND; ++s) used += s_hd[s] > 0;
            s_fix[0] = s_fix[1] = 0;                                   // fewer than two distance symbols: symbols 0 and 1 fill in, unused by any token
            if (used < 2 && s_hd[0] == 0) { s_hd[0] = 1; s_fix[0] = 1; ++used; }
            if (used < 2 && s_hd[1] == 0) { s_hd[1] = 1; s_fix[1] = 1; ++used; }
        }
        __syncthreads();
        for (int s = tid; s < DFL_NLL; s += BGZ_THREADS) if (s_hll[s] > 0) { s_ordll[dfl_rank(s_hll, DFL_NLL, s)] = (uint16_t)s; atomicAdd(&s_mll, 1); }
        if (tid < DFL_ND && s_hd[tid] > 0) { s_ordd[dfl_rank(s_hd, DFL_ND, tid)] = (uint16_t)tid; atomicAdd(&s_md, 1); }
        __syncthreads();
        if (tid == 0) { dfl_code_lengths(s_hll, s_ordll, s_mll, DFL_LL_BITS, s_lenll, s_cnt[0], s_wll, s_parll); dfl_assign_codes(s_lenll, DFL_NLL, DFL_LL_BITS, s_cnt[0], s_tll); }
        if (tid == 64) { dfl_code_lengths(s_hd, s_ordd, s_md, DFL_LL_BITS, s_lend, s_cnt[1], s_wd, s_pard); dfl_assign_codes(s_lend, DFL_ND, DFL_LL_BITS, s_cnt[1], s_td); }
        __syncthreads();
        {   // the bits of the tokens and the end-of-block symbol
            int bits = 0;
            for (int s = tid; s < DFL_NLL; s += BGZ_THREADS) bits += s_hll[s] * ((int)s_lenll[s] + dfl_len_extra_bits(s));
            if (tid < DFL_ND) bits += (s_hd[tid] - (tid < 2 ? s_fix[tid] : 0)) * ((int)s_lend[tid] + dfl_dist_extra_bits(tid));
            if (bits) atomicAdd(&s_bits, bits);
        }
        if (tid == 0) {                                              // the block header: lengths, run-length coded (RFC 1951 3.2.7)
            int hlit = DFL_NLL, hdist = DFL_ND;
            while (hlit > 257 && !s_lenll[hlit - 1]) --hlit;
            while (hdist > 1 && !s_lend[hdist - 1]) --hdist;
            for (int s = 0; s < hlit; ++s) s_seq[s] = s_lenll[s];
            for (int s = 0; s < hdist; ++s) s_seq[hlit + s] = s_lend[s];
            const int ncl = dfl_rle_lengths(s_seq, hlit + hdist, s_rle);
            for (int k = 0; k < ncl; ++k) ++s_hcl[s_rle[k] & 0xff];
            int m = 0;
            for (int s = 0; s < DFL_NCL; ++s) m += s_hcl[s] > 0;
            if (m < 2) { if (s_hcl[0] == 0) { s_hcl[0] = 1; ++m; } if (m < 2) { s_hcl[1] = 1; ++m; } }
            for (int s = 0; s < DFL_NCL; ++s) if (s_hcl[s] > 0) s_ordd[dfl_rank(s_hcl, DFL_NCL, s)] = (uint16_t)s;
            dfl_code_lengths(s_hcl, s_ordd, m, DFL_CL_BITS, s_lencl, s_cnt[2], s_wd, s_pard);
            dfl_assign_codes(s_lencl, DFL_NCL, DFL_CL_BITS, s_cnt[2], s_tcl);
            int hclen = DFL_NCL;
            while (hclen > 4 && !s_lencl[dfl_cl_order(hclen - 1)]) --hclen;
            int hbits = 3 + 5 + 5 + 4 + 3 * hclen;
            for (int k = 0; k < ncl; ++k) { const int sym = s_rle[k] & 0xff; hbits += (int)s_lencl[sym] + dfl_cl_extra_bits(sym); }
            s_hlit = hlit; s_hdist = hdist; s_hclen = hclen; s_ncl = ncl; s_hbits = hbits;
        }
        __syncthreads();

        // ---- 4. the member
        if (tid == 0) {
            const int dyn_bytes = (s_hbits + s_bits + 7) >> 3, stored_bytes = n + 5;
            const int dynamic = dyn_bytes < stored_bytes;
            const int member = BGZF_HEAD + (dynamic ? dyn_bytes : stored_bytes) + BGZF_TAIL;
            s_dynamic = dynamic;
            uint32_t bit = 0;
            bgz_put1(s_stage, bit, 0x04088b1fu, 32); bgz_put1(s_stage, bit, 0, 32);            // ID1 ID2 CM FLG, MTIME
            bgz_put1(s_stage, bit, 0x0006ff00u, 32);                                           // XFL, OS, XLEN
            bgz_put1(s_stage, bit, 0x00024342u, 32);                                           // 'B' 'C', SLEN
            bgz_put1(s_stage, bit, (uint32_t)(member - 1), 16);                                // BSIZE
            if (dynamic) {
                bgz_put1(s_stage, bit, 1, 1); bgz_put1(s_stage, bit, 2, 2);
                bgz_put1(s_stage, bit, (uint32_t)(s_hlit - 257), 5); bgz_put1(s_stage, bit, (uint32_t)(s_hdist - 1), 5); bgz_put1(s_stage, bit, (uint32_t)(s_hclen - 4), 4);
                for (int i = 0; i < s_hclen; ++i) bgz_put1(s_stage, bit, s_lencl[dfl_cl_order(i)], 3);
                for (int k = 0; k < s_ncl; ++k) {
                    const int sym = s_rle[k] & 0xff;
                    const uint32_t e = s_tcl[sym];
                    bgz_put1(s_stage, bit, e & 0xffff, (int)(e >> 16));
                    if (sym >= 16) bgz_put1(s_stage, bit, (uint32_t)(s_rle[k] >> 8), dfl_cl_extra_bits(sym));
                }
            } else {
                bgz_put1(s_stage, bit, 1, 1); bgz_put1(s_stage, bit, 0, 2);
                bit = (bit + 7) & ~7u;
                bgz_put1(s_stage, bit, (uint32_t)n, 16); bgz_put1(s_stage, bit, ~(uint32_t)n & 0xffff, 16);
            }
            s_cb = (int)bit;
        }
        __syncthreads();
        uint32_t obits = 0;
        bgz_flush(s_stage, out_dw, obits, (uint32_t)s_cb, tid);
        const int dynamic = s_dynamic, n_items = dynamic ? s_ntok : n;
        for (int base = 0; base < n_items; base += 4 * BGZ_THREADS) {
            uint32_t a[4], b[4]; int na[4], nb[4];
            int mine = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k = base + 4 * tid + q;
                a[q] = b[q] = 0; na[q] = nb[q] = 0;
                if (k >= n_items) continue;
                if (!dynamic) { a[q] = in[k]; na[q] = 8; }
                else {
                    const uint32_t t = toks[k];
                    if (t & DFL_TOK_MATCH) {
                        const int l = dfl_tok_len(t), d = dfl_tok_dist(t), ls = dfl_len_sym(l), ds = dfl_dist_sym(d);
                        const uint32_t el = s_tll[ls], ed = s_td[ds];
                        const int xl = dfl_len_extra_bits(ls), xd = dfl_dist_extra_bits(ds);
                        a[q] = (el & 0xffff) | (uint32_t)dfl_len_extra(l, xl) << (el >> 16); na[q] = (int)(el >> 16) + xl;
                        b[q] = (ed & 0xffff) | (uint32_t)dfl_dist_extra(d, xd) << (ed >> 16); nb[q] = (int)(ed >> 16) + xd;
                    } else { const uint32_t e = s_tll[t]; a[q] = e & 0xffff; na[q] = (int)(e >> 16); }
                }
                mine += na[q] + nb[q];
            }
            // exclusive scan of the lanes' bit counts: groups of four lanes by wavefront 0, the rest from LDS
            s_scan[tid] = mine;
            __syncthreads();
            if (tid < 64) {
                const int g = s_scan[4 * tid] + s_scan[4 * tid + 1] + s_scan[4 * tid + 2] + s_scan[4 * tid + 3];
                int incl = g;
                for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(incl, o); if (tid >= o) incl += u; }
                s_gp[tid] = incl - g;
                if (tid == 63) s_total = incl;
            }
            __syncthreads();
            uint32_t bit = (obits & 31) + (uint32_t)s_gp[tid >> 2];
            for (int q = 0; q < (tid & 3); ++q) bit += (uint32_t)s_scan[(tid & ~3) + q];
#pragma unroll
            for (int q = 0; q < 4; ++q) { bgz_put(s_stage, bit, a[q], na[q]); bit += na[q]; bgz_put(s_stage, bit, b[q], nb[q]); bit += nb[q]; }
            __syncthreads();
            bgz_flush(s_stage, out_dw, obits, (uint32_t)s_total, tid);
        }
        if (tid == 0) {                                              // end of block, CRC-32, ISIZE
            uint32_t bit = obits & 31;
            if (dynamic) { const uint32_t e = s_tll[DFL_EOB]; bgz_put1(s_stage, bit, e & 0xffff, (int)(e >> 16)); }
            bit = (bit + 7) & ~7u;
            uint32_t crc = 0;
            for (int k = 0; k < BGZ_THREADS; ++k) crc ^= s_red[k];
            bgz_put1(s_stage, bit, ~crc, 32); bgz_put1(s_stage, bit, (uint32_t)n, 32);
            s_cb = (int)(bit - (obits & 31));
        }
        __syncthreads();
        bgz_flush(s_stage, out_dw, obits, (uint32_t)s_cb, tid);
        if (tid == 0) {
            if (obits & 31) out_dw[obits >> 5] = (uint32_t)s_stage[0];
            sizes[blk] = (int32_t)(obits >> 3);
        }
        __syncthreads();
    }
}

// the members, packed: one workgroup per member copies its slot to the member's offset; one more writes the EOF block
__global__ void __launch_bounds__(256) k_bgzf_gather(const uint8_t* slots, const int32_t* sizes, const int64_t* off, int n_blocks, int with_eof, uint8_t* out)
{
    const int blk = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (blk >= n_blocks) {
        if (with_eof && tid < BGZF_EOF_BYTES) out[off[n_blocks] + tid] = bgzf_eof_byte(tid);
        return;
    }
    const uint32_t* S = (const uint32_t*)(slots + (size_t)blk * BGZF_SLOT);
    const uint8_t* s = (const uint8_t*)S;
    uint8_t* d = out + off[blk];
    const int n = sizes[blk];
    int lead = (int)((4 - (off[blk] & 3)) & 3);
    if (lead > n) lead = n;
    const int nw = (n - lead) >> 2, tail = n - lead - 4 * nw;
    if (tid < lead) d[tid] = s[tid];
    uint32_t* D = (uint32_t*)(d + lead);
    const int sh = 8 * (lead & 3);
    for (int w = tid; w < nw; w += 256) {
        const int k = (lead + 4 * w) >> 2;
        D[w] = sh ? S[k] >> sh | S[k + 1] << (32 - sh) : S[k];
    }
    if (tid < tail) d[lead + 4 * nw + tid] = s[lead + 4 * nw + tid];
}

// ------------------------------------------------------------------ BGZF members inflated on the device (bgzf_inflate.h)
// One wavefront per member and 8 KB of LDS, so that many members are in flight per CU (8 as compiled: the registers bind): symbol
// decoding is serial per member and the number of members in flight is the throughput.  The member is worked off in turns; the state between turns
// (bit position, output position, in a block or between blocks) is a few LDS words written by lane 0 only.
//   stage    all lanes load BGZI_WIN bytes of the deflate area from the 16-byte word holding the current bit into LDS with
//            16-byte loads; bytes outside the area are zeroed, so the decoding lane never waits on a global load and never sees a
//            byte that is not the member's.
//   header   (between blocks) lane 0 reads the block header; a stored block is copied by all lanes; for a dynamic block lane 0
//            reads the code-length code and the lengths, for a fixed block all lanes write the fixed lengths; lane 0 makes the
//            count / sorted-symbol arrays and the validity checks; all lanes fill the primary tables by decoding every index.
//   decode   (in a block) lane 0 decodes up to BGZI_TOK tokens (bgzf_deflate.h's format) and their output positions into LDS,
//            checking every distance and length against the member's first and last output byte.
//   output   literals are stored at once; matches in rounds: everything below the lowest unresolved match is final, so every match
//            whose source ends there can go -- one lane per short match, the whole wavefront for a long one.  A match with
//            distance < length reads its source modulo the distance, i.e. only bytes that were final before the round.  Output
//            goes straight to HBM; later rounds read earlier rounds' stores of the same workgroup (same CU) after a
//            workgroup-scope fence.
// Then the CRC-32 of the output by all lanes (slices combined as in k_bgzf_deflate) against the trailer.
struct BgziBits { uint64_t hold; int nbits, wpos; };
static __device__ inline void bgzi_refill(const uint32_t* win, BgziBits& r)          // at least 33 bits afterwards
{
    if (r.nbits <= 32) { r.hold |= (uint64_t)(r.wpos < BGZI_WIN_DW ? win[r.wpos] : 0u) << r.nbits; ++r.wpos; r.nbits += 32; }
}
static __device__ inline uint32_t bgzi_take(BgziBits& r, int n)                      // n <= 31
{
    const uint32_t v = (uint32_t)r.hold & ((1u << n) - 1u);
    r.hold >>= n; r.nbits -= n;
    return v;
}
static __device__ inline void bgzi_open(const uint32_t* win, BgziBits& r, int bit)   // the reader at bit `bit` of the window
{
    r.hold = 0; r.nbits = 0; r.wpos = bit >> 5;
    bgzi_refill(win, r); (void)bgzi_take(r, bit & 31); bgzi_refill(win, r);
}
#define BGZI_POS(r) (8 * base_off + 32 * (r).wpos - (r).nbits)       // the reader's bit position in the deflate area

__global__ void __launch_bounds__(BGZI_THREADS) k_bgzf_inflate(const uint8_t* comp, const BgzfMember* mem, int n_members, int member0, uint8_t* text, int32_t* err)
{
    __shared__ uint32_t s_win[BGZI_WIN_DW], s_tok[BGZI_TOK], s_crc[256];
    __shared__ uint16_t s_tpos[BGZI_TOK], s_pll[1 << BGZI_LL_PB], s_pd[1 << BGZI_D_PB];
    __shared__ uint16_t s_symll[288], s_symd[32], s_symcl[DFL_NCL + 1], s_cntll[16], s_cntd[16], s_cntcl[16], s_offs[16];
    __shared__ uint8_t s_len[288 + 32], s_lencl[DFL_NCL + 1];
    __shared__ int s_bitpos, s_opos, s_inblock, s_last, s_bad, s_done, s_ntok, s_kind, s_slen, s_ssrc, s_sdst;

    const int lane = (int)threadIdx.x, m = (int)blockIdx.x;
    if (m >= n_members) return;
    const BgzfMember M = mem[m];
    const uint8_t* in = comp + M.coff + M.hlen;                      // the deflate area: dlen bytes
    const int dlen = M.csize - M.hlen - BGZF_TAIL, isize = M.isize;
    uint8_t* out = text + M.uoff;
    for (int k = lane; k < 256; k += BGZI_THREADS) s_crc[k] = bgz_crc_table_entry((uint32_t)k);
    if (lane == 0) { s_bitpos = 0; s_opos = 0; s_inblock = 0; s_last = 0; s_bad = 0; s_done = 0; s_ntok = 0; s_kind = 0; }
    __syncthreads();
    bool bad = dlen < 0 || isize < 0 || isize > BGZI_MAX_ISIZE, done = false;        // (the host's walk has checked these)
    // every turn consumes at least one bit or ends the member
    const int64_t max_turns = 8 * (int64_t)(dlen > 0 ? dlen : 0) + 2;
    for (int64_t turn = 0; turn < max_turns && !bad && !done; ++turn) {
        const int bitpos = s_bitpos, opos0 = s_opos, inblock = s_inblock, last = s_last;
        const int byte = bitpos >> 3, base_off = byte - (int)((uintptr_t)(in + byte) & 15);
        __syncthreads();
        // ---- stage
        for (int c = lane; c < BGZI_WIN / 16; c += BGZI_THREADS) {
            const int off = base_off + 16 * c;
            uint32_t w[4] = { 0, 0, 0, 0 };
            if (off + 16 > 0 && off < dlen) {
                const uint4 v = *(const uint4*)(in + off);
                w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
                if (off < 0 || off + 16 > dlen)
                    for (int b = 0; b < 16; ++b) if (off + b < 0 || off + b >= dlen) w[b >> 2] &= ~(0xffu << (8 * (b & 3)));
            }
            for (int k = 0; k < 4; ++k) s_win[4 * c + k] = w[k];
        }
        __syncthreads();
        if (!inblock) {
            // ---- header
            if (lane == 0) {
                BgziBits r;
                bgzi_open(s_win, r, bitpos - 8 * base_off);
                bool fail = false;
                const int fin = (int)bgzi_take(r, 1), type = (int)bgzi_take(r, 2);
                s_kind = type; s_last = fin;
                if (type == 3) fail = true;
                else if (type == 0) {
                    (void)bgzi_take(r, r.nbits & 7);
                    bgzi_refill(s_win, r);
                    const int len = (int)bgzi_take(r, 16), nlen = (int)bgzi_take(r, 16);
                    const int src = BGZI_POS(r) >> 3;
                    if (len != (~nlen & 0xffff) || src + len > dlen || opos0 + len > isize) fail = true;
                    else {
                        s_slen = len; s_ssrc = src; s_sdst = opos0; s_opos = opos0 + len; s_bitpos = 8 * (src + len);
                        if (fin) { if (src + len != dlen || opos0 + len != isize) fail = true; else s_done = 1; }
                    }
                } else {
                    if (type == 2) {
                        bgzi_refill(s_win, r);
                        const int hlit = 257 + (int)bgzi_take(r, 5), hdist = 1 + (int)bgzi_take(r, 5), hclen = 4 + (int)bgzi_take(r, 4);
                        const int total = hlit + hdist;
                        if (hlit > DFL_NLL || hdist > DFL_ND) fail = true;
                        for (int i = 0; i < DFL_NCL; ++i) s_lencl[i] = 0;
                        for (int i = 0; i < hclen; ++i) { bgzi_refill(s_win, r); s_lencl[dfl_cl_order(i)] = (uint8_t)bgzi_take(r, 3); }
                        if (!fail && !dfl_canonical(s_lencl, DFL_NCL, BGZI_CODES, s_cntcl, s_symcl, s_offs)) fail = true;
                        int i = 0;
                        while (!fail && i < total) {                 // at most 316 lengths
                            bgzi_refill(s_win, r);
                            const uint32_t e = dfl_decode_walk((uint32_t)r.hold, s_cntcl, s_symcl, DFL_CL_BITS);
                            if (!e) { fail = true; break; }
                            (void)bgzi_take(r, (int)(e >> 12));
                            const int sym = (int)(e & 0xfff);
                            if (sym < 16) { s_len[i++] = (uint8_t)sym; continue; }
                            int rep, val = 0;
                            if (sym == 16) { if (i == 0) { fail = true; break; } val = s_len[i - 1]; rep = 3 + (int)bgzi_take(r, 2); }
                            else if (sym == 17) rep = 3 + (int)bgzi_take(r, 3);
                            else rep = 11 + (int)bgzi_take(r, 7);
                            if (i + rep > total) { fail = true; break; }
                            for (; rep > 0; --rep) s_len[i++] = (uint8_t)val;
                        }
                        if (!fail && s_len[DFL_EOB] == 0) fail = true;
                        if (!fail) {                                 // the distance lengths to their own place, the rest zero
                            for (int k = hdist - 1; k >= 0; --k) s_len[288 + k] = s_len[hlit + k];
                            for (int k = hlit; k < 288; ++k) s_len[k] = 0;
                            for (int k = 288 + hdist; k < 320; ++k) s_len[k] = 0;
                        }
                    }
                    const int pos = BGZI_POS(r);
                    if (pos > 8 * dlen) fail = true;
                    s_bitpos = pos;
                }
                if (fail) s_bad = 1;
            }
            __syncthreads();
            const int kind = s_kind;
            bad = s_bad != 0;
            if (!bad && kind == 0) {                                 // a stored block: within both areas, checked above
                const int n = s_slen;
                const uint8_t* src = in + s_ssrc;
                uint8_t* dst = out + s_sdst;
                for (int i = lane; i < n; i += BGZI_THREADS) dst[i] = src[i];
            }
            if (!bad && kind == 1) {
                for (int s = lane; s < 288; s += BGZI_THREADS) s_len[s] = (uint8_t)dfl_fixed_ll_len(s);
                if (lane < 32) s_len[288 + lane] = 5;
            }
            __syncthreads();
            if (!bad && kind != 0) {
                if (lane == 0) {
                    if (dfl_canonical(s_len, 288, BGZI_LENS, s_cntll, s_symll, s_offs) && dfl_canonical(s_len + 288, 32, BGZI_DISTS, s_cntd, s_symd, s_offs)) s_inblock = 1;
                    else s_bad = 1;
                }
                __syncthreads();
                bad = s_bad != 0;
                if (!bad) {
                    for (int e = lane; e < 1 << BGZI_LL_PB; e += BGZI_THREADS) s_pll[e] = (uint16_t)dfl_decode_walk((uint32_t)e, s_cntll, s_symll, BGZI_LL_PB);
                    for (int e = lane; e < 1 << BGZI_D_PB; e += BGZI_THREADS) s_pd[e] = (uint16_t)dfl_decode_walk((uint32_t)e, s_cntd, s_symd, BGZI_D_PB);
                }
            }
            __syncthreads();
            done = s_done != 0;
            continue;
        }
        // ---- decode
        if (lane == 0) {
            BgziBits r;
            bgzi_open(s_win, r, bitpos - 8 * base_off);
            int ntok = 0, opos = opos0;
            bool fail = false, eob = false;
            while (ntok < BGZI_TOK && r.wpos + 2 <= BGZI_WIN_DW) {
                bgzi_refill(s_win, r);
                uint32_t e = s_pll[(uint32_t)r.hold & ((1u << BGZI_LL_PB) - 1u)];
                if (!e) e = dfl_decode_walk((uint32_t)r.hold, s_cntll, s_symll, DFL_LL_BITS);
                if (!e) { fail = true; break; }
                (void)bgzi_take(r, (int)(e >> 12));
                const int sym = (int)(e & 0xfff);
                if (sym < DFL_EOB) {
                    if (opos >= isize) { fail = true; break; }
                    s_tok[ntok] = (uint32_t)sym; s_tpos[ntok] = (uint16_t)opos;
                    ++ntok; ++opos;
                    continue;
                }
                if (sym == DFL_EOB) { eob = true; break; }
                if (sym >= DFL_NLL) { fail = true; break; }
                const int len = dfl_len_base(sym) + (int)bgzi_take(r, dfl_len_extra_bits(sym));
                bgzi_refill(s_win, r);
                e = s_pd[(uint32_t)r.hold & ((1u << BGZI_D_PB) - 1u)];
                if (!e) e = dfl_decode_walk((uint32_t)r.hold, s_cntd, s_symd, DFL_LL_BITS);
                if (!e) { fail = true; break; }
                (void)bgzi_take(r, (int)(e >> 12));
                const int dsym = (int)(e & 0xfff);
                if (dsym >= DFL_ND) { fail = true; break; }
                const int dist = dfl_dist_base(dsym) + (int)bgzi_take(r, dfl_dist_extra_bits(dsym));
                if (dist > opos || opos + len > isize) { fail = true; break; }
                s_tok[ntok] = dfl_tok_match(len, dist); s_tpos[ntok] = (uint16_t)opos;
                ++ntok; opos += len;
            }
            const int pos = BGZI_POS(r);
            if (pos > 8 * dlen) fail = true;                         // the bits came from beyond the deflate area
            if (!fail && eob) {
                s_inblock = 0;
                if (last) { if (((pos + 7) >> 3) != dlen || opos != isize) fail = true; else s_done = 1; }
            }
            s_ntok = ntok; s_opos = opos; s_bitpos = pos;
            if (fail) s_bad = 1;
        }
        __syncthreads();
        bad = s_bad != 0;
        done = s_done != 0;
        if (bad) break;
        // ---- output
        const int ntok = s_ntok;
        uint32_t t[BGZI_TOK / BGZI_THREADS]; int p[BGZI_TOK / BGZI_THREADS]; bool un[BGZI_TOK / BGZI_THREADS];
#pragma unroll
        for (int j = 0; j < BGZI_TOK / BGZI_THREADS; ++j) {
            const int k = lane + BGZI_THREADS * j;
            t[j] = 0; p[j] = 0; un[j] = false;
            if (k >= ntok) continue;
            t[j] = s_tok[k]; p[j] = s_tpos[k];
            if (t[j] & DFL_TOK_MATCH) un[j] = p[j] + dfl_tok_len(t[j]) <= isize && dfl_tok_dist(t[j]) <= p[j];     // (as the decoding lane checked)
            else if (p[j] < isize) out[p[j]] = (uint8_t)t[j];
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __syncthreads();
        for (int round = 0; round < BGZI_TOK; ++round) {             // every round resolves the lowest unresolved match at least
            int f = 0x7fffffff;
#pragma unroll
            for (int j = 0; j < BGZI_TOK / BGZI_THREADS; ++j) if (un[j] && p[j] < f) f = p[j];
            for (int o = 32; o > 0; o >>= 1) { const int u = __shfl_xor(f, o); if (u < f) f = u; }
            if (f == 0x7fffffff) break;
#pragma unroll
            for (int j = 0; j < BGZI_TOK / BGZI_THREADS; ++j) {
                const int len = dfl_tok_len(t[j]), d = dfl_tok_dist(t[j]);
                const bool can = un[j] && p[j] - d + (len < d ? len : d) <= f;
                const bool big = can && len > BGZI_COOP_LEN;
                unsigned long long mask = __ballot(big);
                while (mask) {                                       // a long match: the whole wavefront
                    const int from = __ffsll((long long)mask) - 1;
                    mask &= mask - 1;
                    const int bp = __shfl(p[j], from);
                    const uint32_t bt = __shfl(t[j], from);
                    const int bl = dfl_tok_len(bt), bd = dfl_tok_dist(bt);
                    for (int i = lane; i < bl; i += BGZI_THREADS) out[bp + i] = out[bp - bd + (bd >= bl ? i : i % bd)];
                }
                if (can && !big) {                                   // a short one: this lane, eight bytes at a time
                    const uint8_t* src = out + p[j] - d;
                    uint8_t* dst = out + p[j];
                    for (int c = 0; c < len; c += 8) {
                        uint8_t v[8];
#pragma unroll
                        for (int q = 0; q < 8; ++q) v[q] = c + q < len ? src[d >= len ? c + q : (c + q) % d] : (uint8_t)0;
#pragma unroll
                        for (int q = 0; q < 8; ++q) if (c + q < len) dst[c + q] = v[q];
                    }
                }
                if (can) un[j] = false;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            __syncthreads();
        }
    }
    if (!bad && !done) bad = true;
    // ---- CRC-32 of the output against the trailer
    if (!bad) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __syncthreads();
        const int per = (isize + BGZI_THREADS - 1) / BGZI_THREADS, lo = lane * per < isize ? lane * per : isize, hi = lo + per < isize ? lo + per : isize;
        uint32_t c = lane == 0 ? 0xffffffffu : 0u;
        for (int q = lo; q < hi; ++q) c = s_crc[(c ^ out[q]) & 0xff] ^ (c >> 8);
        uint32_t x = lane == 0 || lo < hi ? bgz_crc_mul(c, bgz_crc_xpow8((uint32_t)(isize - hi))) : 0u;
        for (int o = 32; o > 0; o >>= 1) x ^= __shfl_xor(x, o);
        const uint8_t* tr = comp + M.coff + M.csize - BGZF_TAIL;
        const uint32_t want = (uint32_t)tr[0] | (uint32_t)tr[1] << 8 | (uint32_t)tr[2] << 16 | (uint32_t)tr[3] << 24;
        if (~x != want) bad = true;
    }
    if (bad && lane == 0) atomicMax(err, (int32_t)(BGZI_NO_ERROR - (member0 + m)));
}

// ------------------------------------------------------------------ stable radix sort of (key, index) pairs (bam_sort.h)
// the lanes' words of SortBits, OR-ed over the wavefront, then into bits[] by one lane per wavefront (every lane of the
// workgroup calls this)
static __device__ inline void sort_bits_flush(const int32_t* w, int32_t* bits)
{
    for (int k = 0; k <= SORT_BITS_HAS_OTHER; ++k) {
        int v = w[k];
        for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o);
        if (((int)threadIdx.x & 63) == 0 && v) atomicOr(&bits[k], v);
    }
}

__global__ void __launch_bounds__(SORT_THREADS) k_sort_bits(const uint64_t* keys, int64_t n, int32_t* bits)
{
    int32_t w[SORT_BITS_N];
    for (int k = 0; k < SORT_BITS_N; ++k) w[k] = 0;
    const int64_t step = (int64_t)gridDim.x * SORT_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * SORT_THREADS + (int)threadIdx.x; i < n; i += step) sort_bits_add(keys[i], w);
    sort_bits_flush(w, bits);
}

// step 1 of a pass: the tile's count of every digit, digit-major
__global__ void __launch_bounds__(SORT_THREADS) k_sort_hist(const uint64_t* keys, int64_t n, int byte, int n_tiles, int32_t* hist)
{
    __shared__ int s_h[SORT_RADIX];
    const int tid = (int)threadIdx.x;
    s_h[tid] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * SORT_TILE;
    for (int j = 0; j < SORT_ITEMS; ++j) {
        const int64_t i = base + j * SORT_THREADS + tid;
        if (i < n) atomicAdd(&s_h[sort_digit(keys[i], byte)], 1);
    }
    __syncthreads();
    hist[(int64_t)tid * n_tiles + (int)blockIdx.x] = s_h[tid];
}

// step 3: the stable scatter.  off = the scan of hist; idx == null: the identity (the first pass)
__global__ void __launch_bounds__(SORT_THREADS) k_sort_scatter(const uint64_t* keys, const uint32_t* idx, int64_t n, int byte, int n_tiles, const int64_t* off,
                                                               uint64_t* keys_out, uint32_t* idx_out)
{
    __shared__ uint16_t s_cnt[SORT_ITEMS * (SORT_THREADS / 64)][SORT_RADIX];      // per (item, wave): the count of every digit, then its exclusive prefix
    __shared__ int64_t s_base[SORT_RADIX];
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int k = 0; k < SORT_ITEMS * (SORT_THREADS / 64); ++k) s_cnt[k][tid] = 0;
    s_base[tid] = off[(int64_t)tid * n_tiles + (int)blockIdx.x];
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * SORT_TILE;
    uint64_t key[SORT_ITEMS];
    int rank[SORT_ITEMS];
#pragma unroll
    for (int j = 0; j < SORT_ITEMS; ++j) {
        const int64_t i = base + j * SORT_THREADS + tid;
        const bool valid = i < n;
        key[j] = valid ? keys[i] : 0;
        const int d = sort_digit(key[j], byte);
        unsigned long long same = __ballot(valid);                    // the lanes of the wave that hold the same digit
        for (int bit = 0; bit < 8; ++bit) {
            const unsigned long long set = __ballot(d >> bit & 1);
            same &= (d >> bit & 1) ? set : ~set;
        }
        rank[j] = __popcll(same & ((1ull << lane) - 1));
        if (valid && rank[j] == 0) s_cnt[j * (SORT_THREADS / 64) + wv][d] = (uint16_t)__popcll(same);
    }
    __syncthreads();
    {   // lane = digit: the groups before each (item, wave) group
        int run = 0;
        for (int k = 0; k < SORT_ITEMS * (SORT_THREADS / 64); ++k) { const int c = s_cnt[k][tid]; s_cnt[k][tid] = (uint16_t)run; run += c; }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < SORT_ITEMS; ++j) {
        const int64_t i = base + j * SORT_THREADS + tid;
        if (i >= n) continue;
        const int d = sort_digit(key[j], byte);
        const int64_t at = s_base[d] + s_cnt[j * (SORT_THREADS / 64) + wv][d] + rank[j];
        keys_out[at] = key[j];
        idx_out[at] = idx ? idx[i] : (uint32_t)i;
    }
}

// ------------------------------------------------------------------ coordinate-sorted BAM records (bam_sort.h)
// step 1: one lane per read walks the read's records along block_size and counts them; the OR / AND of their keys on the way
__global__ void __launch_bounds__(64) k_bamrec_count(const uint8_t* bam, const int64_t* bam_off, int n_reads, int32_t* counts, int32_t* bits, int32_t* err)
{
    const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    int32_t w[SORT_BITS_N];
    for (int k = 0; k < SORT_BITS_N; ++k) w[k] = 0;
    if (r < n_reads) {
        int64_t o = bam_off[r];
        const int64_t hi = bam_off[r + 1];
        int32_t cnt = 0;
        bool bad = false;
        while (o < hi) {
            if (hi - o < BAMSORT_MIN_REC) { bad = true; break; }
            const int64_t size = 4 + (int64_t)(int32_t)bamsort_ld32(bam + o);
            if (size < BAMSORT_MIN_REC || size > hi - o) { bad = true; break; }
            sort_bits_add(bamsort_key(bam + o), w);
            ++cnt; o += size;
        }
        counts[r] = bad ? 0 : cnt;
        if (bad) atomicOr(err, BAMSORT_ERR_WALK);
    }
    sort_bits_flush(w, bits);
}

// step 2 (after the scan of the counts): key, place and size of every record, in response order
__global__ void __launch_bounds__(64) k_bamrec_keys(const uint8_t* bam, const int64_t* bam_off, int n_reads, const int64_t* first, uint64_t* keys, int64_t* src_off, int32_t* sizes)
{
    const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (r >= n_reads) return;
    int64_t o = bam_off[r];
    const int64_t k0 = first[r], k1 = first[r + 1];
    for (int64_t k = k0; k < k1; ++k) {
        const int32_t size = 4 + (int32_t)bamsort_ld32(bam + o);
        keys[k] = bamsort_key(bam + o); src_off[k] = o; sizes[k] = size;
        o += size;
    }
}

// the sizes in sorted order (their scan gives the records' places in the sorted stream)
__global__ void __launch_bounds__(256) k_bamrec_sizes(const uint32_t* idx, const int32_t* sizes, int n, int32_t* out)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n) out[i] = sizes[idx[i]];
}

// the gather, balanced by bytes: every workgroup fills BAMSORT_CHUNK bytes of the destination.  One lane finds the records
// that overlap the chunk (their places are ascending), the workgroup loads their bounds into LDS, and every lane then looks
// up the record of each of its dwords there.  A dword inside one record is one load and one store; a dword across a
// boundary, and the tail of the stream, go byte by byte.
__global__ void __launch_bounds__(256) k_bamrec_gather(const uint8_t* src, const int64_t* src_off, const uint32_t* idx, const int64_t* dst_off, int n_rec, int64_t total, uint8_t* dst)
{
    __shared__ int64_t s_src[BAMSORT_CHUNK_RECS];
    __shared__ int32_t s_dst[BAMSORT_CHUNK_RECS + 1];
    __shared__ int s_r0, s_n;
    const int tid = (int)threadIdx.x;
    const int64_t lo = (int64_t)blockIdx.x * BAMSORT_CHUNK, hi = total - lo < BAMSORT_CHUNK ? total : lo + BAMSORT_CHUNK;
    if (tid == 0) {
        int a = 0, b = n_rec - 1;                                    // the last record that starts at or before lo
        while (a < b) { const int m = (int)(((int64_t)a + b + 1) >> 1); if (dst_off[m] <= lo) a = m; else b = m - 1; }
        int c = a, e = n_rec - 1;                                    // the last record that starts before hi
        while (c < e) { const int m = (int)(((int64_t)c + e + 1) >> 1); if (dst_off[m] < hi) c = m; else e = m - 1; }
        s_r0 = a;
        s_n = c - a + 1 < BAMSORT_CHUNK_RECS ? c - a + 1 : BAMSORT_CHUNK_RECS;    // (records of at least BAMSORT_MIN_REC bytes: never more)
    }
    __syncthreads();
    const int r0 = s_r0, nr = s_n;
    for (int k = tid; k < nr; k += 256) { s_src[k] = src_off[idx[r0 + k]]; s_dst[k] = (int32_t)(dst_off[r0 + k] - lo); }
    if (tid == 0) s_dst[nr] = (int32_t)(dst_off[r0 + nr] - lo);
    __syncthreads();
    int len = (int)(hi - lo);
    if (len > s_dst[nr]) len = s_dst[nr];
    for (int x = 4 * tid; x < len; x += 4 * 256) {
        int a = 0, b = nr - 1;                                       // the record of byte x
        while (a < b) { const int m = (a + b + 1) >> 1; if (s_dst[m] <= x) a = m; else b = m - 1; }
        if (x + 4 <= len && x + 4 <= s_dst[a + 1]) *(uint32_t*)(dst + lo + x) = bamsort_ld32(src + s_src[a] + (x - s_dst[a]));
        else
            for (int q = 0; q < 4 && x + q < len; ++q) {
                while (a + 1 < nr && s_dst[a + 1] <= x + q) ++a;
                dst[lo + x + q] = src[s_src[a] + (x + q - s_dst[a])];
            }
    }
}

// ------------------------------------------------------------------ the BAI index of the sorted, compressed records (bam_sort.h)
// one lane per record: the bin key, the windows the record overlaps, the count of unplaced records
__global__ void __launch_bounds__(64) k_bai_records(BaiView v)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    bool unplaced = false;
    if (i < v.n_rec) {
        const uint8_t* rec = v.bam + v.rec_off[i];
        const int64_t size = v.rec_off[i + 1] - v.rec_off[i];
        const int32_t refid = (int32_t)bamsort_ld32(rec + 4), pos = (int32_t)bamsort_ld32(rec + 8);
        uint64_t key = SORT_KEY_LAST;
        if (refid == -1) unplaced = true;
        else if (refid < 0 || refid >= v.n_ref || pos < 0) atomicOr(v.err, BAMSORT_ERR_WALK);
        else {
            const uint32_t bmq = bamsort_ld32(rec + 12), fnc = bamsort_ld32(rec + 16);
            const int64_t l_name = bmq & 0xff, n_cig = fnc & 0xffff;
            if (36 + l_name + 4 * n_cig > size) atomicOr(v.err, BAMSORT_ERR_WALK);
            else {
                const uint8_t* cig = rec + 36 + l_name;
                int64_t span = 0;
                for (int64_t c = 0; c < n_cig; ++c) {
                    const uint32_t x = bamsort_ld32(cig + 4 * c), op = x & 0xf;
                    if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) span += x >> 4;
                }
                const int64_t end = (int64_t)pos + (span > 0 ? span : 1);
                const int32_t w0 = v.win_base[refid], n_win = v.win_base[refid + 1] - w0;
                key = (uint64_t)(uint32_t)refid << 32 | (bmq >> 16);
                if (end > BAI_MAX_END) atomicOr(v.err, BAMSORT_ERR_END);
                else if ((end - 1) >> BAI_WINDOW_SHIFT >= n_win) atomicOr(v.err, BAMSORT_ERR_WINDOW);
                else for (int64_t w = pos >> BAI_WINDOW_SHIFT; w <= (end - 1) >> BAI_WINDOW_SHIFT; ++w) atomicMax(&v.win[w0 + w], v.n_rec - 1 - i);
            }
        }
        v.keys[i] = key;
    }
    const int c = __popcll(__ballot(unplaced));
    if (((int)threadIdx.x & 63) == 0 && c) atomicAdd(v.n_no_coor, c);
}

// positions of the (refID, bin)-sorted list at which a chunk starts
__global__ void __launch_bounds__(256) k_bai_mark(const uint64_t* keys, const uint32_t* idx, int n, int32_t* start)
{
    const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (j < n) start[j] = j == 0 || keys[j] != keys[j - 1] || idx[j] != idx[j - 1] + 1;
}

// the chunks, compacted: cid = the scan of start
__global__ void __launch_bounds__(256) k_bai_chunks(const uint64_t* keys, const uint32_t* idx, int n, const int32_t* start, const int64_t* cid, const int64_t* rec_off,
                                                    const int64_t* member_off, int64_t coffset0, BaiChunk* out)
{
    const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (j >= n) return;
    const int64_t c = cid[j] + start[j] - 1;
    if (start[j]) { out[c].key = keys[j]; out[c].beg = bai_voffset(member_off, coffset0, rec_off[idx[j]]); }
    if (j == n - 1 || start[j + 1]) out[c].end = bai_voffset(member_off, coffset0, rec_off[idx[j] + 1]);
}

// the windows' smallest record index as that record's virtual offset (SORT_KEY_LAST: no record)
__global__ void __launch_bounds__(256) k_bai_windows(const int32_t* win, int n_win, int n_rec, const int64_t* rec_off, const int64_t* member_off, int64_t coffset0, uint64_t* out)
{
    const int w = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (w < n_win) out[w] = win[w] < 0 ? SORT_KEY_LAST : bai_voffset(member_off, coffset0, rec_off[n_rec - 1 - win[w]]);
}

// ------------------------------------------------------------------ duplicate marking between the encoder and the sort (bam_dup.h)
// a lane's count, added up over the wavefront, into *dst by one lane (every lane of the wavefront calls this)
static __device__ inline void dup_wave_add(int v, int32_t* dst)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (((int)threadIdx.x & 63) == 0 && v) atomicAdd(dst, v);
}

// (a) one lane per template walks the records of its reads along block_size, as k_bamrec_count does: the primaries, their ends from
// the records' own CIGARs, the fragment and pair keys, is_paired, the place of QUAL, the counts.  A template with an error has no entry.
__global__ void __launch_bounds__(64) k_dup_entries(DupView v)
{
    const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    int n_unpaired = 0, n_pair = 0, n_sec = 0, n_unmapped = 0, max_len = 0, err = 0;
    if (t < v.n_tmpl) {
        const int r0 = v.paired ? 2 * t : t, nr = v.paired && r0 + 1 < v.n_reads ? 2 : 1;
        DupEnd e[2];
        bool has[2] = { false, false };
        for (int k = 0; k < nr && !err; ++k) {
            int64_t o = v.bam_off[r0 + k];
            const int64_t hi = v.bam_off[r0 + k + 1];
            bool primary = false;
            while (o < hi) {
                if (hi - o < BAMSORT_MIN_REC) { err = BAMDUP_ERR_WALK; break; }
                const int64_t size = 4 + (int64_t)(int32_t)bamsort_ld32(v.bam + o);
                if (size < BAMSORT_MIN_REC || size > hi - o) { err = BAMDUP_ERR_WALK; break; }
                const uint32_t flag = dup_ld16(v.bam + o + 18);
                if (flag & 0x900) ++n_sec;
                else if (primary) { err = BAMDUP_ERR_PRIMARY; break; }
                else {
                    primary = true;
                    if (flag & 4) ++n_unmapped;
                    else {
                        err = dup_end(v.bam + o, size, o, e[k]);
                        if (err) break;
                        has[k] = true;
                    }
                }
                o += size;
            }
        }
        if (err) { has[0] = has[1] = false; n_sec = n_unmapped = 0; }
        for (int k = 0; k < nr; ++k) {
            const bool p = has[k] && (e[k].flag & 1) && !(e[k].flag & 8);
            v.frag_end[r0 + k] = has[k] ? e[k].key : SORT_KEY_LAST;
            v.qual_off[r0 + k] = has[k] ? e[k].qual_off : 0;
            v.l_seq[r0 + k] = has[k] ? e[k].l_seq : 0;
            v.is_paired[r0 + k] = p ? 1 : 0;
            if (has[k] && !p) ++n_unpaired;
            if (has[k] && e[k].l_seq > max_len) max_len = e[k].l_seq;
        }
        if (v.paired) {
            const bool both = has[0] && has[1];
            v.pair_a[t] = !both ? SORT_KEY_LAST : e[0].key < e[1].key ? e[0].key : e[1].key;
            v.pair_b[t] = !both ? SORT_KEY_LAST : e[0].key < e[1].key ? e[1].key : e[0].key;
            n_pair = both ? 1 : 0;
        }
    }
    dup_wave_add(n_unpaired, &v.cnt[DUP_CNT_UNPAIRED]);
    dup_wave_add(n_pair, &v.cnt[DUP_CNT_PAIRS]);
    dup_wave_add(n_sec, &v.cnt[DUP_CNT_SECONDARY]);
    dup_wave_add(n_unmapped, &v.cnt[DUP_CNT_UNMAPPED]);
    for (int o = 32; o > 0; o >>= 1) { const int m = __shfl_xor(max_len, o); max_len = m > max_len ? m : max_len; err |= __shfl_xor(err, o); }
    if (((int)threadIdx.x & 63) == 0) {
        if (max_len) atomicMax(&v.cnt[DUP_CNT_MAX_LEN], max_len);
        if (err) atomicOr(&v.cnt[DUP_CNT_ERR], err);
    }
}

// (b) the scores, by the lane groups of k_bam_emit: G lanes per read (8, or the wavefront for long reads) share out the aligned
// 32-bit words of QUAL, take the up to three bytes before the first and after the last singly, and add up within the group
template <int G>
__global__ void __launch_bounds__(256) k_dup_scores(DupView v)
{
    const int r = blockIdx.x * (256 / G) + ((int)threadIdx.x / G), sub = (int)threadIdx.x % G;
    int32_t s = 0;
    if (r < v.n_reads) {
        const int32_t n = v.l_seq[r];
        const uint8_t* q = v.bam + v.qual_off[r];
        const int32_t lead = (int32_t)((4 - ((uintptr_t)q & 3)) & 3), head = n < lead ? n : lead;
        const int32_t nw = (n - head) >> 2, tail = n - head - 4 * nw;
        if (sub < head) s += dup_qual(q[sub]);
        const uint32_t* w = (const uint32_t*)(q + head);
        for (int32_t k = sub; k < nw; k += G) s += dup_qual4(w[k]);
        if (sub < tail) s += dup_qual(q[head + 4 * nw + sub]);
    }
    for (int o = G / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (r < v.n_reads && sub == 0) v.score[r] = s > DUP_SCORE_CAP ? DUP_SCORE_CAP : s;
}

// (c) the first sort keys: the read's score under is_paired, the template's score
__global__ void __launch_bounds__(256) k_dup_score_keys(DupView v, uint64_t* frag_key, uint64_t* pair_key)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < v.n_reads) frag_key[i] = v.frag_end[i] == SORT_KEY_LAST ? SORT_KEY_LAST : dup_score_key(v.score[i], !v.is_paired[i]);
    if (v.paired && i < v.n_tmpl) pair_key[i] = v.pair_a[i] == SORT_KEY_LAST ? SORT_KEY_LAST : dup_score_key(v.score[2 * i] + v.score[2 * i + 1], false);
}

// the next key of a chain of sorts, in the order the last one left
__global__ void __launch_bounds__(256) k_dup_gather(const uint64_t* src, const uint32_t* idx, int n, uint64_t* out)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n) out[i] = src[idx[i]];
}

// The verdicts.  keys / idx: the entries after the last sort; second: the pairs' other key (by entry), or null.  The first entry
// of a run of equal keys is its keeper -- the highest score, then the lowest index -- and among fragments a paired entry where
// there is one, so every later entry of the run is a duplicate unless it is itself paired (is_paired == null: the pair rule).
__global__ void __launch_bounds__(256) k_dup_decide(const uint64_t* keys, const uint32_t* idx, const uint64_t* second, int n, const uint8_t* is_paired, uint8_t* dup)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n || keys[i] == SORT_KEY_LAST) return;
    const uint32_t e = idx[i];
    const bool head = i == 0 || keys[i] != keys[i - 1] || (second && second[e] != second[idx[i - 1]]);
    dup[e] = !head && !(is_paired && is_paired[e]) ? 1 : 0;
}

// (d) one lane per template walks its records again and sets or clears 0x400 in byte 19 of each: a byte store by the only lane that
// owns the record.  The duplicates are counted on the way.
__global__ void __launch_bounds__(64) k_dup_flags(DupView v)
{
    const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    int n_frag = 0, n_pair = 0;
    if (t < v.n_tmpl) {
        const int r0 = v.paired ? 2 * t : t, nr = v.paired && r0 + 1 < v.n_reads ? 2 : 1;
        n_pair = v.paired ? v.pair_dup[t] : 0;
        for (int k = 0; k < nr; ++k) n_frag += v.frag_dup[r0 + k];
        const uint8_t bit = n_pair || n_frag ? 4 : 0;
        int64_t o = v.bam_off[r0];
        const int64_t hi = v.bam_off[r0 + nr];
        while (hi - o >= BAMSORT_MIN_REC) {                              // (the walk of k_dup_entries has passed)
            const int64_t size = 4 + (int64_t)(int32_t)bamsort_ld32(v.bam + o);
            if (size < BAMSORT_MIN_REC || size > hi - o) break;
            const uint8_t was = v.bam[o + 19], now = (uint8_t)((was & ~4) | bit);
            if (now != was) v.bam[o + 19] = now;
            o += size;
        }
    }
    dup_wave_add(n_frag, &v.cnt[DUP_CNT_UNPAIRED_DUP]);
    dup_wave_add(n_pair, &v.cnt[DUP_CNT_PAIR_DUP]);
}

// ------------------------------------------------------------------ alignment QC: a reduction over the records (bam_qc.h)
#define QC_THREADS 256
static __device__ inline unsigned long long qc_wave_sum(unsigned long long v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
static __device__ inline int qc_wave_max(int v)
{
    for (int o = 32; o > 0; o >>= 1) { const int u = __shfl_xor(v, o); v = u > v ? u : v; }
    return v;
}

// (a) one lane per item (a read's records, or one record), a fixed grid striding over the items.  Per round every lane has at most
// one record: the flag counters are ballots and popcounts kept by the lane whose number is the counter's word, the sums stay in the
// lanes until the end, equal (refID, unmapped) are combined in the wave before one global add per distinct value, and mapq_hist and
// the insert sizes below BAMQC_ISIZE_LDS go to the workgroup's copies in LDS.  Every wave runs its rounds in uniform control flow.
__global__ void __launch_bounds__(QC_THREADS, 4) k_qc_records(QcView v)
{
    __shared__ unsigned long long s_cnt[2 * QC_F_N + QC_S_N];
    __shared__ uint32_t s_mapq[BAMQC_MAPQ_BINS];
    __shared__ uint32_t s_isize[QC_ORIENTATIONS * BAMQC_ISIZE_LDS];
    __shared__ int32_t s_ext[2 * QC_ORIENTATIONS + 2];                 // the extremes as bam_qc.h encodes them, the longest read, the errors
    const int tid = (int)threadIdx.x, lane = tid & 63;
    for (int j = tid; j < 2 * QC_F_N + QC_S_N; j += QC_THREADS) s_cnt[j] = 0;
    for (int j = tid; j < BAMQC_MAPQ_BINS; j += QC_THREADS) s_mapq[j] = 0;
    for (int j = tid; j < QC_ORIENTATIONS * BAMQC_ISIZE_LDS; j += QC_THREADS) s_isize[j] = 0;
    if (tid < 2 * QC_ORIENTATIONS + 2) s_ext[tid] = 0;
    __syncthreads();
    unsigned long long f_acc = 0, sums[QC_S_N];
    for (int k = 0; k < QC_S_N; ++k) sums[k] = 0;
    int32_t max_len = 0, err = 0, mn0 = 0, mn1 = 0, mn2 = 0, mx0 = 0, mx1 = 0, mx2 = 0;
    const int64_t stride = (int64_t)gridDim.x * QC_THREADS;
    for (int64_t base = (int64_t)blockIdx.x * QC_THREADS; base < v.n_items; base += stride) {
        const int64_t i = base + tid;
        int64_t o = 0, hi = 0;
        if (i < v.n_items) { o = v.off[i]; hi = v.off[i + 1]; }
        bool live = o < hi;
        while (wave_any(live)) {
            QcRec q = {};
            bool ok = false;
            if (live) {
                int e = 0;
                int64_t size = 0;
                if (hi - o < BAMSORT_MIN_REC) e = BAMQC_ERR_WALK;
                else {
                    size = 4 + (int64_t)(int32_t)bamsort_ld32(v.bam + o);
                    if (size < BAMSORT_MIN_REC || size > hi - o || (!v.grouped && size != hi - o)) e = BAMQC_ERR_WALK;
                }
                if (!e) e = qc_record(v.bam + o, size, v.n_contigs, q);
                if (e) { err |= e; live = false; }
                else { ok = true; o += size; live = o < hi; }
            }
            // the flag counters: word 2k + w
            const uint32_t fm = ok ? q.fmask : 0u;
            const bool w1 = ok && q.w != 0;
            const bool any_w1 = wave_any(w1);
#pragma unroll
            for (int k = 0; k < QC_F_N; ++k) {
                const bool bit = (fm >> k & 1u) != 0;
                const int c0 = __popcll(wave_ballot_b(bit && !w1));
                if (lane == 2 * k) f_acc += (unsigned long long)c0;
                if (any_w1) {
                    const int c1 = __popcll(wave_ballot_b(bit && w1));
                    if (lane == 2 * k + 1) f_acc += (unsigned long long)c1;
                }
            }
            // the contigs: one add per distinct (refID, unmapped) of the wave
            const int32_t key = ok && q.refid >= 0 ? q.refid * 2 + ((fm >> QC_F_MAPPED & 1u) ? 0 : 1) : -1;
            unsigned long long rem = wave_ballot_b(key >= 0);
            while (rem) {
                const int leader = __ffsll((long long)rem) - 1;
                const int32_t k = wave_bcast(key, leader);
                const unsigned long long same = wave_ballot_b(key == k);
                if (lane == leader) atomicAdd(&v.blk[QC_W_CONTIG + k], (unsigned long long)__popcll(same));
                rem &= ~same;
            }
            if (ok) {
                if (q.refid < 0) sums[QC_S_UNPLACED] += 1;
                if (q.primary) {
                    sums[QC_S_SEQUENCES] += 1; sums[QC_S_TOTAL_LENGTH] += (unsigned long long)q.l_seq;
                    if (q.l_seq > max_len) max_len = q.l_seq;
                }
                if (q.mapped_primary) {
                    if (q.mapq == 0) sums[QC_S_READS_MQ0] += 1;
                    sums[QC_S_BASES_MAPPED] += (unsigned long long)q.l_seq; sums[QC_S_BASES_MAPPED_CIGAR] += q.m_cigar; sums[QC_S_BASES_SOFT_CLIPPED] += q.soft;
                    sums[QC_S_INS_EVENTS] += q.ins_ev; sums[QC_S_INS_BASES] += q.ins_b; sums[QC_S_DEL_EVENTS] += q.del_ev; sums[QC_S_DEL_BASES] += q.del_b;
                    sums[QC_S_MISMATCHES] += q.nm; sums[QC_S_RECORDS_WITHOUT_NM] += q.no_nm ? 1 : 0;
                    atomicAdd(&s_mapq[q.mapq], 1u);
                }
                if (q.orient >= 0) {
                    if (q.x < BAMQC_ISIZE_LDS) atomicAdd(&s_isize[q.orient * BAMQC_ISIZE_LDS + (int)q.x], 1u);
                    else atomicAdd(&v.blk[QC_W_ISIZE + q.orient * BAMQC_ISIZE_BINS + (q.x < BAMQC_ISIZE_BINS - 1 ? (int)q.x : BAMQC_ISIZE_BINS - 1)], 1ull);
                    const int32_t en = qc_dev_min_enc(q.x), ex = qc_dev_max_enc(q.x);
                    if (q.orient == QC_FR) { mn0 = en > mn0 ? en : mn0; mx0 = ex > mx0 ? ex : mx0; }
                    else if (q.orient == QC_RF) { mn1 = en > mn1 ? en : mn1; mx1 = ex > mx1 ? ex : mx1; }
                    else { mn2 = en > mn2 ? en : mn2; mx2 = ex > mx2 ? ex : mx2; }
                }
            }
        }
    }
    // the wave's part into LDS, then the workgroup's into the block: one global add per non-zero word
    if (lane < 2 * QC_F_N && f_acc) atomicAdd(&s_cnt[lane], f_acc);
    for (int k = 0; k < QC_S_N; ++k) {
        const unsigned long long t = qc_wave_sum(sums[k]);
        if (lane == 0 && t) atomicAdd(&s_cnt[2 * QC_F_N + k], t);
    }
    mn0 = qc_wave_max(mn0); mn1 = qc_wave_max(mn1); mn2 = qc_wave_max(mn2);
    mx0 = qc_wave_max(mx0); mx1 = qc_wave_max(mx1); mx2 = qc_wave_max(mx2);
    max_len = qc_wave_max(max_len);
    for (int o = 32; o > 0; o >>= 1) err |= __shfl_xor(err, o);
    if (lane == 0) {
        if (mn0) atomicMax(&s_ext[0], mn0);
        if (mn1) atomicMax(&s_ext[1], mn1);
        if (mn2) atomicMax(&s_ext[2], mn2);
        if (mx0) atomicMax(&s_ext[3], mx0);
        if (mx1) atomicMax(&s_ext[4], mx1);
        if (mx2) atomicMax(&s_ext[5], mx2);
        if (max_len) atomicMax(&s_ext[6], max_len);
        if (err) atomicOr(&s_ext[7], err);
    }
    __syncthreads();
    for (int j = tid; j < 2 * QC_F_N + QC_S_N; j += QC_THREADS) if (s_cnt[j]) atomicAdd(&v.blk[QC_W_FLAG + j], s_cnt[j]);
    for (int j = tid; j < BAMQC_MAPQ_BINS; j += QC_THREADS) if (s_mapq[j]) atomicAdd(&v.blk[QC_W_MAPQ + j], (unsigned long long)s_mapq[j]);
    for (int j = tid; j < QC_ORIENTATIONS * BAMQC_ISIZE_LDS; j += QC_THREADS)
        if (s_isize[j]) atomicAdd(&v.blk[QC_W_ISIZE + (j / BAMQC_ISIZE_LDS) * BAMQC_ISIZE_BINS + j % BAMQC_ISIZE_LDS], (unsigned long long)s_isize[j]);
    if (tid < 2 * QC_ORIENTATIONS && s_ext[tid]) atomicMax((int*)&v.blk[QC_W_ISIZE_MIN + tid], s_ext[tid]);      // (the low half of a little-endian word)
    if (tid == 6 && s_ext[6]) atomicMax((int*)&v.blk[QC_W_SUM + QC_S_MAX_LENGTH], s_ext[6]);
    if (tid == 7 && s_ext[7]) atomicOr((int*)&v.blk[QC_W_ERR], s_ext[7]);
}

// (b) qual_hist, by the lane groups of k_dup_scores: G lanes per item (8, or the wavefront for long reads).  The group walks its
// item's records itself (a handful of loads of one cache line), and for every primary record with qualities shares out the aligned
// 32-bit words of QUAL, the up to three bytes before the first and after the last going singly.  One copy of the histogram per wave
// in LDS, flushed once per workgroup.  Runs after k_qc_records found no error, and still checks every bound itself.
template <int G>
__global__ void __launch_bounds__(QC_THREADS) k_qc_qual(QcView v)
{
    __shared__ unsigned long long s_q[QC_THREADS / 64][BAMQC_QUAL_BINS];
    const int tid = (int)threadIdx.x, sub = tid % G, per = QC_THREADS / G;
    for (int j = tid; j < (QC_THREADS / 64) * BAMQC_QUAL_BINS; j += QC_THREADS) s_q[j / BAMQC_QUAL_BINS][j % BAMQC_QUAL_BINS] = 0;
    __syncthreads();
    unsigned long long* const h = s_q[tid >> 6];
    for (int64_t base = (int64_t)blockIdx.x * per; base < v.n_items; base += (int64_t)gridDim.x * per) {
        const int64_t i = base + tid / G;
        int64_t o = 0, hi = 0;
        if (i < v.n_items) { o = v.off[i]; hi = v.off[i + 1]; }
        while (hi - o >= BAMSORT_MIN_REC) {
            const uint8_t* rec = v.bam + o;
            const int64_t size = 4 + (int64_t)(int32_t)bamsort_ld32(rec);
            if (size < BAMSORT_MIN_REC || size > hi - o) break;
            const uint32_t f = qc_ld16(rec + 18);
            const int32_t n = (int32_t)bamsort_ld32(rec + 20);
            const int64_t qo = 36 + (int64_t)rec[12] + 4 * (int64_t)qc_ld16(rec + 16) + ((int64_t)n + 1) / 2;
            if (!(f & 0x900) && n > 0 && qo + n <= size && rec[qo] != 0xff) {
                const uint8_t* q = rec + qo;
                const int32_t lead = (int32_t)((4 - ((uintptr_t)q & 3)) & 3), head = n < lead ? n : lead;
                const int32_t nw = (n - head) >> 2, tail = n - head - 4 * nw;
                if (sub < head) atomicAdd(&h[qc_qual_bin(q[sub])], 1ull);
                const uint32_t* w = (const uint32_t*)(q + head);
                for (int32_t k = sub; k < nw; k += G) {
                    const uint32_t x = w[k];
                    const uint32_t b0 = qc_qual_bin(x & 0xff), b1 = qc_qual_bin(x >> 8 & 0xff), b2 = qc_qual_bin(x >> 16 & 0xff), b3 = qc_qual_bin(x >> 24);
                    if (b0 == b1 && b1 == b2 && b2 == b3) atomicAdd(&h[b0], 4ull);
                    else { atomicAdd(&h[b0], 1ull); atomicAdd(&h[b1], 1ull); atomicAdd(&h[b2], 1ull); atomicAdd(&h[b3], 1ull); }
                }
                if (sub < tail) atomicAdd(&h[qc_qual_bin(q[head + 4 * nw + sub])], 1ull);
            }
            o += size;
        }
    }
    __syncthreads();
    if (tid < BAMQC_QUAL_BINS) {
        unsigned long long t = 0;
        for (int wv = 0; wv < QC_THREADS / 64; ++wv) t += s_q[wv][tid];
        if (t) atomicAdd(&v.blk[QC_W_QUAL + tid], t);
    }
}

// ------------------------------------------------------------------ base-level QC: tables per sequencing cycle and GC bias (bam_baseqc.h)
#define BQC_THREADS 256
// A workgroup's 32-bit copy of a 64-bit word of the block.  For the batches of this library a copy cannot wrap: a workgroup adds at
// most 255 (one QUAL byte) per record to a word, and a call holds fewer than 2^31 / 36 records of 36 bytes or more in under 2 GiB.
// bwamem_hip_baseqc_add_records_device takes streams up to 2^40 bytes, for which no such bound holds, so a wrap is carried into the
// word itself: the flush then adds what is left, and the sum is exact for any stream.
static __device__ inline void bqc_lds_add(uint32_t* s, uint32_t x, unsigned long long* word)
{
    const uint32_t old = atomicAdd(s, x);
    if (old + x < old) atomicAdd(word, 1ull << 32);
}
// ... for a sum that may itself exceed 32 bits: the high part goes to the word directly
static __device__ inline void bqc_lds_add64(uint32_t* s, unsigned long long x, unsigned long long* word)
{
    bqc_lds_add(s, (uint32_t)x, word);
    if (x >> 32) atomicAdd(word, x >> 32 << 32);
}
// one count of a table: the workgroup's copy below BASEQC_LDS_CYCLES, the lane's register for the capped last bin, else HBM
template <typename C>
static __device__ inline void bqc_count(uint32_t* s_tab, unsigned long long* g_tab, int32_t e, int32_t bin, uint32_t x, C& cap)
{
    if (bin < BASEQC_LDS_CYCLES) bqc_lds_add(&s_tab[e * BASEQC_LDS_CYCLES + bin], x, &g_tab[e * BASEQC_CYCLES + bin]);
    else if (bin == BASEQC_CYCLES - 1) cap += x;
    else atomicAdd(&g_tab[e * BASEQC_CYCLES + bin], (unsigned long long)x);
}
static __device__ inline void bqc_flush(const uint32_t* s_tab, unsigned long long* g_tab, int tid)
{
    for (int j = tid; j < BASEQC_ENDS * BASEQC_LDS_CYCLES; j += BQC_THREADS)
        if (s_tab[j]) atomicAdd(&g_tab[(j / BASEQC_LDS_CYCLES) * BASEQC_CYCLES + j % BASEQC_LDS_CYCLES], (unsigned long long)s_tab[j]);
}

// (a) every check of bam_baseqc.h, one lane per item (a read's records, or one record): the errors, records[], qcfail_skipped and the
// longest contributing read.  Reads no reference byte; the other kernels run only when it leaves no error.
__global__ void __launch_bounds__(BQC_THREADS) k_bqc_check(BqcView v)
{
    __shared__ unsigned long long s_cnt[BASEQC_ENDS + 1];
    __shared__ int32_t s_ext[2];                                       // the longest read, the errors
    const int tid = (int)threadIdx.x, lane = tid & 63;
    if (tid < BASEQC_ENDS + 1) s_cnt[tid] = 0;
    if (tid < 2) s_ext[tid] = 0;
    __syncthreads();
    unsigned long long n[BASEQC_ENDS + 1] = { 0, 0, 0, 0 };
    int32_t max_len = 0, err = 0;
    for (int64_t i = (int64_t)blockIdx.x * BQC_THREADS + tid; i < v.n_items; i += (int64_t)gridDim.x * BQC_THREADS) {
        int64_t o = v.off[i];
        const int64_t hi = v.off[i + 1];
        while (o < hi) {
            int e = 0;
            int64_t size = 0;
            BqcRec r = {};
            if (hi - o < BAMSORT_MIN_REC) e = BASEQC_ERR_WALK;
            else {
                size = 4 + (int64_t)(int32_t)bamsort_ld32(v.bam + o);
                if (size < BAMSORT_MIN_REC || size > hi - o || (!v.grouped && size != hi - o)) e = BASEQC_ERR_WALK;
            }
            if (!e) e = bqc_fields(v.bam + o, size, v.n_contigs, r);
            if (!e && r.primary && !(r.f & 4)) e = bqc_mapped(v.bam + o, v.ann_len, r);
            if (e) { err |= e; break; }
            if (r.counted) {
                n[0] += r.e == 0; n[1] += r.e == 1; n[2] += r.e == 2;
                if (r.l_seq > max_len) max_len = r.l_seq;
            } else if (r.primary) n[BASEQC_ENDS] += 1;
            o += size;
        }
    }
    for (int k = 0; k < BASEQC_ENDS + 1; ++k) {
        const unsigned long long t = qc_wave_sum(n[k]);
        if (lane == 0 && t) atomicAdd(&s_cnt[k], t);
    }
    max_len = qc_wave_max(max_len);
    for (int o = 32; o > 0; o >>= 1) err |= __shfl_xor(err, o);
    if (lane == 0) {
        if (max_len) atomicMax(&s_ext[0], max_len);
        if (err) atomicOr(&s_ext[1], err);
    }
    __syncthreads();
    if (tid < BASEQC_ENDS + 1 && s_cnt[tid]) atomicAdd(&v.blk[BQ_W_RECORDS + tid], s_cnt[tid]);       // (qcfail_skipped follows records[])
    if (tid == 0 && s_ext[0]) atomicMax((int*)&v.blk[BQ_W_MAX_LEN], s_ext[0]);                        // (the low half of a little-endian word)
    if (tid == 0 && s_ext[1]) atomicOr((int*)&v.blk[BQ_W_ERR], s_ext[1]);
}

// The next record among the item's bytes [o, hi) that counts (mapped: that is a mapped primary and passes bqc_mapped): its fields in
// r, o behind it.  Every lane of a group takes the same steps.  Where the bytes do not chain the item ends (k_bqc_check has refused
// such a stream): every bound is checked again here.
static __device__ inline bool bqc_next(const BqcView& v, int64_t& o, int64_t hi, bool mapped, const uint8_t*& rec, BqcRec& r)
{
    while (hi - o >= BAMSORT_MIN_REC) {
        rec = v.bam + o;
        const int64_t size = 4 + (int64_t)(int32_t)bamsort_ld32(rec);
        if (size < BAMSORT_MIN_REC || size > hi - o) break;
        o += size;
        if (bqc_fields(rec, size, v.n_contigs, r) != 0) break;
        if (mapped ? r.mapped && bqc_mapped(rec, v.ann_len, r) == 0 : r.counted) return true;
    }
    o = hi;
    return false;
}

// (b) base[], qual_sum[] / qual_n[] and read_gc[], by lane groups of G lanes per item as k_qc_qual has them.  The group shares out the
// aligned 32-bit words of QUAL, the up to three bytes before the first and after the last going singly; a lane reads the SEQ bytes of
// its own indices.  The group's rounds are uniform over the wave: the reads' GC is summed over the group by shuffles.
template <int G>
__global__ void __launch_bounds__(BQC_THREADS) k_bqc_bases(BqcView v)
{
    __shared__ uint32_t s_base[BASEQC_ENDS * BASEQC_LDS_CYCLES * BASEQC_BASES], s_qs[BASEQC_ENDS * BASEQC_LDS_CYCLES], s_qn[BASEQC_ENDS * BASEQC_LDS_CYCLES];
    __shared__ uint32_t s_rgc[BASEQC_ENDS * BASEQC_GC_BINS];
    const int tid = (int)threadIdx.x, sub = tid % G, per = BQC_THREADS / G;
    for (int j = tid; j < BASEQC_ENDS * BASEQC_LDS_CYCLES * BASEQC_BASES; j += BQC_THREADS) s_base[j] = 0;
    for (int j = tid; j < BASEQC_ENDS * BASEQC_LDS_CYCLES; j += BQC_THREADS) { s_qs[j] = 0; s_qn[j] = 0; }
    for (int j = tid; j < BASEQC_ENDS * BASEQC_GC_BINS; j += BQC_THREADS) s_rgc[j] = 0;
    __syncthreads();
    unsigned long long* const g_base = v.blk + BQ_W_BASE;
    for (int64_t first = (int64_t)blockIdx.x * per; first < v.n_items; first += (int64_t)gridDim.x * per) {
        const int64_t i = first + tid / G;
        int64_t o = 0, hi = 0;
        if (i < v.n_items) { o = v.off[i]; hi = v.off[i + 1]; }
        for (;;) {
            BqcRec r = {};
            const uint8_t* rec = nullptr;
            const bool have = bqc_next(v, o, hi, false, rec, r);
            if (!wave_any(have)) break;
            uint32_t gc = 0, acgt = 0;
            if (have && r.l_seq > 0) {
                const uint8_t* seq = rec + r.seq_off;
                const uint8_t* q = rec + r.qual_off;
                const int32_t n = r.l_seq, e = r.e;
                const bool hq = q[0] != 0xff;
                uint32_t cap_b[BASEQC_BASES] = { 0, 0, 0, 0, 0 }, cap_qn = 0;
                unsigned long long cap_qs = 0;                                    // (up to 255 per base of a record of any length)
                auto put = [&](int64_t idx, uint32_t qv) {
                    const int32_t code = bqc_code(seq, idx), k = bqc_column(code, r.rev), bin = bqc_bin(r, idx);
                    if (code < 4) { ++acgt; gc += (code == 1 || code == 2) ? 1u : 0u; }
                    if (bin < BASEQC_LDS_CYCLES) {
                        const int32_t w = e * BASEQC_LDS_CYCLES + bin;
                        bqc_lds_add(&s_base[w * BASEQC_BASES + k], 1u, &g_base[(e * BASEQC_CYCLES + bin) * BASEQC_BASES + k]);
                    } else if (bin == BASEQC_CYCLES - 1) {
#pragma unroll
                        for (int kk = 0; kk < BASEQC_BASES; ++kk) cap_b[kk] += k == kk ? 1u : 0u;
                    } else atomicAdd(&g_base[(e * BASEQC_CYCLES + bin) * BASEQC_BASES + k], 1ull);
                    if (hq) {
                        bqc_count(s_qs, v.blk + BQ_W_QUAL_SUM, e, bin, qv, cap_qs);
                        bqc_count(s_qn, v.blk + BQ_W_QUAL_N, e, bin, 1u, cap_qn);
                    }
                };
                const int32_t lead = (int32_t)((4 - ((uintptr_t)q & 3)) & 3), head = n < lead ? n : lead;
                const int32_t nw = (n - head) >> 2, tail = n - head - 4 * nw;
                if (sub < head) put(sub, q[sub]);
                const uint32_t* w = (const uint32_t*)(q + head);
                for (int32_t k = sub; k < nw; k += G) {
                    const uint32_t x = w[k];
                    const int64_t i0 = (int64_t)head + 4 * (int64_t)k;
                    put(i0, x & 0xff); put(i0 + 1, x >> 8 & 0xff); put(i0 + 2, x >> 16 & 0xff); put(i0 + 3, x >> 24);
                }
                if (sub < tail) put((int64_t)head + 4 * (int64_t)nw + sub, q[head + 4 * nw + sub]);
                // the capped last bin: once per record and lane
                const int32_t last = e * BASEQC_CYCLES + BASEQC_CYCLES - 1;
#pragma unroll
                for (int kk = 0; kk < BASEQC_BASES; ++kk) if (cap_b[kk]) atomicAdd(&g_base[last * BASEQC_BASES + kk], (unsigned long long)cap_b[kk]);
                if (cap_qs) atomicAdd(&v.blk[BQ_W_QUAL_SUM + last], cap_qs);
                if (cap_qn) atomicAdd(&v.blk[BQ_W_QUAL_N + last], (unsigned long long)cap_qn);
            }
#pragma unroll
            for (int m = G / 2; m > 0; m >>= 1) { gc += __shfl_xor(gc, m); acgt += __shfl_xor(acgt, m); }
            if (have && sub == 0 && acgt) {
                const int32_t b = r.e * BASEQC_GC_BINS + bqc_read_gc_bin(gc, acgt);
                bqc_lds_add(&s_rgc[b], 1u, &v.blk[BQ_W_READ_GC + b]);
            }
        }
    }
    __syncthreads();
    for (int j = tid; j < BASEQC_ENDS * BASEQC_LDS_CYCLES * BASEQC_BASES; j += BQC_THREADS)
        if (s_base[j]) {
            const int w = j / BASEQC_BASES;
            atomicAdd(&g_base[((w / BASEQC_LDS_CYCLES) * BASEQC_CYCLES + w % BASEQC_LDS_CYCLES) * BASEQC_BASES + j % BASEQC_BASES], (unsigned long long)s_base[j]);
        }
    bqc_flush(s_qs, v.blk + BQ_W_QUAL_SUM, tid);
    bqc_flush(s_qn, v.blk + BQ_W_QUAL_N, tid);
    for (int j = tid; j < BASEQC_ENDS * BASEQC_GC_BINS; j += BQC_THREADS) if (s_rgc[j]) atomicAdd(&v.blk[BQ_W_READ_GC + j], (unsigned long long)s_rgc[j]);
}

// (c) the mapped primaries: aligned[], mism[], ins[], del_ev[], soft[] and the GC-bias window, by the same lane groups.  bqc_next has
// passed bqc_mapped for the record before a reference byte is read: the whole span lies inside the contig, hence inside the packed
// reference.  The lanes of a group share out the SEQ indices of every operation; the reference comes 16 bases per 32-bit load (a
// one-word cache per lane, as PacCache); lanes 0..7 of the group take one word of the window each for the masked popcount.
template <int G>
__global__ void __launch_bounds__(BQC_THREADS) k_bqc_aligned(BqcView v)
{
    __shared__ uint32_t s_al[BASEQC_ENDS * BASEQC_LDS_CYCLES], s_mm[BASEQC_ENDS * BASEQC_LDS_CYCLES], s_in[BASEQC_ENDS * BASEQC_LDS_CYCLES],
                        s_de[BASEQC_ENDS * BASEQC_LDS_CYCLES], s_so[BASEQC_ENDS * BASEQC_LDS_CYCLES];
    __shared__ uint32_t s_gcb[3 * BASEQC_GC_BINS];                     // gcb_reads, gcb_qual_sum, gcb_qual_n: a few GC counts take nearly every record
    const int tid = (int)threadIdx.x, sub = tid % G, per = BQC_THREADS / G;
    for (int j = tid; j < BASEQC_ENDS * BASEQC_LDS_CYCLES; j += BQC_THREADS) { s_al[j] = 0; s_mm[j] = 0; s_in[j] = 0; s_de[j] = 0; s_so[j] = 0; }
    for (int j = tid; j < 3 * BASEQC_GC_BINS; j += BQC_THREADS) s_gcb[j] = 0;
    __syncthreads();
    const uint32_t* const pacw = (const uint32_t*)v.pac;
    unsigned long long skipped = 0;
    for (int64_t first = (int64_t)blockIdx.x * per; first < v.n_items; first += (int64_t)gridDim.x * per) {
        const int64_t i = first + tid / G;
        int64_t o = 0, hi = 0;
        if (i < v.n_items) { o = v.off[i]; hi = v.off[i + 1]; }
        for (;;) {
            BqcRec r = {};
            const uint8_t* rec = nullptr;
            const bool have = bqc_next(v, o, hi, true, rec, r);
            if (!wave_any(have)) break;
            // the window: its validity by every lane, its GC by the words
            bool valid = false;
            uint32_t g = 0;
            int64_t ref0 = 0;
            if (have) {
                ref0 = v.ann_offset[r.refid];
                const int64_t s = r.rev ? (int64_t)r.pos + r.span - BASEQC_WINDOW : (int64_t)r.pos;
                valid = s >= 0 && s + BASEQC_WINDOW <= (int64_t)v.ann_len[r.refid] && bqc_window_clear(v.holes, v.n_holes, ref0 + s);
                const int64_t a = ref0 + s, b = a + BASEQC_WINDOW, wd = (a >> 4) + sub;
                if (valid && sub < 8 && wd * 16 < b) {
                    const int64_t lo = a > wd * 16 ? a : wd * 16, up = b < wd * 16 + 16 ? b : wd * 16 + 16;
                    g = (uint32_t)bqc_word_gc(*AS_GLOBAL(const uint32_t, pacw + wd), (int)(lo - wd * 16), (int)(up - wd * 16));
                }
            }
            g += __shfl_xor(g, 4); g += __shfl_xor(g, 2); g += __shfl_xor(g, 1);       // lanes 0..7 of the group: all of the window's words
            // the walk
            unsigned long long qsum = 0;
            if (have) {
                const uint8_t* seq = rec + r.seq_off;
                const uint8_t* q = rec + r.qual_off;
                const int32_t e = r.e;
                const bool wq = valid && r.l_seq > 0 && q[0] != 0xff;             // the window wants the sum of QUAL
                uint32_t cap_al = 0, cap_mm = 0, cap_in = 0, cap_de = 0, cap_so = 0;
                int64_t i0 = 0, p0 = ref0 + r.pos, cw = -1;
                uint32_t cv = 0;
                for (int32_t c = 0; c < r.n_cig; ++c) {
                    const uint32_t x = bamsort_ld32(rec + r.cig_off + 4 * (int64_t)c), op = x & 0xf;
                    const int64_t len = (int64_t)(x >> 4);
                    if (op == 0 || op == 7 || op == 8) {
                        // four consecutive bases per lane and step: their loads are issued together, then the counts
                        for (int64_t j4 = 4 * (int64_t)sub; j4 < len; j4 += 4 * G) {
                            const int nb = len - j4 < 4 ? (int)(len - j4) : 4;
                            bool mm[4] = { false, false, false, false };
#pragma unroll
                            for (int u = 0; u < 4; ++u)
                                if (u < nb) {
                                    const int64_t p = p0 + j4 + u;
                                    if (p >> 4 != cw) { cw = p >> 4; cv = *AS_GLOBAL(const uint32_t, pacw + cw); }
                                    mm[u] = bqc_code(seq, i0 + j4 + u) != bqc_word_base(cv, (int)(p & 15));
                                    if (wq) qsum += q[i0 + j4 + u];
                                }
#pragma unroll
                            for (int u = 0; u < 4; ++u)
                                if (u < nb) {
                                    const int32_t bin = bqc_bin(r, i0 + j4 + u);
                                    bqc_count(s_al, v.blk + BQ_W_ALIGNED, e, bin, 1u, cap_al);
                                    if (mm[u]) bqc_count(s_mm, v.blk + BQ_W_MISM, e, bin, 1u, cap_mm);
                                }
                        }
                        i0 += len; p0 += len;
                    } else if (op == 1 || op == 4) {
                        for (int64_t j = sub; j < len; j += G) {
                            const int32_t bin = bqc_bin(r, i0 + j);
                            if (op == 1) bqc_count(s_in, v.blk + BQ_W_INS, e, bin, 1u, cap_in);
                            else bqc_count(s_so, v.blk + BQ_W_SOFT, e, bin, 1u, cap_so);
                            if (wq) qsum += q[i0 + j];
                        }
                        i0 += len;
                    } else if (op == 2) {
                        if (sub == 0) bqc_count(s_de, v.blk + BQ_W_DEL, e, bqc_bin(r, i0 - 1), 1u, cap_de);
                        p0 += len;
                    } else if (op == 3) p0 += len;
                }
                const int32_t last = e * BASEQC_CYCLES + BASEQC_CYCLES - 1;       // the capped last bin: once per record and lane
                if (cap_al) atomicAdd(&v.blk[BQ_W_ALIGNED + last], (unsigned long long)cap_al);
                if (cap_mm) atomicAdd(&v.blk[BQ_W_MISM + last], (unsigned long long)cap_mm);
                if (cap_in) atomicAdd(&v.blk[BQ_W_INS + last], (unsigned long long)cap_in);
                if (cap_de) atomicAdd(&v.blk[BQ_W_DEL + last], (unsigned long long)cap_de);
                if (cap_so) atomicAdd(&v.blk[BQ_W_SOFT + last], (unsigned long long)cap_so);
            }
#pragma unroll
            for (int m = G / 2; m > 0; m >>= 1) qsum += __shfl_xor(qsum, m);
            if (have && sub == 0) {
                if (!valid) skipped += 1;
                else {
                    bqc_lds_add(&s_gcb[g], 1u, &v.blk[BQ_W_GCB_READS + g]);
                    if (r.l_seq > 0 && rec[r.qual_off] != 0xff) {
                        bqc_lds_add64(&s_gcb[BASEQC_GC_BINS + g], qsum, &v.blk[BQ_W_GCB_QUAL_SUM + g]);
                        bqc_lds_add(&s_gcb[2 * BASEQC_GC_BINS + g], (uint32_t)r.l_seq, &v.blk[BQ_W_GCB_QUAL_N + g]);
                    }
                }
            }
        }
    }
    skipped = qc_wave_sum(skipped);
    if ((tid & 63) == 0 && skipped) atomicAdd(&v.blk[BQ_W_GCB_SKIPPED], skipped);
    __syncthreads();
    bqc_flush(s_al, v.blk + BQ_W_ALIGNED, tid);
    bqc_flush(s_mm, v.blk + BQ_W_MISM, tid);
    bqc_flush(s_in, v.blk + BQ_W_INS, tid);
    bqc_flush(s_de, v.blk + BQ_W_DEL, tid);
    bqc_flush(s_so, v.blk + BQ_W_SOFT, tid);
    for (int j = tid; j < 3 * BASEQC_GC_BINS; j += BQC_THREADS) if (s_gcb[j]) atomicAdd(&v.blk[BQ_W_GCB_READS + j], (unsigned long long)s_gcb[j]);      // (the three tables follow each other)
}

// windows[]: the valid window starts of the whole packed reference by GC count.  A workgroup stages a tile of GCW_TILE bases plus the
// 25 bytes of the last start's window in LDS with coalesced 32-bit loads; a lane slides over GCW_RUN consecutive starts, adding the
// base that enters and dropping the one that leaves.  The run's contig and its first hole come from one binary search each and are
// walked from there.  (60 starts are 15 bytes: the lanes' bytes fall in different banks.)
enum { GCW_THREADS = 256, GCW_RUN = 60, GCW_TILE = GCW_THREADS * GCW_RUN, GCW_BYTES = GCW_TILE / 4 + 28 };
static_assert(GCW_RUN % 4 == 0 && GCW_BYTES % 4 == 0 && GCW_BYTES >= (GCW_TILE + BASEQC_WINDOW + 3) / 4, "a tile starts on a byte and holds the last window");
__global__ void __launch_bounds__(GCW_THREADS) k_gc_windows(GcWinView v)
{
    __shared__ uint32_t s_pac[GCW_BYTES / 4];
    __shared__ uint32_t s_h[BASEQC_GC_BINS];
    const int tid = (int)threadIdx.x;
    if (tid < BASEQC_GC_BINS) s_h[tid] = 0;
    const uint8_t* const sb = (const uint8_t*)s_pac;
    const int64_t n_tiles = (v.l_pac + GCW_TILE - 1) / GCW_TILE;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t t0 = tile * GCW_TILE, byte0 = t0 >> 2;
        __syncthreads();                                                 // (the tile before is done with; s_h is zeroed)
        for (int j = tid; j < GCW_BYTES / 4; j += GCW_THREADS)
            s_pac[j] = byte0 + 4 * (int64_t)j < v.pac_bytes ? *AS_GLOBAL(const uint32_t, (const uint32_t*)(v.pac + byte0) + j) : 0u;
        __syncthreads();
        const int64_t g0 = t0 + (int64_t)tid * GCW_RUN, g1 = g0 + GCW_RUN < v.l_pac ? g0 + GCW_RUN : v.l_pac;
        if (g0 >= g1) continue;
        int32_t c = 0;
        {   // the contig of g0: the last one that starts at or before it
            int32_t lo = 0, hi = v.n_contigs - 1;
            while (lo < hi) { const int32_t mid = lo + (hi - lo + 1) / 2; if (v.ann_offset[mid] <= g0) lo = mid; else hi = mid - 1; }
            c = lo;
        }
        int64_t cend = v.ann_offset[c] + v.ann_len[c];
        int32_t hk = bqc_first_hole(v.holes, v.n_holes, g0);
        auto is_gc = [&](int64_t rel) { const uint32_t b = sb[rel >> 2] >> ((~rel & 3) << 1) & 3u; return (int32_t)((b ^ b >> 1) & 1u); };
        int32_t gc = 0;
        for (int j = 0; j < BASEQC_WINDOW; ++j) gc += is_gc(g0 - t0 + j);
        for (int64_t g = g0; g < g1; ++g) {
            while (g >= cend && c + 1 < v.n_contigs) { ++c; cend = v.ann_offset[c] + v.ann_len[c]; }
            while (hk < v.n_holes && v.holes[hk].end <= g) ++hk;
            if (g + BASEQC_WINDOW <= cend && (hk >= v.n_holes || v.holes[hk].off >= g + BASEQC_WINDOW)) bqc_lds_add(&s_h[gc], 1u, &v.out[gc]);
            gc += is_gc(g - t0 + BASEQC_WINDOW) - is_gc(g - t0);
        }
    }
    __syncthreads();
    if (tid < BASEQC_GC_BINS && s_h[tid]) atomicAdd(&v.out[tid], (unsigned long long)s_h[tid]);
}

static int qc_grid(int64_t n_blocks, int n_cu, int per_cu)
{
    const int64_t cap = (int64_t)(n_cu > 0 ? n_cu : 1) * per_cu;
    return (int)(n_blocks < 1 ? 1 : n_blocks < cap ? n_blocks : cap);
}
void launch_qc_records(hipStream_t st, const QcView& v, int n_cu)
{
    hipLaunchKernelGGL(k_qc_records, dim3(qc_grid(((int64_t)v.n_items + QC_THREADS - 1) / QC_THREADS, n_cu, 8)), dim3(QC_THREADS), 0, st, v);
}
void launch_qc_qual(hipStream_t st, const QcView& v, int max_len, int n_cu)
{
    if (max_len > 1000) hipLaunchKernelGGL(k_qc_qual<64>, dim3(qc_grid(((int64_t)v.n_items + 3) / 4, n_cu, 16)), dim3(QC_THREADS), 0, st, v);      // long reads: a wavefront per read
    else hipLaunchKernelGGL(k_qc_qual<8>, dim3(qc_grid(((int64_t)v.n_items + 31) / 32, n_cu, 16)), dim3(QC_THREADS), 0, st, v);
}
// The grids of the base-level QC: k_bqc_bases keeps 22.2 KiB of LDS and k_bqc_aligned 16.2 KiB, so six and eight workgroups of four
// waves fit a CU's 160 KiB beside each other with room to spare; the grid is that many per CU and strides over the rest.
void launch_bqc_check(hipStream_t st, const BqcView& v, int n_cu)
{
    hipLaunchKernelGGL(k_bqc_check, dim3(qc_grid(((int64_t)v.n_items + BQC_THREADS - 1) / BQC_THREADS, n_cu, 8)), dim3(BQC_THREADS), 0, st, v);
}
void launch_bqc_bases(hipStream_t st, const BqcView& v, int max_len, int n_cu)
{
    if (max_len > 1000) hipLaunchKernelGGL(k_bqc_bases<64>, dim3(qc_grid(((int64_t)v.n_items + 3) / 4, n_cu, 6)), dim3(BQC_THREADS), 0, st, v);      // long reads: a wavefront per read
    else hipLaunchKernelGGL(k_bqc_bases<8>, dim3(qc_grid(((int64_t)v.n_items + 31) / 32, n_cu, 6)), dim3(BQC_THREADS), 0, st, v);
}
void launch_bqc_aligned(hipStream_t st, const BqcView& v, int max_len, int n_cu)
{
    if (max_len > 1000) hipLaunchKernelGGL(k_bqc_aligned<64>, dim3(qc_grid(((int64_t)v.n_items + 3) / 4, n_cu, 8)), dim3(BQC_THREADS), 0, st, v);
    else hipLaunchKernelGGL(k_bqc_aligned<8>, dim3(qc_grid(((int64_t)v.n_items + 31) / 32, n_cu, 8)), dim3(BQC_THREADS), 0, st, v);
}
void launch_gc_windows(hipStream_t st, const GcWinView& v, int n_cu)
{
    hipLaunchKernelGGL(k_gc_windows, dim3(qc_grid((v.l_pac + GCW_TILE - 1) / GCW_TILE, n_cu, 8)), dim3(GCW_THREADS), 0, st, v);
}

void launch_dup_entries(hipStream_t st, const DupView& v)
{
    hipLaunchKernelGGL(k_dup_entries, dim3((v.n_tmpl + 63) / 64), dim3(64), 0, st, v);
}
void launch_dup_scores(hipStream_t st, const DupView& v, int max_len)
{
    if (max_len > 1000) hipLaunchKernelGGL(k_dup_scores<64>, dim3((v.n_reads + 3) / 4), dim3(256), 0, st, v);      // long reads: a wavefront per read
    else hipLaunchKernelGGL(k_dup_scores<8>, dim3((v.n_reads + 31) / 32), dim3(256), 0, st, v);
}
void launch_dup_score_keys(hipStream_t st, const DupView& v, uint64_t* frag_key, uint64_t* pair_key)
{
    hipLaunchKernelGGL(k_dup_score_keys, dim3((v.n_reads + 255) / 256), dim3(256), 0, st, v, frag_key, pair_key);
}
void launch_dup_gather(hipStream_t st, const uint64_t* src, const uint32_t* idx, int n, uint64_t* out)
{
    hipLaunchKernelGGL(k_dup_gather, dim3((n + 255) / 256), dim3(256), 0, st, src, idx, n, out);
}
void launch_dup_decide(hipStream_t st, const uint64_t* keys, const uint32_t* idx, const uint64_t* second, int n, const uint8_t* is_paired, uint8_t* dup)
{
    hipLaunchKernelGGL(k_dup_decide, dim3((n + 255) / 256), dim3(256), 0, st, keys, idx, second, n, is_paired, dup);
}
void launch_dup_flags(hipStream_t st, const DupView& v)
{
    hipLaunchKernelGGL(k_dup_flags, dim3((v.n_tmpl + 63) / 64), dim3(64), 0, st, v);
}

void launch_sort_bits(hipStream_t st, const uint64_t* keys, int64_t n, int32_t* bits)
{
    if (n <= 0) return;
    const int64_t g = (n + SORT_TILE - 1) / SORT_TILE;
    hipLaunchKernelGGL(k_sort_bits, dim3((unsigned)(g < 1024 ? g : 1024)), dim3(SORT_THREADS), 0, st, keys, n, bits);
}
void launch_sort_hist(hipStream_t st, const uint64_t* keys, int64_t n, int byte, int32_t* hist)
{
    const int nt = (int)sort_n_tiles(n);
    hipLaunchKernelGGL(k_sort_hist, dim3(nt), dim3(SORT_THREADS), 0, st, keys, n, byte, nt, hist);
}
void launch_sort_scatter(hipStream_t st, const uint64_t* keys, const uint32_t* idx, int64_t n, int byte, const int64_t* off, uint64_t* keys_out, uint32_t* idx_out)
{
    const int nt = (int)sort_n_tiles(n);
    hipLaunchKernelGGL(k_sort_scatter, dim3(nt), dim3(SORT_THREADS), 0, st, keys, idx, n, byte, nt, off, keys_out, idx_out);
}
void launch_bamrec_count(hipStream_t st, const uint8_t* bam, const int64_t* bam_off, int n_reads, int32_t* counts, int32_t* bits, int32_t* err)
{
    hipLaunchKernelGGL(k_bamrec_count, dim3((n_reads + 63) / 64), dim3(64), 0, st, bam, bam_off, n_reads, counts, bits, err);
}
void launch_bamrec_keys(hipStream_t st, const uint8_t* bam, const int64_t* bam_off, int n_reads, const int64_t* first, uint64_t* keys, int64_t* src_off, int32_t* sizes)
{
    hipLaunchKernelGGL(k_bamrec_keys, dim3((n_reads + 63) / 64), dim3(64), 0, st, bam, bam_off, n_reads, first, keys, src_off, sizes);
}
void launch_bamrec_sizes(hipStream_t st, const uint32_t* idx, const int32_t* sizes, int n, int32_t* out)
{
    hipLaunchKernelGGL(k_bamrec_sizes, dim3((n + 255) / 256), dim3(256), 0, st, idx, sizes, n, out);
}
void launch_bamrec_gather(hipStream_t st, const uint8_t* src, const int64_t* src_off, const uint32_t* idx, const int64_t* dst_off, int n_rec, int64_t total, uint8_t* dst)
{
    hipLaunchKernelGGL(k_bamrec_gather, dim3((unsigned)((total + BAMSORT_CHUNK - 1) / BAMSORT_CHUNK)), dim3(256), 0, st, src, src_off, idx, dst_off, n_rec, total, dst);
}
void launch_bai_records(hipStream_t st, const BaiView& v)
{
    hipLaunchKernelGGL(k_bai_records, dim3((v.n_rec + 63) / 64), dim3(64), 0, st, v);
}
void launch_bai_mark(hipStream_t st, const uint64_t* keys, const uint32_t* idx, int n, int32_t* start)
{
    hipLaunchKernelGGL(k_bai_mark, dim3((n + 255) / 256), dim3(256), 0, st, keys, idx, n, start);
}
void launch_bai_chunks(hipStream_t st, const uint64_t* keys, const uint32_t* idx, int n, const int32_t* start, const int64_t* cid, const int64_t* rec_off,
                       const int64_t* member_off, int64_t coffset0, BaiChunk* out)
{
    hipLaunchKernelGGL(k_bai_chunks, dim3((n + 255) / 256), dim3(256), 0, st, keys, idx, n, start, cid, rec_off, member_off, coffset0, out);
}
void launch_bai_windows(hipStream_t st, const int32_t* win, int n_win, int n_rec, const int64_t* rec_off, const int64_t* member_off, int64_t coffset0, uint64_t* out)
{
    hipLaunchKernelGGL(k_bai_windows, dim3((n_win + 255) / 256), dim3(256), 0, st, win, n_win, n_rec, rec_off, member_off, coffset0, out);
}

int bgzf_grid(int n_cu, int64_t n_blocks)
{
    const int64_t g = 4ll * (n_cu > 0 ? n_cu : 256);
    return (int)(n_blocks < g ? n_blocks : g);
}
size_t bgzf_token_bytes(int grid) { return (size_t)grid * BGZF_IN * sizeof(uint32_t); }
void launch_bgzf_deflate(hipStream_t st, const uint8_t* src, int64_t n, int n_blocks, int grid, uint8_t* slots, int32_t* sizes, uint32_t* tokens)
{
    if (n_blocks <= 0) return;
    hipLaunchKernelGGL(k_bgzf_deflate, dim3(grid), dim3(BGZ_THREADS), 0, st, src, n, n_blocks, slots, sizes, tokens);
}
void launch_bgzf_gather(hipStream_t st, const uint8_t* slots, const int32_t* sizes, const int64_t* off, int n_blocks, bool with_eof, uint8_t* out)
{
    hipLaunchKernelGGL(k_bgzf_gather, dim3(n_blocks + 1), dim3(256), 0, st, slots, sizes, off, n_blocks, with_eof ? 1 : 0, out);
}

void launch_bgzf_inflate(hipStream_t st, const uint8_t* comp, const BgzfMember* mem, int n_members, int member0, uint8_t* text, int32_t* err)
{
    if (n_members > 0) hipLaunchKernelGGL(k_bgzf_inflate, dim3((unsigned)n_members), dim3(BGZI_THREADS), 0, st, comp, mem, n_members, member0, text, err);
}

void launch_bam_size(hipStream_t st, const BamTile& t)
{
    if (t.n_reads <= 0) return;
    if (t.tags) hipLaunchKernelGGL(k_bam_size<true>, dim3((t.n_reads + 63) / 64), dim3(64), 0, st, t);
    else hipLaunchKernelGGL(k_bam_size<false>, dim3((t.n_reads + 63) / 64), dim3(64), 0, st, t);
}
template <bool TAGS>
static void launch_bam_emit_t(hipStream_t st, const BamTile& t)
{
    if (t.max_len > 1000) {                                          // long reads: a wavefront per read
        if (t.qual) hipLaunchKernelGGL((k_bam_emit<64, true, TAGS>), dim3((t.n_reads + 3) / 4), dim3(256), 0, st, t);
        else hipLaunchKernelGGL((k_bam_emit<64, false, TAGS>), dim3((t.n_reads + 3) / 4), dim3(256), 0, st, t);
    } else if (t.qual) hipLaunchKernelGGL((k_bam_emit<8, true, TAGS>), dim3((t.n_reads + 31) / 32), dim3(256), 0, st, t);
    else hipLaunchKernelGGL((k_bam_emit<8, false, TAGS>), dim3((t.n_reads + 31) / 32), dim3(256), 0, st, t);
}
void launch_bam_emit(hipStream_t st, const BamTile& t)
{
    if (t.n_reads <= 0) return;
    if (t.tags) launch_bam_emit_t<true>(st, t); else launch_bam_emit_t<false>(st, t);
}
void launch_bam_tag_size(hipStream_t st, const BamTile& t)
{
    if (t.n_reads <= 0) return;
    hipLaunchKernelGGL(k_bam_tag_size, dim3((t.n_reads + 63) / 64), dim3(64), 0, st, t);
}
void launch_bam_tag_text(hipStream_t st, const BamTile& t)
{
    if (t.n_reads <= 0) return;
    if (t.max_len > 1000) hipLaunchKernelGGL(k_bam_tag_text<64>, dim3((t.n_reads + 3) / 4), dim3(256), 0, st, t);
    else hipLaunchKernelGGL(k_bam_tag_text<8>, dim3((t.n_reads + 31) / 32), dim3(256), 0, st, t);
}

void launch_qual_check(hipStream_t st, const uint8_t* raw, const uint8_t* qual, const int64_t* raw_off, int n_reads, int32_t* err)
{
    if (n_reads <= 0) return;
    hipLaunchKernelGGL(k_qual_check, dim3((n_reads + 63) / 64), dim3(64), 0, st, raw, qual, raw_off, n_reads, err);
}
void launch_mate_names(hipStream_t st, const uint8_t* names, const int64_t* name_off, int n_pairs, int32_t* err)
{
    if (n_pairs <= 0) return;
    hipLaunchKernelGGL(k_mate_names, dim3((n_pairs + 63) / 64), dim3(64), 0, st, names, name_off, n_pairs, err);
}
void launch_fastq_count(hipStream_t st, const uint8_t* text, int64_t n, int32_t* counts)
{
    hipLaunchKernelGGL(k_fastq_count, dim3((unsigned)fastq_n_chunks(n)), dim3(FASTQ_THREADS), 0, st, text, n, counts);
}
void launch_fastq_starts(hipStream_t st, const FastqText& t)
{
    hipLaunchKernelGGL(k_fastq_starts, dim3((unsigned)fastq_n_chunks(t.n)), dim3(FASTQ_THREADS), 0, st, t);
}
void launch_fastq_records(hipStream_t st, const FastqText& t, const FastqOut& o)
{
    if (t.n_rec <= 0) return;
    hipLaunchKernelGGL(k_fastq_records, dim3((t.n_rec + 63) / 64), dim3(64), 0, st, t, o);
}
void launch_fastq_copy(hipStream_t st, const FastqText& t, const FastqOut& o, int max_len)
{
    if (t.n_rec <= 0) return;
    if (max_len > 1000) hipLaunchKernelGGL(k_fastq_copy<64>, dim3((t.n_rec + 3) / 4), dim3(256), 0, st, t, o);     // long reads: a wavefront per read
    else hipLaunchKernelGGL(k_fastq_copy<8>, dim3((t.n_rec + 31) / 32), dim3(256), 0, st, t, o);
}

void launch_post1(hipStream_t st, const DevIndex& ix, const MemOpt& opt, const TileView& tv)
{
    if (tv.n_reads <= 0) return;
    if (tv.max_len > 1000) {                                         // long reads: a wavefront per read
        int ring = 64;
        long long need = 8ll * (opt.w > 0 ? opt.w : 0) + 16;
        if (need > (long long)tv.max_len + 4) need = (long long)tv.max_len + 4;
        if (need > 4096) need = 4096;
        while (ring < need) ring <<= 1;
        hipLaunchKernelGGL(k_post1<true>, dim3(tv.n_reads), dim3(64), 3 * (size_t)ring * sizeof(int32_t), st, ix, opt, tv, ring);
        return;
    }
    hipLaunchKernelGGL(k_post1<false>, dim3((tv.n_reads + 63) / 64), dim3(64), 0, st, ix, opt, tv, 64);
}
void launch_final_prep(hipStream_t st, const DevIndex& ix, const MemOpt& opt, const TileView& tv)
{
    if (tv.n_reads <= 0) return;
    hipLaunchKernelGGL(k_final_prep, dim3((tv.n_reads + 63) / 64), dim3(64), 0, st, ix, opt, tv);
}
void launch_final_se(hipStream_t st, const DevIndex& ix, const MemOpt& opt, const TileView& tv, const void* job_out, const uint32_t* job_cig, int cig_cap)
{
    if (tv.n_reads <= 0) return;
    JobView jv; jv.out = (const DpOut*)job_out; jv.cig = job_cig; jv.cig_cap = cig_cap;
    hipLaunchKernelGGL(k_final_se, dim3((tv.n_reads + 63) / 64), dim3(64), 0, st, ix, opt, tv, jv);
}
void launch_pack(hipStream_t st, const TileView& tv, uint8_t* dst)
{
    if (tv.n_reads <= 0) return;
    hipLaunchKernelGGL(k_pack, dim3((tv.n_reads + 31) / 32), dim3(256), 0, st, tv, dst);
}
