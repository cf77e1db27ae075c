// sam_writer.cpp -- SAM text on the native side (additive, not part of the reference ABI).
//
// GATK callers decode the response of jnibwa_createAlignments into BwaMemAlignment objects (BwaMemAligner.java:215-308) and
// re-encode those as SAM records themselves.  bwamem_hip_response_to_sam does that round trip natively: it walks the request
// (pSeq: count + NUL-terminated base strings, BwaMemAligner.java:198-209) and the response (layout of jnibwa.c:43-98) side by
// side and writes one SAM line per record.  The reference contains no SAM writer, so the line layout follows the SAM
// specification and, where the specification leaves a choice, upstream's mem_aln2sam (bwamem.c) as this repository restates it:
//   * FLAG is the record's flag (strand, mate, secondary and supplementary bits are already there: BwaMemIndexTest.java:84-127 pins
//     0x61/0x63/0x91/0x93 on the response itself);
//   * records after a read's first one turn soft clips into hard clips and carry only the aligned bases (upstream without -Y);
//   * SEQ is the read as sequenced for forward alignments, its reverse complement for reverse ones; QUAL is '*' (the request has none);
//     bwamem_hip_response_to_sam_q takes the qualities next to the request and writes them in the order of SEQ (reversed, clipped),
//     and ends every line with RG:Z:<ID> when given a read group;
//   * RNEXT/PNEXT/TLEN from the record's mate fields ("=" for the same contig); unmapped reads of a pair take their mate's place;
//   * tags NM:i MD:Z AS:i XS:i and XA:Z when the record has them.
// Read names: supplied by the caller, else "r<index>" (paired: "p<pair index>" for both mates).
// Two deliberate deviations from upstream's text are kept: a secondary record carries its SEQ (upstream writes '*'), and records
// on ALT contigs keep their soft clips as the rule above treats every later record (upstream keeps soft clips on ALT hits).
//
// The BAM encoder (bam_encode.h, kernels in k_post.hip) is bound to the same rules: a BAM record must decode to exactly the line
// written here for the same response record, the two deviations included.  This file also holds the host side of the BAM
// path: the uncompressed BAM header, BGZF framing by worker threads, and bwamem_hip_align_to_bam.
// BGZF (SAM specification 4.1): blocks of at most 0xff00 input bytes, each a gzip member with the BC extra field, then the
// 28-byte EOF block.  Level 0 writes stored deflate blocks with a CRC-32 of its own and needs nothing else; levels 1..9 take
// compress2 and crc32 from libz.so.1, loaded at run time (a zlib stream minus its 2-byte header and 4-byte Adler-32 trailer is
// the raw deflate stream a gzip member wants).  Without that library levels >= 1 fail and level 0 still works.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <errno.h>
#include <unistd.h>
#include <dlfcn.h>
#include <algorithm>
#include <atomic>
#include <string>
#include <thread>
#include <vector>
#include "bam_encode.h"
#include "bam_qc.h"
#include "bam_baseqc.h"
#include "index_io.h"
#include "../../include/bwamem_hip.h"

namespace {

struct Out {
    std::string s;
    void put(const char* p) { s += p; }
    void put(const std::string& p) { s += p; }
    void num(long long v) { char b[32]; snprintf(b, sizeof b, "%lld", v); s += b; }
    void ch(char c) { s.push_back(c); }
};

inline int32_t rd32(const uint8_t*& p) { int32_t v; memcpy(&v, p, 4); p += 4; return v; }

inline char comp(char c)
{
    switch (c) { case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A';
                 case 'a': return 't'; case 'c': return 'g'; case 'g': return 'c'; case 't': return 'a'; default: return c; }
}

// ---- BGZF
const size_t BGZF_BLOCK = 0xff00;                       // input bytes per block at most
const size_t BGZF_OVERHEAD = 18 + 5 + 8;                // header, one stored-block header, CRC32 + ISIZE
const uint8_t BGZF_EOF[28] = { 0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0 };

struct Crc32 {                                          // slice-by-8, reflected polynomial 0xEDB88320
    uint32_t t[8][256];
    Crc32() {
        for (uint32_t i = 0; i < 256; ++i) { uint32_t c = i; for (int k = 0; k < 8; ++k) c = c & 1 ? 0xEDB88320u ^ (c >> 1) : c >> 1; t[0][i] = c; }
        for (uint32_t i = 0; i < 256; ++i) for (int k = 1; k < 8; ++k) t[k][i] = t[0][t[k - 1][i] & 0xff] ^ (t[k - 1][i] >> 8);
    }
    uint32_t of(const uint8_t* p, size_t n) const {
        uint32_t c = 0xffffffffu;
        while (n >= 8) {
            uint32_t a, b; memcpy(&a, p, 4); memcpy(&b, p + 4, 4);
            a ^= c;
            c = t[7][a & 0xff] ^ t[6][a >> 8 & 0xff] ^ t[5][a >> 16 & 0xff] ^ t[4][a >> 24] ^ t[3][b & 0xff] ^ t[2][b >> 8 & 0xff] ^ t[1][b >> 16 & 0xff] ^ t[0][b >> 24];
            p += 8; n -= 8;
        }
        while (n--) c = t[0][(c ^ *p++) & 0xff] ^ (c >> 8);
        return ~c;
    }
};
const Crc32& crc_tab() { static const Crc32 c; return c; }

struct Zlib {                                           // compress2 and crc32 of libz.so.1, if it is there
    typedef int (*compress2_t)(unsigned char*, unsigned long*, const unsigned char*, unsigned long, int);
    typedef unsigned long (*crc32_t)(unsigned long, const unsigned char*, unsigned int);
    compress2_t compress2 = nullptr; crc32_t crc32 = nullptr;
    // ... and its inflate, for plain gzip streams (bwamem_gunzip_host).  z_stream as zlib 1.2 and later lay it out.
    struct Stream {
        const unsigned char* next_in; unsigned avail_in; unsigned long total_in;
        unsigned char* next_out; unsigned avail_out; unsigned long total_out;
        const char* msg; void* state; void* zalloc; void* zfree; void* opaque; int data_type; unsigned long adler, reserved;
    };
    typedef int (*inflate_init2_t)(Stream*, int, const char*, int);
    typedef int (*inflate_t)(Stream*, int);
    typedef int (*inflate_end_t)(Stream*);
    inflate_init2_t inflateInit2_ = nullptr; inflate_t inflate = nullptr; inflate_end_t inflateReset = nullptr, inflateEnd = nullptr;
    Zlib() {
        void* h = dlopen("libz.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!h) return;
        compress2 = (compress2_t)dlsym(h, "compress2"); crc32 = (crc32_t)dlsym(h, "crc32");
        if (!compress2 || !crc32) compress2 = nullptr, crc32 = nullptr;
        inflateInit2_ = (inflate_init2_t)dlsym(h, "inflateInit2_"); inflate = (inflate_t)dlsym(h, "inflate");
        inflateReset = (inflate_end_t)dlsym(h, "inflateReset"); inflateEnd = (inflate_end_t)dlsym(h, "inflateEnd");
        if (!inflateInit2_ || !inflate || !inflateReset || !inflateEnd) inflateInit2_ = nullptr;
    }
};
const Zlib& zlib() { static const Zlib z; return z; }

inline void le16(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }
inline void le32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

// one BGZF block of n <= BGZF_BLOCK input bytes into dst (room for n + BGZF_OVERHEAD) -> its size
size_t bgzf_block(const uint8_t* src, size_t n, int level, uint8_t* dst)
{
    static const uint8_t head[16] = { 0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0 };
    memcpy(dst, head, 16);
    uint8_t* c = dst + 18;
    size_t n_c = 0;
    if (level > 0) {
        // the zlib stream lands two bytes early, so that its deflate data starts at c; the two bytes it overwrites are rewritten below
        unsigned long len = (unsigned long)(n + BGZF_OVERHEAD - 16);
        if (zlib().compress2(dst + 16, &len, src, (unsigned long)n, level) == 0 && len >= 6 && len - 6 <= n + 5) n_c = (size_t)len - 6;
    }
    if (n_c == 0) {                                     // level 0 (or deflate made it longer): one stored block
        c[0] = 1; le16(c + 1, (uint32_t)n); le16(c + 3, ~(uint32_t)n & 0xffff);
        if (n) memcpy(c + 5, src, n);
        n_c = n + 5;
    }
    const size_t total = 18 + n_c + 8;
    le16(dst + 16, (uint32_t)(total - 1));
    const uint32_t crc = level > 0 ? (uint32_t)zlib().crc32(zlib().crc32(0, nullptr, 0), src, (unsigned int)n) : crc_tab().of(src, n);
    le32(c + n_c, crc); le32(c + n_c + 4, (uint32_t)n);
    return total;
}

int bgzf_threads(int n_threads, size_t n_blocks)
{
    int cap = 16;                                       // not the machine's core count: the process shares the host with others
    { const char* e = getenv("BWAMEM_HIP_BGZF_MAX_THREADS"); if (e && atoi(e) > 0) cap = atoi(e); }
    if (n_threads <= 0 || n_threads > cap) n_threads = cap;
    if ((size_t)n_threads > n_blocks) n_threads = (int)n_blocks;
    return n_threads < 1 ? 1 : n_threads;
}

// src as BGZF blocks (+ the EOF block): malloc'ed, or null
uint8_t* bgzf_compress(const uint8_t* src, size_t n, int level, int n_threads, bool with_eof, size_t* out_bytes)
{
    *out_bytes = 0;
    if (level < 0 || level > 9 || (n && !src)) return nullptr;
    if (level > 0 && !zlib().compress2) { fprintf(stderr, "[bwamem_hip] bgzf: libz.so.1 could not be loaded; only level 0 is available\n"); return nullptr; }
    const size_t n_blocks = (n + BGZF_BLOCK - 1) / BGZF_BLOCK, slot = BGZF_BLOCK + BGZF_OVERHEAD;
    uint8_t* out = (uint8_t*)malloc(n_blocks * slot + sizeof BGZF_EOF);
    if (!out) return nullptr;
    std::vector<uint32_t> size(n_blocks);
    std::atomic<size_t> next(0);
    auto work = [&]() {
        for (;;) {
            const size_t i = next++;
            if (i >= n_blocks) return;
            const size_t at = i * BGZF_BLOCK, len = n - at < BGZF_BLOCK ? n - at : BGZF_BLOCK;
            size[i] = (uint32_t)bgzf_block(src + at, len, level, out + i * slot);
        }
    };
    {
        std::vector<std::thread> th;
        const int nt = bgzf_threads(n_threads, n_blocks);
        try { for (int k = 1; k < nt; ++k) th.emplace_back(work); } catch (...) { /* fewer threads: the others take the blocks */ }
        work();
        for (std::thread& t : th) t.join();
    }
    size_t o = 0;
    for (size_t i = 0; i < n_blocks; ++i) { if (o != i * slot) memmove(out + o, out + i * slot, size[i]); o += size[i]; }
    if (with_eof) { memcpy(out + o, BGZF_EOF, sizeof BGZF_EOF); o += sizeof BGZF_EOF; }
    *out_bytes = o;
    return out;
}

bool write_all(int fd, const uint8_t* p, size_t n)
{
    while (n) {
        const ssize_t w = write(fd, p, n);
        if (w < 0) { if (errno == EINTR) continue; return false; }
        p += w; n -= (size_t)w;
    }
    return true;
}

struct Freed { void* p; explicit Freed(void* p_ = nullptr) : p(p_) {} ~Freed() { free(p); } Freed(const Freed&) = delete; Freed& operator=(const Freed&) = delete; };
struct BatchOwner { bwamem_batch_t* b; ~BatchOwner() { bwamem_hip_batch_free(b); } };

}  // namespace

// the contig names and lengths of an open index (pipeline.cpp)
const std::vector<ContigInfo>& bwamem_index_contigs(const bwaidx_t* idx);
// the QC accumulator's two-step add and its contig table (pipeline.cpp)
extern "C" {
int bwamem_qc_batch_block(bwamem_qc_t* q, bwamem_batch_t* b, uint64_t** blk);
void bwamem_qc_commit(bwamem_qc_t* q, const uint64_t* blk);
const char* bwamem_qc_contig(const bwamem_qc_t* q, int i, int64_t* len);
// the same two steps of the base-level QC accumulator, and its index
int bwamem_baseqc_batch_block(bwamem_baseqc_t* q, bwamem_batch_t* b, uint64_t** blk);
void bwamem_baseqc_commit(bwamem_baseqc_t* q, const uint64_t* blk);
bwaidx_t* bwamem_baseqc_index(const bwamem_baseqc_t* q);
}

// A plain gzip stream (one or several concatenated members, as `gzip` writes them) inflated on the host through libz.so.1: such a
// stream has no member sizes and cannot be cut for the device (bgzf_inflate.h).  false with a message when the library is not
// there, the stream is damaged, or the text would exceed `limit` bytes.  (pipeline.cpp: bwamem_hip_batch_upload_fastq_gz)
bool bwamem_gunzip_host(const void* src, size_t n, size_t limit, std::vector<char>& out)
{
    const Zlib& z = zlib();
    out.clear();
    if (!z.inflateInit2_) { fprintf(stderr, "[bwamem_hip] gunzip: libz.so.1 could not be loaded, and a plain gzip stream is inflated on the host; recompress the file with bgzip (BGZF is inflated on the device)\n"); return false; }
    Zlib::Stream zs;
    memset(&zs, 0, sizeof zs);
    if (z.inflateInit2_(&zs, 15 + 16, "1", (int)sizeof zs) != 0) { fprintf(stderr, "[bwamem_hip] gunzip: inflateInit2 failed\n"); return false; }
    bool ok = true;
    size_t in_at = 0, have = 0;
    out.resize(std::min(limit, std::max<size_t>(4 * n, 1 << 16)) + 1);
    for (;;) {
        if (zs.avail_in == 0 && in_at < n) { const size_t c = std::min<size_t>(n - in_at, 1u << 30); zs.next_in = (const unsigned char*)src + in_at; zs.avail_in = (unsigned)c; in_at += c; }
        if (have == out.size()) {
            if (have > limit) { fprintf(stderr, "[bwamem_hip] gunzip: a call is one request under 2 GiB\n"); ok = false; break; }
            out.resize(std::min(limit + 1, out.size() * 2));
        }
        const size_t room = std::min<size_t>(out.size() - have, 1u << 30);
        zs.next_out = (unsigned char*)out.data() + have; zs.avail_out = (unsigned)room;
        const int rc = z.inflate(&zs, 0);
        have += room - zs.avail_out;
        if (rc == 1) {                                              // the end of a member: another may follow
            if (zs.avail_in == 0 && in_at == n) break;
            if (z.inflateReset(&zs) != 0) { ok = false; break; }
        } else if (rc != 0 && !(rc == -5 && zs.avail_out == 0)) {    // (Z_BUF_ERROR with no room left only asks for more room)
            fprintf(stderr, "[bwamem_hip] gunzip: not a valid gzip stream (%s)\n", zs.msg ? zs.msg : rc == -5 ? "truncated" : "error");
            ok = false; break;
        }
    }
    z.inflateEnd(&zs);
    if (ok && have > limit) { fprintf(stderr, "[bwamem_hip] gunzip: a call is one request under 2 GiB\n"); ok = false; }
    if (ok) out.resize(have); else out.clear();
    return ok;
}

extern "C" {

char* bwamem_hip_sam_header(bwaidx_t* idx, size_t* pBytes)
{
    if (pBytes) *pBytes = 0;
    if (!idx) return 0;
    try {
        Out o;
        o.put("@HD\tVN:1.6\tSO:unsorted\tGO:query\n");
        for (const ContigInfo& c : bwamem_index_contigs(idx)) { o.put("@SQ\tSN:"); o.put(c.name); o.put("\tLN:"); o.num(c.len); o.ch('\n'); }
        o.put("@PG\tID:bwamem-hip\tPN:bwamem-hip\tVN:"); o.put(jnibwa_getVersion()); o.ch('\n');
        char* r = (char*)malloc(o.s.size() + 1);
        if (!r) return 0;
        memcpy(r, o.s.data(), o.s.size() + 1);
        if (pBytes) *pBytes = o.s.size();
        return r;
    } catch (...) { return 0; }
}

}  // extern "C"

namespace {

// What SA / MC / MQ need of one read (the rule at the top of bam_encode.h), taken from the response by a walk of its own: the SA
// entry of every record ("" for records that are unmapped or secondary), and record 0 as the mate sees it.
struct ReadTags { std::vector<std::string> sa; bool mapped0 = false; int mapq0 = 0; std::string cigar0; };

bool response_tags(const uint8_t* p, const uint8_t* end, uint32_t n_reads, int paired, const std::vector<ContigInfo>& contigs, std::vector<ReadTags>& out)
{
    static const char OPS[] = "MIDNSHP=X";
    out.assign(n_reads, ReadTags());
    for (uint32_t r = 0; r < n_reads; ++r) {
        if (paired && (n_reads & 1u) && r == n_reads - 1) continue;
        if (p + 4 > end) return false;
        const int32_t n_aln = rd32(p);
        for (int32_t k = 0; k < n_aln; ++k) {
            if (p + 4 > end) return false;
            const int32_t fm = rd32(p);
            const int flag = (fm >> 16) & 0xffff;
            std::string entry;
            if (!(flag & 4)) {
                if (p + 24 > end) return false;
                const int32_t rid = rd32(p), pos = rd32(p), nm = rd32(p);
                p += 8;
                const int32_t n_cig = rd32(p);
                if (rid < 0 || rid >= (int32_t)contigs.size() || n_cig < 0 || p + 4 * (size_t)n_cig + 4 > end) return false;
                std::string cigar;
                for (int32_t c = 0; c < n_cig; ++c) { const uint32_t v = (uint32_t)rd32(p); cigar += std::to_string(v >> 4); cigar += (v & 0xf) < 9 ? OPS[v & 0xf] : '?'; }
                if (cigar.empty()) cigar = "*";
                for (int s = 0; s < 2; ++s) {                           // MD, XA
                    if (p + 4 > end) return false;
                    const int32_t l = rd32(p);
                    if (l < 0 || p + ((l + 3) & ~3) > end) return false;
                    p += (l + 3) & ~3;
                }
                if (!(flag & 0x100))
                    entry = contigs[rid].name + "," + std::to_string((long long)pos + 1) + "," + (flag & 0x10 ? "-" : "+") + "," + cigar + "," + std::to_string(fm & 0xff) + "," + std::to_string(nm) + ";";
                if (k == 0) { out[r].mapped0 = true; out[r].mapq0 = fm & 0xff; out[r].cigar0 = cigar; }
            }
            if ((flag & 9) == 1) { if (p + 12 > end) return false; p += 12; }
            out[r].sa.push_back(entry);
        }
    }
    return true;
}

}  // namespace

extern "C" {

// quals: the reads' Phred+33 strings back to back, NUL-terminated like the request's reads, or null; rg_id: a read group's ID, or null;
// tags: BAM_TAG_* (SA / MC / MQ after XA)
static char* response_to_sam(bwaidx_t* idx, const char* pSeq, const void* response, size_t responseBytes, const char* const* readNames, int paired,
                             const char* quals, const char* rg_id, size_t* pBytes, unsigned tags = 0)
{
    if (pBytes) *pBytes = 0;
    if (!idx || !pSeq || !response) return 0;
    try {
        const std::vector<ContigInfo>& contigs = bwamem_index_contigs(idx);
        uint32_t n_reads; memcpy(&n_reads, pSeq, 4);
        const char* q = pSeq + 4;
        const char* ql = quals;
        const uint8_t* p = (const uint8_t*)response;
        const uint8_t* const end = p + responseBytes;
        Out o;
        o.s.reserve(responseBytes * 4 + (size_t)n_reads * 64);
        static const char OPS[] = "MIDNSHP=X";
        if (tags & ~(unsigned)BAM_TAG_ALL) return 0;
        if (!paired) tags &= BAM_TAG_SA;
        std::vector<ReadTags> rt;
        if (tags && !response_tags(p, end, n_reads, paired, contigs, rt)) return 0;
        for (uint32_t r = 0; r < n_reads; ++r) {
            const size_t l_seq = strlen(q);
            const char* seq = q;
            q += l_seq + 1;
            const char* qual = ql;
            if (ql) { if (strlen(ql) != l_seq) return 0; ql += l_seq + 1; }
            std::string name;
            if (readNames && readNames[r]) name = readNames[r];
            else { char b[32]; snprintf(b, sizeof b, paired ? "p%u" : "r%u", paired ? r >> 1 : r); name = b; }
            if (paired && (n_reads & 1u) && r == n_reads - 1) continue;      // an odd last read of a paired call produces no bytes (jnibwa.c:214: n >> 1 pairs)
            if (p + 4 > end) return 0;
            const int32_t n_aln = rd32(p);
            for (int32_t k = 0; k < n_aln; ++k) {
                if (p + 4 > end) return 0;
                const int32_t fm = rd32(p);
                const int flag = (fm >> 16) & 0xffff, mapq = fm & 0xff;
                int32_t rid = -1, pos = -1, nm = 0, as = 0, xs = 0, n_cig = 0;
                std::vector<uint32_t> cig;
                std::string md, xa;
                if (!(flag & 4)) {
                    if (p + 24 > end) return 0;
                    rid = rd32(p); pos = rd32(p); nm = rd32(p); as = rd32(p); xs = rd32(p); n_cig = rd32(p);
                    if (n_cig < 0 || p + 4 * (size_t)n_cig + 4 > end) return 0;
                    cig.resize((size_t)n_cig);
                    for (int32_t c = 0; c < n_cig; ++c) cig[c] = (uint32_t)rd32(p);
                    const int32_t n_md = rd32(p);
                    if (n_md < 0 || p + ((n_md + 3) & ~3) + 4 > end) return 0;
                    md.assign((const char*)p, (size_t)n_md); p += (n_md + 3) & ~3;
                    const int32_t n_xa = rd32(p);
                    if (n_xa < 0 || p + ((n_xa + 3) & ~3) > end) return 0;
                    xa.assign((const char*)p, (size_t)n_xa); p += (n_xa + 3) & ~3;
                }
                int32_t mrid = -1, mpos = -1, tlen = 0;
                const bool has_mate = (flag & 9) == 1;
                if (has_mate) { if (p + 12 > end) return 0; mrid = rd32(p); mpos = rd32(p); tlen = rd32(p); }
                if (rid >= (int32_t)contigs.size() || mrid >= (int32_t)contigs.size()) return 0;
                // ---- the line
                const bool hard = k > 0 && !(flag & 4);             // later records of a read: clipped bases are not repeated
                o.put(name); o.ch('\t'); o.num(flag); o.ch('\t');
                if (rid >= 0) { o.put(contigs[rid].name); o.ch('\t'); o.num((long long)pos + 1); }
                else if (has_mate && mrid >= 0) { o.put(contigs[mrid].name); o.ch('\t'); o.num((long long)mpos + 1); }     // an unmapped mate sits at its mate's place
                else o.put("*\t0");
                o.ch('\t'); o.num(mapq); o.ch('\t');
                int clip5 = 0, clip3 = 0;
                if (cig.empty()) o.ch('*');
                else {
                    for (size_t c = 0; c < cig.size(); ++c) {
                        int op = (int)(cig[c] & 0xf); const uint32_t len = cig[c] >> 4;
                        if (op == 4 || op == 5) { if (c == 0) clip5 = (int)len; else clip3 = (int)len; if (hard) op = 5; }
                        o.num(len); o.ch(op < 9 ? OPS[op] : '?');
                    }
                }
                o.ch('\t');
                if (has_mate && mrid >= 0) { if (mrid == rid || rid < 0) o.ch('='); else o.put(contigs[mrid].name); o.ch('\t'); o.num((long long)mpos + 1); }
                else if (has_mate && rid >= 0) { o.put("=\t"); o.num((long long)pos + 1); }                                 // the mate is unmapped: it sits here
                else o.put("*\t0");
                o.ch('\t'); o.num(has_mate && rid >= 0 && mrid >= 0 ? tlen : 0); o.ch('\t');
                // SEQ: as sequenced, or its reverse complement; the clips are in alignment (reference-strand) order
                size_t b = 0, e = l_seq;
                if (hard) { b = (size_t)clip5; e = l_seq - (size_t)clip3; if (b > e) { b = 0; e = l_seq; } }
                if (l_seq == 0) o.ch('*');
                else if (flag & 0x10) { for (size_t i = b; i < e; ++i) o.ch(comp(seq[l_seq - 1 - i])); }
                else o.s.append(seq + b, e - b);
                o.ch('\t');
                if (!qual || e == b) o.ch('*');
                else if (flag & 0x10) { for (size_t i = b; i < e; ++i) o.ch(qual[l_seq - 1 - i]); }
                else o.s.append(qual + b, e - b);
                if (!(flag & 4)) {
                    o.put("\tNM:i:"); o.num(nm);
                    if (!md.empty()) { o.put("\tMD:Z:"); o.put(md); }
                    o.put("\tAS:i:"); o.num(as);
                    if (xs >= 0) { o.put("\tXS:i:"); o.num(xs); }
                    if (!xa.empty()) { o.put("\tXA:Z:"); o.put(xa); }
                }
                if ((tags & BAM_TAG_SA) && !rt[r].sa[(size_t)k].empty()) {
                    std::string others;
                    for (size_t j = 0; j < rt[r].sa.size(); ++j) if (j != (size_t)k) others += rt[r].sa[j];
                    if (!others.empty()) { o.put("\tSA:Z:"); o.put(others); }
                }
                if ((tags & (BAM_TAG_MC | BAM_TAG_MQ)) && (r ^ 1u) < n_reads && rt[r ^ 1u].mapped0) {
                    if (tags & BAM_TAG_MC) { o.put("\tMC:Z:"); o.put(rt[r ^ 1u].cigar0); }
                    if (tags & BAM_TAG_MQ) { o.put("\tMQ:i:"); o.num(rt[r ^ 1u].mapq0); }
                }
                if (rg_id) { o.put("\tRG:Z:"); o.put(rg_id); }
                o.ch('\n');
            }
        }
        if (p != end) return 0;
        char* res = (char*)malloc(o.s.size() + 1);
        if (!res) return 0;
        memcpy(res, o.s.data(), o.s.size() + 1);
        if (pBytes) *pBytes = o.s.size();
        return res;
    } catch (...) { return 0; }
}

char* bwamem_hip_response_to_sam(bwaidx_t* idx, const char* pSeq, const void* response, size_t responseBytes, const char* const* readNames, int paired, size_t* pBytes)
{
    return response_to_sam(idx, pSeq, response, responseBytes, readNames, paired, nullptr, nullptr, pBytes);
}

char* bwamem_hip_response_to_sam_q(bwaidx_t* idx, const char* pSeq, const void* response, size_t responseBytes, const char* const* readNames, int paired,
                                   const char* quals, const char* rgId, size_t* pBytes)
{
    return response_to_sam(idx, pSeq, response, responseBytes, readNames, paired, quals, rgId, pBytes);
}

char* bwamem_hip_response_to_sam_tags(bwaidx_t* idx, const char* pSeq, const void* response, size_t responseBytes, const char* const* readNames, int paired,
                                      const char* quals, const char* rgId, unsigned tags, size_t* pBytes)
{
    return response_to_sam(idx, pSeq, response, responseBytes, readNames, paired, quals, rgId, pBytes, tags);
}

// header text with the read group's line after the last @SQ line; false: the line is refused
static bool header_text_rg(const char* text, size_t l_text, const char* rg_line, std::string& out)
{
    const char* id = nullptr;
    if (bam_rg_id(rg_line, &id) <= 0) { fprintf(stderr, "[bwamem_hip] header: not one \"@RG\\t\" line with an ID: field of 1..254 bytes\n"); return false; }
    size_t at = 0, after_sq = 0;
    while (at < l_text) {
        const char* eol = (const char*)memchr(text + at, '\n', l_text - at);
        const size_t next = eol ? (size_t)(eol - text) + 1 : l_text;
        if (next - at >= 3 && !memcmp(text + at, "@SQ", 3)) after_sq = next;
        at = next;
    }
    out.assign(text, after_sq); out += rg_line; out += '\n'; out.append(text + after_sq, l_text - after_sq);
    return true;
}

char* bwamem_hip_sam_header_rg(bwaidx_t* idx, const char* rg_line, size_t* pBytes)
{
    if (pBytes) *pBytes = 0;
    try {
        size_t l_text = 0;
        Freed text(bwamem_hip_sam_header(idx, &l_text));
        if (!text.p) return 0;
        std::string o;
        if (!rg_line) o.assign((const char*)text.p, l_text);
        else if (!header_text_rg((const char*)text.p, l_text, rg_line, o)) return 0;
        char* r = (char*)malloc(o.size() + 1);
        if (!r) return 0;
        memcpy(r, o.c_str(), o.size() + 1);
        if (pBytes) *pBytes = o.size();
        return r;
    } catch (...) { return 0; }
}

// ---- BAM
void* bwamem_hip_bam_header(bwaidx_t* idx, size_t* pBytes)
{
    if (pBytes) *pBytes = 0;
    if (!idx) return 0;
    try {
        size_t l_text = 0;
        Freed text(bwamem_hip_sam_header(idx, &l_text));
        if (!text.p || l_text > 0x7fffffff) return 0;
        const std::vector<ContigInfo>& contigs = bwamem_index_contigs(idx);
        std::string o("BAM\1", 4);
        auto put32 = [&](int32_t v) { uint8_t b[4]; le32(b, (uint32_t)v); o.append((const char*)b, 4); };
        put32((int32_t)l_text); o.append((const char*)text.p, l_text);
        put32((int32_t)contigs.size());
        for (const ContigInfo& c : contigs) {
            if (c.len > 0x7fffffff) return 0;
            put32((int32_t)c.name.size() + 1); o.append(c.name.c_str(), c.name.size() + 1); put32((int32_t)c.len);
        }
        void* r = malloc(o.size() ? o.size() : 1);
        if (!r) return 0;
        memcpy(r, o.data(), o.size());
        if (pBytes) *pBytes = o.size();
        return r;
    } catch (...) { return 0; }
}

void* bwamem_hip_bgzf_compress(const void* src, size_t n, int level, int n_threads, int with_eof, size_t* pBytes)
{
    size_t bytes = 0;
    void* r = 0;
    try { r = bgzf_compress((const uint8_t*)src, n, level, n_threads, with_eof != 0, &bytes); } catch (...) { r = 0; }
    if (pBytes) *pBytes = r ? bytes : 0;
    return r;
}

int64_t bwamem_hip_bam_record_bytes(const void* rec, size_t n_words, int k, int32_t l_read, int32_t l_name)
{
    try {
        if (!rec || l_read < 0 || l_name < 1 || l_name > 254) return -BAM_ERR_PARSE;
        BamRec R;
        const int err = bam_parse((const uint32_t*)rec, (int64_t)n_words, k, l_read, 0x7fffffff, R);
        if (err) return -err;
        R.name = 0; R.name_letter = 0; R.name_idx = 0; R.l_name = l_name;
        const int32_t t = bam_layout(R);
        return t < 0 ? -BAM_ERR_SPAN : t;
    } catch (...) { return -BAM_ERR_PARSE; }
}

int bwamem_hip_align_to_bam(bwaidx_t* idx, const mem_opt_t* opt, const mem_pestat_t* pes, const char* pSeq, size_t nBytes, const char* const* readNames,
                            int level, int fd, int write_header)
{
    try {
        if (!idx || !opt || !pSeq || nBytes < 4 || fd < 0 || level < 0 || level > 9) return -1;
        if (level > 0 && !zlib().compress2) { fprintf(stderr, "[bwamem_hip] align_to_bam: libz.so.1 could not be loaded; only level 0 is available\n"); return -1; }
        uint32_t n_reads; memcpy(&n_reads, pSeq, 4);
        int32_t flag; memcpy(&flag, (const char*)opt + 60, 4);                  // mem_opt_t.flag (BwaMemAligner.java:75)
        const int paired = (flag & 0x2) != 0;
        std::string blob; std::vector<int64_t> name_off;
        if (readNames) {
            name_off.reserve((size_t)n_reads + 1);
            for (uint32_t i = 0; i < n_reads; ++i) { name_off.push_back((int64_t)blob.size()); if (readNames[i]) blob += readNames[i]; }
            name_off.push_back((int64_t)blob.size());
        }
        BatchOwner bo{ bwamem_hip_batch_upload(idx, pSeq, nBytes) };
        if (!bo.b) return -1;
        if (bwamem_hip_batch_keep_offsets(bo.b, 1) != 0 || bwamem_hip_batch_align(idx, opt, pes, bo.b, 0) != 0) return -1;
        if (bwamem_hip_batch_encode_bam(bo.b, paired, readNames ? blob.data() : nullptr, readNames ? name_off.data() : nullptr) != 0) return -1;
        const size_t n = bwamem_hip_batch_bam_bytes(bo.b);
        Freed recs(malloc(n ? n : 1));
        if (!recs.p || bwamem_hip_batch_bam_download(bo.b, recs.p) != 0) return -1;
        if (write_header) {
            size_t nh = 0, nz = 0;
            Freed hdr(bwamem_hip_bam_header(idx, &nh));
            if (!hdr.p) return -1;
            Freed z(bgzf_compress((const uint8_t*)hdr.p, nh, level, 0, false, &nz));
            if (!z.p || !write_all(fd, (const uint8_t*)z.p, nz)) return -1;
        }
        size_t nz = 0;
        Freed z(bgzf_compress((const uint8_t*)recs.p, n, level, 0, true, &nz));
        if (!z.p || !write_all(fd, (const uint8_t*)z.p, nz)) return -1;
        return 0;
    } catch (...) { return -1; }
}

// bwamem_hip_align_to_bam with the BGZF members made on the device: only compressed bytes are downloaded, and libz is not touched
int bwamem_hip_align_to_bam_device(bwaidx_t* idx, const mem_opt_t* opt, const mem_pestat_t* pes, const char* pSeq, size_t nBytes, const char* const* readNames,
                                   int fd, int write_header)
{
    try {
        if (!idx || !opt || !pSeq || nBytes < 4 || fd < 0) return -1;
        uint32_t n_reads; memcpy(&n_reads, pSeq, 4);
        int32_t flag; memcpy(&flag, (const char*)opt + 60, 4);                  // mem_opt_t.flag (BwaMemAligner.java:75)
        const int paired = (flag & 0x2) != 0;
        std::string blob; std::vector<int64_t> name_off;
        if (readNames) {
            name_off.reserve((size_t)n_reads + 1);
            for (uint32_t i = 0; i < n_reads; ++i) { name_off.push_back((int64_t)blob.size()); if (readNames[i]) blob += readNames[i]; }
            name_off.push_back((int64_t)blob.size());
        }
        BatchOwner bo{ bwamem_hip_batch_upload(idx, pSeq, nBytes) };
        if (!bo.b) return -1;
        if (bwamem_hip_batch_keep_offsets(bo.b, 1) != 0 || bwamem_hip_batch_align(idx, opt, pes, bo.b, 0) != 0) return -1;
        if (bwamem_hip_batch_encode_bam(bo.b, paired, readNames ? blob.data() : nullptr, readNames ? name_off.data() : nullptr) != 0) return -1;
        if (write_header) {
            size_t nh = 0, nz = 0;
            Freed hdr(bwamem_hip_bam_header(idx, &nh));
            if (!hdr.p) return -1;
            Freed z(bwamem_hip_bgzf_compress_device(idx, hdr.p, nh, 0, &nz));
            if (!z.p || !write_all(fd, (const uint8_t*)z.p, nz)) return -1;
        }
        if (bwamem_hip_batch_bam_bytes(bo.b) == 0) return write_all(fd, BGZF_EOF, sizeof BGZF_EOF) ? 0 : -1;      // no record: the EOF block alone
        if (bwamem_hip_batch_compress_bam(bo.b, 1) != 0) return -1;
        const size_t nz = bwamem_hip_batch_bgzf_bytes(bo.b);
        Freed z(malloc(nz ? nz : 1));
        if (!z.p || bwamem_hip_batch_bgzf_download(bo.b, z.p) != 0 || !write_all(fd, (const uint8_t*)z.p, nz)) return -1;
        return 0;
    } catch (...) { return -1; }
}

// bwamem_hip_bam_header with the @HD line of a coordinate-sorted file
void* bwamem_hip_bam_header_sorted(bwaidx_t* idx, size_t* pBytes)
{
    if (pBytes) *pBytes = 0;
    try {
        size_t n = 0;
        Freed hdr(bwamem_hip_bam_header(idx, &n));
        if (!hdr.p || n < 8) return 0;
        const uint8_t* h = (const uint8_t*)hdr.p;
        const size_t l_text = (size_t)h[4] | (size_t)h[5] << 8 | (size_t)h[6] << 16 | (size_t)h[7] << 24;
        const void* eol = l_text <= n - 8 ? memchr(h + 8, '\n', l_text) : 0;
        if (!eol) return 0;
        std::string text("@HD\tVN:1.6\tSO:coordinate");
        text.append((const char*)eol, (const char*)h + 8 + l_text);
        std::string o("BAM\1", 4);
        uint8_t b[4]; le32(b, (uint32_t)text.size());
        o.append((const char*)b, 4); o += text; o.append((const char*)h + 8 + l_text, n - 8 - l_text);
        void* r = malloc(o.size());
        if (!r) return 0;
        memcpy(r, o.data(), o.size());
        if (pBytes) *pBytes = o.size();
        return r;
    } catch (...) { return 0; }
}

// bwamem_hip_bam_header / _sorted with the read group's line after the last @SQ line (rg_line == null: the header as it is)
void* bwamem_hip_bam_header_rg(bwaidx_t* idx, int sorted, const char* rg_line, size_t* pBytes)
{
    if (pBytes) *pBytes = 0;
    try {
        size_t n = 0;
        Freed hdr(sorted ? bwamem_hip_bam_header_sorted(idx, &n) : bwamem_hip_bam_header(idx, &n));
        if (!hdr.p || n < 8) return 0;
        const uint8_t* h = (const uint8_t*)hdr.p;
        const size_t l_text = (size_t)h[4] | (size_t)h[5] << 8 | (size_t)h[6] << 16 | (size_t)h[7] << 24;
        if (l_text > n - 8) return 0;
        std::string text;
        if (!rg_line) text.assign((const char*)h + 8, l_text);
        else if (!header_text_rg((const char*)h + 8, l_text, rg_line, text)) return 0;
        if (text.size() > 0x7fffffff) return 0;
        std::string o("BAM\1", 4);
        uint8_t b[4]; le32(b, (uint32_t)text.size());
        o.append((const char*)b, 4); o += text; o.append((const char*)h + 8 + l_text, n - 8 - l_text);
        void* r = malloc(o.size());
        if (!r) return 0;
        memcpy(r, o.data(), o.size());
        if (pBytes) *pBytes = o.size();
        return r;
    } catch (...) { return 0; }
}

}  // extern "C"

namespace {

// An aligned batch to a file, everything on the device: encode (names: the caller's, or null), mark duplicates if asked (counts: the
// totals, or null), sort if asked, compress, index if asked (fd_bai >= 0), write.  The header carries rg_line when there is one.
// Everything is made before the first byte is written.
int batch_to_bam_file(bwaidx_t* idx, bwamem_batch_t* b, int paired, const char* names, const int64_t* name_off, const char* rg_line, int mark_dup,
                      bwamem_dup_counts_t* counts, int sort, int fd, int fd_bai, int write_header, unsigned tags = 0, bwamem_qc_t* qc = nullptr,
                      bwamem_baseqc_t* bq = nullptr)
{
    if (tags && bwamem_hip_batch_set_tags(b, tags) != 0) return -1;
    if (bwamem_hip_batch_encode_bam(b, paired, names, name_off) != 0) return -1;
    if (mark_dup && bwamem_hip_batch_mark_duplicates(b, paired, counts) != 0) return -1;
    uint64_t* qc_words_ = nullptr;                                      // the batch's QC block: reduced here, added when everything is written
    if (qc && bwamem_qc_batch_block(qc, b, &qc_words_) != 0) return -1;
    Freed qc_blk(qc_words_);
    uint64_t* bq_words_ = nullptr;                                      // ... and its base-level QC block
    if (bq && bwamem_baseqc_batch_block(bq, b, &bq_words_) != 0) return -1;
    Freed bq_blk(bq_words_);
    if (sort && bwamem_hip_batch_sort_bam(b) != 0) return -1;
    size_t nh = 0, nzh = 0, nz = 0, nb = 0;
    Freed zh, z, bai;
    if (write_header) {
        Freed hdr(bwamem_hip_bam_header_rg(idx, sort, rg_line, &nh));
        if (!hdr.p) return -1;
        zh.p = bwamem_hip_bgzf_compress_device(idx, hdr.p, nh, 0, &nzh);
        if (!zh.p) return -1;
    }
    if (bwamem_hip_batch_bam_bytes(b) != 0) {
        if (bwamem_hip_batch_compress_bam(b, 1) != 0) return -1;
        nz = bwamem_hip_batch_bgzf_bytes(b);
        z.p = malloc(nz ? nz : 1);
        if (!z.p || bwamem_hip_batch_bgzf_download(b, z.p) != 0) return -1;
    }
    if (fd_bai >= 0) {
        bai.p = bwamem_hip_batch_index_bam(b, (int64_t)nzh, &nb);
        if (!bai.p) return -1;
    }
    if (write_header && !write_all(fd, (const uint8_t*)zh.p, nzh)) return -1;
    if (z.p ? !write_all(fd, (const uint8_t*)z.p, nz) : !write_all(fd, BGZF_EOF, sizeof BGZF_EOF)) return -1;      // no record: the EOF block alone
    if (fd_bai >= 0 && !write_all(fd_bai, (const uint8_t*)bai.p, nb)) return -1;
    if (qc) bwamem_qc_commit(qc, (const uint64_t*)qc_blk.p);
    if (bq) bwamem_baseqc_commit(bq, (const uint64_t*)bq_blk.p);
    return 0;
}

// the request calls that go through batch_to_bam_file
int request_to_bam_file(const char* what, bwaidx_t* idx, const mem_opt_t* opt, const mem_pestat_t* pes, const char* pSeq, size_t nBytes, const char* const* readNames,
                        int mark_dup, bwamem_dup_counts_t* counts, int sort, int fd, int fd_bai, int write_header)
{
    try {
        if (!idx || !opt || !pSeq || nBytes < 4 || fd < 0) return -1;
        if (fd_bai >= 0 && !(sort && write_header)) { fprintf(stderr, "[bwamem_hip] %s: an index needs %sthe header in the same file\n", what, sort ? "" : "a sorted file with "); return -1; }
        uint32_t n_reads; memcpy(&n_reads, pSeq, 4);
        int32_t flag; memcpy(&flag, (const char*)opt + 60, 4);                  // mem_opt_t.flag (BwaMemAligner.java:75)
        const int paired = (flag & 0x2) != 0;
        std::string blob; std::vector<int64_t> name_off;
        if (readNames) {
            name_off.reserve((size_t)n_reads + 1);
            for (uint32_t i = 0; i < n_reads; ++i) { name_off.push_back((int64_t)blob.size()); if (readNames[i]) blob += readNames[i]; }
            name_off.push_back((int64_t)blob.size());
        }
        BatchOwner bo{ bwamem_hip_batch_upload(idx, pSeq, nBytes) };
        if (!bo.b) return -1;
        if (bwamem_hip_batch_keep_offsets(bo.b, 1) != 0 || bwamem_hip_batch_align(idx, opt, pes, bo.b, 0) != 0) return -1;
        return batch_to_bam_file(idx, bo.b, paired, readNames ? blob.data() : nullptr, readNames ? name_off.data() : nullptr, nullptr, mark_dup, counts, sort, fd, fd_bai,
                                 write_header);
    } catch (...) { return -1; }
}

int fastq_to_bam_file(const char* what, bwaidx_t* idx, const mem_opt_t* opt, const mem_pestat_t* pes, const char* text1, size_t n1, const char* text2, size_t n2,
                      const char* rg_line, int mark_dup, bwamem_dup_counts_t* counts, int sort, int fd, int fd_bai, int write_header, bool gz = false, unsigned tags = 0,
                      bwamem_qc_t* qc = nullptr, bwamem_baseqc_t* bq = nullptr)
{
    try {
        if (!idx || !opt || fd < 0) return -1;
        if (fd_bai >= 0 && !(sort && write_header)) { fprintf(stderr, "[bwamem_hip] %s: an index needs a sorted file with its header\n", what); return -1; }
        int32_t flag; memcpy(&flag, (const char*)opt + 60, 4);                  // mem_opt_t.flag (BwaMemAligner.java:75)
        const int paired = (flag & 0x2) != 0;
        int64_t bad = -1;
        int64_t bad_member = -1;
        BatchOwner bo{ gz ? bwamem_hip_batch_upload_fastq_gz(idx, text1, n1, text2, n2, &bad, &bad_member) : bwamem_hip_batch_upload_fastq(idx, text1, n1, text2, n2, &bad) };
        if (!bo.b) return -1;
        if (rg_line && bwamem_hip_batch_set_read_group(bo.b, rg_line) != 0) return -1;
        if (bwamem_hip_batch_keep_offsets(bo.b, 1) != 0 || bwamem_hip_batch_align(idx, opt, pes, bo.b, 0) != 0) return -1;
        return batch_to_bam_file(idx, bo.b, paired, nullptr, nullptr, rg_line, mark_dup, counts, sort, fd, fd_bai, write_header, tags, qc, bq);
    } catch (...) { return -1; }
}

}  // namespace

extern "C" {

// bwamem_hip_align_to_bam_device with the records coordinate-sorted on the device, and the BAI index into fd_bai when asked for
int bwamem_hip_align_to_sorted_bam(bwaidx_t* idx, const mem_opt_t* opt, const mem_pestat_t* pes, const char* pSeq, size_t nBytes, const char* const* readNames,
                                   int fd, int fd_bai, int write_header)
{
    return request_to_bam_file("align_to_sorted_bam", idx, opt, pes, pSeq, nBytes, readNames, 0, nullptr, 1, fd, fd_bai, write_header);
}

// ... with the duplicates marked on the device between encode and sort (bam_dup.h); sort == 0: response order and the plain header
int bwamem_hip_align_to_marked_bam(bwaidx_t* idx, const mem_opt_t* opt, const mem_pestat_t* pes, const char* pSeq, size_t nBytes, const char* const* readNames,
                                   int sort, int fd, int fd_bai, int write_header, bwamem_dup_counts_t* counts)
{
    if (counts) memset(counts, 0, sizeof *counts);
    return request_to_bam_file("align_to_marked_bam", idx, opt, pes, pSeq, nBytes, readNames, 1, counts, sort != 0, fd, fd_bai, write_header);
}

// FASTQ text in, a BAM file out: the text is taken apart on the device (fastq_parse.h), so the records carry the reads' own names and
// base qualities, and RG:Z when rg_line names a read group
int bwamem_hip_align_fastq_to_bam(bwaidx_t* idx, const mem_opt_t* opt, const mem_pestat_t* pes, const char* text1, size_t n1, const char* text2, size_t n2,
                                  const char* rg_line, int sort, int fd, int fd_bai, int write_header)
{
    return fastq_to_bam_file("align_fastq_to_bam", idx, opt, pes, text1, n1, text2, n2, rg_line, 0, nullptr, sort, fd, fd_bai, write_header);
}

// ... with the duplicates marked on the device between encode and sort (bam_dup.h)
int bwamem_hip_align_fastq_to_marked_bam(bwaidx_t* idx, const mem_opt_t* opt, const mem_pestat_t* pes, const char* text1, size_t n1, const char* text2, size_t n2,
                                         const char* rg_line, int sort, int fd, int fd_bai, int write_header, bwamem_dup_counts_t* counts)
{
    if (counts) memset(counts, 0, sizeof *counts);
    return fastq_to_bam_file("align_fastq_to_marked_bam", idx, opt, pes, text1, n1, text2, n2, rg_line, 1, counts, sort, fd, fd_bai, write_header);
}

// ... from compressed FASTQ (bgzf_inflate.h): BGZF streams are inflated on the device, plain gzip streams on the host.  mark_dup == 0
// (and counts == NULL) is bwamem_hip_align_fastq_to_bam on the inflated texts.
int bwamem_hip_align_fastq_gz_to_marked_bam(bwaidx_t* idx, const mem_opt_t* opt, const mem_pestat_t* pes, const void* gz1, size_t n1, const void* gz2, size_t n2,
                                            const char* rg_line, int sort, int fd, int fd_bai, int write_header, int mark_dup, bwamem_dup_counts_t* counts)
{
    if (counts) memset(counts, 0, sizeof *counts);
    return fastq_to_bam_file("align_fastq_gz_to_marked_bam", idx, opt, pes, (const char*)gz1, n1, (const char*)gz2, n2, rg_line, mark_dup != 0, mark_dup ? counts : nullptr,
                             sort, fd, fd_bai, write_header, true);
}

// The one-call entry point with its choices in a struct: bwamem_hip_align_fastq_gz_to_marked_bam / _fastq_to_marked_bam by the first
// two bytes of the input, plus the optional tags.  Fields beyond o->size are zero.
int bwamem_hip_fastq_to_bam(bwaidx_t* idx, const mem_opt_t* opt, const mem_pestat_t* pes, const void* in1, size_t n1, const void* in2, size_t n2,
                            const bwamem_bam_options_t* o, int fd, int fd_bai, bwamem_dup_counts_t* counts)
{
    return bwamem_hip_fastq_to_bam_qc(idx, opt, pes, in1, n1, in2, n2, o, fd, fd_bai, counts, nullptr);
}

// ... with the batch added to a QC accumulator (bam_qc.h) after the marking and before the sort, once the whole call has succeeded
int bwamem_hip_fastq_to_bam_qc(bwaidx_t* idx, const mem_opt_t* opt, const mem_pestat_t* pes, const void* in1, size_t n1, const void* in2, size_t n2,
                               const bwamem_bam_options_t* o, int fd, int fd_bai, bwamem_dup_counts_t* counts, bwamem_qc_t* qc)
{
    return bwamem_hip_fastq_to_bam_metrics(idx, opt, pes, in1, n1, in2, n2, o, fd, fd_bai, counts, qc, nullptr);
}

// ... and to a base-level QC accumulator (bam_baseqc.h) at the same point; either accumulator may be null
int bwamem_hip_fastq_to_bam_metrics(bwaidx_t* idx, const mem_opt_t* opt, const mem_pestat_t* pes, const void* in1, size_t n1, const void* in2, size_t n2,
                                    const bwamem_bam_options_t* o, int fd, int fd_bai, bwamem_dup_counts_t* counts, bwamem_qc_t* qc, bwamem_baseqc_t* bq)
{
    if (counts) memset(counts, 0, sizeof *counts);
    bwamem_bam_options_t v;
    memset(&v, 0, sizeof v);
    if (o) {
        if (o->size < sizeof(size_t) || o->size > sizeof v) { fprintf(stderr, "[bwamem_hip] fastq_to_bam: options of %zu bytes (this library knows %zu)\n", o->size, sizeof v); return -1; }
        memcpy(&v, o, o->size);
    }
    if (v.tags & ~(unsigned)BAM_TAG_ALL) { fprintf(stderr, "[bwamem_hip] fastq_to_bam: unknown tag bits 0x%x\n", v.tags & ~(unsigned)BAM_TAG_ALL); return -1; }
    auto is_gz = [](const void* p, size_t n) { return p && n >= 2 && ((const uint8_t*)p)[0] == 0x1f && ((const uint8_t*)p)[1] == 0x8b; };
    const bool gz = is_gz(in1, n1);
    if (in2 && n2 && is_gz(in2, n2) != gz) { fprintf(stderr, "[bwamem_hip] fastq_to_bam: one input is compressed and the other is not\n"); return -1; }
    return fastq_to_bam_file("fastq_to_bam", idx, opt, pes, (const char*)in1, n1, (const char*)in2, n2, v.rg_line, v.mark_dup != 0, v.mark_dup ? counts : nullptr,
                             v.sort != 0, fd, fd_bai, v.write_header, gz, v.tags, qc, bq);
}

// ---- the QC reports (bam_qc.h): plain text, '\n' line ends
//   FLAGSTAT     sixteen lines "<passed> + <failed> <label>"; mapped, primary mapped, properly paired and singletons end in
//                " (P : F)", the two columns as %.2f%% of total, primary, paired and paired, or N/A over a zero
//   IDXSTATS     name, length, mapped, unmapped per contig in index order, then "*\t0\t0\t<unplaced>"
//   SUMMARY      "key\tvalue": the single counters by their field names, then error_rate (mismatches / bases_mapped_cigar),
//                average_length, average_quality, q20_bases, q30_bases, percent_duplication (primary_duplicates / primary_mapped,
//                both columns); doubles as %.6f, N/A over a zero
//   INSERT_SIZE  a header, a line per non-empty orientation (median and MAD %.1f, mean and standard deviation %.6f), an empty line,
//                "insert_size\tFR\tRF\tTANDEM" and a line per bin that is non-zero in any orientation
char* bwamem_hip_qc_report(const bwamem_qc_t* q, int kind, size_t* pBytes)
{
    if (pBytes) *pBytes = 0;
    try {
        bwamem_qc_counts_t c;
        if (!q || bwamem_hip_qc_counts(q, &c) != 0) return nullptr;
        std::string o;
        char buf[512];
        auto ratio = [&](uint64_t a, uint64_t b, const char* fmt, double scale) -> std::string {
            if (!b) return "N/A";
            char t[64]; snprintf(t, sizeof t, fmt, scale * (double)a / (double)b); return t;
        };
        auto array = [&](int which) { std::vector<uint64_t> a((size_t)std::max<int64_t>(bwamem_hip_qc_array(q, which, nullptr, 0), 0)); bwamem_hip_qc_array(q, which, a.data(), a.size()); return a; };
        if (kind == BWAMEM_HIP_QC_FLAGSTAT) {
            static const char* const label[16] = { "in total (QC-passed reads + QC-failed reads)", "primary", "secondary", "supplementary", "duplicates", "primary duplicates",
                "mapped", "primary mapped", "paired in sequencing", "read1", "read2", "properly paired", "with itself and mate mapped", "singletons",
                "with mate mapped to a different chr", "with mate mapped to a different chr (mapQ>=5)" };
            const uint64_t (*row)[2] = &c.total;                        // the sixteen pairs are laid out in the order of the lines
            for (int k = 0; k < 16; ++k) {
                snprintf(buf, sizeof buf, "%llu + %llu %s", (unsigned long long)row[k][0], (unsigned long long)row[k][1], label[k]);
                o += buf;
                const uint64_t* den = k == 6 ? c.total : k == 7 ? c.primary : k == 11 || k == 13 ? c.paired : nullptr;
                if (den) o += " (" + ratio(row[k][0], den[0], "%.2f%%", 100.0) + " : " + ratio(row[k][1], den[1], "%.2f%%", 100.0) + ")";
                o += "\n";
            }
        } else if (kind == BWAMEM_HIP_QC_IDXSTATS) {
            const std::vector<uint64_t> m = array(BWAMEM_HIP_QC_CONTIG_MAPPED), u = array(BWAMEM_HIP_QC_CONTIG_UNMAPPED);
            for (size_t i = 0; i < m.size(); ++i) {
                int64_t len = 0;
                const char* name = bwamem_qc_contig(q, (int)i, &len);
                o += name ? name : "";
                snprintf(buf, sizeof buf, "\t%lld\t%llu\t%llu\n", (long long)len, (unsigned long long)m[i], (unsigned long long)u[i]);
                o += buf;
            }
            snprintf(buf, sizeof buf, "*\t0\t0\t%llu\n", (unsigned long long)c.unplaced);
            o += buf;
        } else if (kind == BWAMEM_HIP_QC_SUMMARY) {
            static const char* const key[14] = { "unplaced", "sequences", "total_length", "max_length", "reads_mq0", "bases_mapped", "bases_mapped_cigar", "bases_soft_clipped",
                "ins_events", "ins_bases", "del_events", "del_bases", "mismatches", "records_without_nm" };
            const uint64_t* val = &c.unplaced;
            for (int k = 0; k < 14; ++k) { snprintf(buf, sizeof buf, "%s\t%llu\n", key[k], (unsigned long long)val[k]); o += buf; }
            const std::vector<uint64_t> qh = array(BWAMEM_HIP_QC_QUAL);
            uint64_t nq = 0, sq = 0, q20 = 0, q30 = 0;
            for (size_t v = 0; v < qh.size(); ++v) { nq += qh[v]; sq += qh[v] * v; if (v >= 20) q20 += qh[v]; if (v >= 30) q30 += qh[v]; }
            o += "error_rate\t" + ratio(c.mismatches, c.bases_mapped_cigar, "%.6f", 1.0) + "\n";
            o += "average_length\t" + ratio(c.total_length, c.sequences, "%.6f", 1.0) + "\n";
            o += "average_quality\t" + ratio(sq, nq, "%.6f", 1.0) + "\n";
            snprintf(buf, sizeof buf, "q20_bases\t%llu\nq30_bases\t%llu\n", (unsigned long long)q20, (unsigned long long)q30);
            o += buf;
            o += "percent_duplication\t" + ratio(c.primary_duplicates[0] + c.primary_duplicates[1], c.primary_mapped[0] + c.primary_mapped[1], "%.6f", 1.0) + "\n";
        } else if (kind == BWAMEM_HIP_QC_INSERT_SIZE) {
            static const char* const name[3] = { "FR", "RF", "TANDEM" };
            std::vector<uint64_t> h[3];
            o += "PAIR_ORIENTATION\tREAD_PAIRS\tMIN_INSERT_SIZE\tMAX_INSERT_SIZE\tMEDIAN_INSERT_SIZE\tMEDIAN_ABSOLUTE_DEVIATION\tMEAN_INSERT_SIZE\tSTANDARD_DEVIATION\n";
            for (int k = 0; k < 3; ++k) {
                h[k] = array(BWAMEM_HIP_QC_ISIZE_FR + k);
                const QcIsizeStats s = qc_isize_stats(h[k].data());
                if (!s.n) continue;
                snprintf(buf, sizeof buf, "%s\t%llu\t%llu\t%llu\t%.1f\t%.1f\t%.6f\t%.6f\n", name[k], (unsigned long long)s.n, (unsigned long long)c.isize_min[k],
                         (unsigned long long)c.isize_max[k], s.median, s.mad, s.mean, s.sd);
                o += buf;
            }
            o += "\ninsert_size\tFR\tRF\tTANDEM\n";
            for (int v = 0; v < BAMQC_ISIZE_BINS; ++v)
                if (h[0][v] | h[1][v] | h[2][v]) {
                    snprintf(buf, sizeof buf, "%d\t%llu\t%llu\t%llu\n", v, (unsigned long long)h[0][v], (unsigned long long)h[1][v], (unsigned long long)h[2][v]);
                    o += buf;
                }
        } else return nullptr;
        char* r = (char*)malloc(o.size() + 1);
        if (!r) return nullptr;
        memcpy(r, o.c_str(), o.size() + 1);
        if (pBytes) *pBytes = o.size();
        return r;
    } catch (...) { return nullptr; }
}

// ---- the base-level QC reports (bam_baseqc.h): plain text, '\n' line ends.  Every double is a / b of two integers turned into
// doubles at the end, printed with a fixed format; over an empty denominator it is 0.
//   CYCLES   per end e with records: "# end <e> records <n>", the column names, and a row per cycle 0 .. the last one with a non-zero
//            word in any table: cycle, bases (the sum of base[]), mean_quality (qual_sum / qual_n, %.4f), the fractions of A C G T N
//            (%.6f), aligned, mismatch_rate (mism / aligned, %.6f), insertions, deletions, soft_clips
//   GC       "# gcb_skipped <n>", the column names and 101 rows: gc, windows, reads, normalized_coverage ((reads[g] / sum reads) /
//            (windows[g] / sum windows), computed as reads[g] * sum windows over sum reads * windows[g], %.6f), mean_base_quality
//            (gcb_qual_sum / gcb_qual_n, %.4f); an empty line; "gc_percent<TAB>end0<TAB>end1<TAB>end2" and the 101 rows of read_gc
char* bwamem_hip_baseqc_report(const bwamem_baseqc_t* q, int kind, size_t* pBytes)
{
    if (pBytes) *pBytes = 0;
    try {
        bwamem_baseqc_counts_t c;
        if (!q || bwamem_hip_baseqc_counts(q, &c) != 0) return nullptr;
        std::string o;
        char buf[512];
        auto array = [&](int which) { std::vector<uint64_t> a((size_t)std::max<int64_t>(bwamem_hip_baseqc_array(q, which, nullptr, 0), 0)); bwamem_hip_baseqc_array(q, which, a.data(), a.size()); return a; };
        auto ratio = [](uint64_t a, uint64_t b) { return b ? (double)a / (double)b : 0.0; };
        if (kind == BWAMEM_HIP_BASEQC_CYCLES) {
            const std::vector<uint64_t> base = array(BWAMEM_HIP_BASEQC_BASE), qs = array(BWAMEM_HIP_BASEQC_QUAL_SUM), qn = array(BWAMEM_HIP_BASEQC_QUAL_N),
                al = array(BWAMEM_HIP_BASEQC_ALIGNED), mm = array(BWAMEM_HIP_BASEQC_MISM), in = array(BWAMEM_HIP_BASEQC_INS), de = array(BWAMEM_HIP_BASEQC_DEL),
                so = array(BWAMEM_HIP_BASEQC_SOFT);
            for (int e = 0; e < BASEQC_ENDS; ++e) {
                if (!c.records[e]) continue;
                snprintf(buf, sizeof buf, "# end %d records %llu\n", e, (unsigned long long)c.records[e]);
                o += buf;
                o += "cycle\tbases\tmean_quality\tA\tC\tG\tT\tN\taligned\tmismatch_rate\tinsertions\tdeletions\tsoft_clips\n";
                int last = -1;
                for (int cy = 0; cy < BASEQC_CYCLES; ++cy) {
                    const size_t w = (size_t)e * BASEQC_CYCLES + cy;
                    uint64_t any = qs[w] | qn[w] | al[w] | mm[w] | in[w] | de[w] | so[w];
                    for (int k = 0; k < BASEQC_BASES; ++k) any |= base[w * BASEQC_BASES + k];
                    if (any) last = cy;
                }
                for (int cy = 0; cy <= last; ++cy) {
                    const size_t w = (size_t)e * BASEQC_CYCLES + cy;
                    uint64_t n = 0;
                    for (int k = 0; k < BASEQC_BASES; ++k) n += base[w * BASEQC_BASES + k];
                    snprintf(buf, sizeof buf, "%d\t%llu\t%.4f", cy, (unsigned long long)n, ratio(qs[w], qn[w]));
                    o += buf;
                    for (int k = 0; k < BASEQC_BASES; ++k) { snprintf(buf, sizeof buf, "\t%.6f", ratio(base[w * BASEQC_BASES + k], n)); o += buf; }
                    snprintf(buf, sizeof buf, "\t%llu\t%.6f\t%llu\t%llu\t%llu\n", (unsigned long long)al[w], ratio(mm[w], al[w]), (unsigned long long)in[w],
                             (unsigned long long)de[w], (unsigned long long)so[w]);
                    o += buf;
                }
            }
        } else if (kind == BWAMEM_HIP_BASEQC_GC) {
            uint64_t win[BASEQC_GC_BINS];
            if (bwamem_hip_index_gc_windows(bwamem_baseqc_index(q), win) != 0) return nullptr;
            const std::vector<uint64_t> rd = array(BWAMEM_HIP_BASEQC_GCB_READS), gs = array(BWAMEM_HIP_BASEQC_GCB_QUAL_SUM), gn = array(BWAMEM_HIP_BASEQC_GCB_QUAL_N),
                rg = array(BWAMEM_HIP_BASEQC_READ_GC);
            uint64_t n_win = 0, n_rd = 0;
            for (int g = 0; g < BASEQC_GC_BINS; ++g) { n_win += win[g]; n_rd += rd[g]; }
            snprintf(buf, sizeof buf, "# gcb_skipped %llu\n", (unsigned long long)c.gcb_skipped);
            o += buf;
            o += "gc\twindows\treads\tnormalized_coverage\tmean_base_quality\n";
            for (int g = 0; g < BASEQC_GC_BINS; ++g) {
                const unsigned __int128 num = (unsigned __int128)rd[g] * n_win, den = (unsigned __int128)n_rd * win[g];
                snprintf(buf, sizeof buf, "%d\t%llu\t%llu\t%.6f\t%.4f\n", g, (unsigned long long)win[g], (unsigned long long)rd[g], den ? (double)num / (double)den : 0.0,
                         ratio(gs[g], gn[g]));
                o += buf;
            }
            o += "\ngc_percent\tend0\tend1\tend2\n";
            for (int g = 0; g < BASEQC_GC_BINS; ++g) {
                snprintf(buf, sizeof buf, "%d\t%llu\t%llu\t%llu\n", g, (unsigned long long)rg[g], (unsigned long long)rg[BASEQC_GC_BINS + g], (unsigned long long)rg[2 * BASEQC_GC_BINS + g]);
                o += buf;
            }
        } else return nullptr;
        char* r = (char*)malloc(o.size() + 1);
        if (!r) return nullptr;
        memcpy(r, o.c_str(), o.size() + 1);
        if (pBytes) *pBytes = o.size();
        return r;
    } catch (...) { return nullptr; }
}

}  // extern "C"
