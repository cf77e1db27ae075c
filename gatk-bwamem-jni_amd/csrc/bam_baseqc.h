// bam_baseqc.h -- base-level QC on the device (quality, base and mismatch tables per sequencing cycle, GC bias): the rule, and the
// helpers the kernels (k_post.hip, next to k_qc_*) share with the host (pipeline.cpp, sam_writer.cpp).  Plain C++ that compiles
// for the device, the emulation build and the host.
//
// Scope: a second reduction over BAM records, beside bam_qc.h and apart from it (a type, a block and a serialized form of its own).
// Everything below is a function of the multiset of records and of the index alone, so it is the same before and after the sort and
// adds across calls, devices and processes: adding two blocks is adding their words.  The tables restate what Picard
// MeanQualityByCycle, BaseDistributionByCycle and CollectGcBiasMetrics and the mismatch, indel and GC sections of samtools stats
// document; parity with the output of those tools is not checked anywhere in this project (its machines have none of them): the
// checked contract is the rule below.  The GC-bias window is simpler than Picard's: a window that touches any .amb hole is left
// out, where Picard leaves out windows with more than four N.  Per-base depth is not built.
//
// Records and fields: as bam_qc.h documents them (block_size, then refID at 4, pos 8, l_read_name 12, n_cigar 16, flag 18, l_seq 20,
// the name, the CIGAR, SEQ, QUAL).  Only primary records (f & 0x900 == 0) contribute; a primary with f & 0x200 contributes nothing
// and counts in qcfail_skipped; every other primary counts in records[e].
//   end e     1 if f & 1 and f & 0x40; 2 if f & 1 and f & 0x80 and not 0x40; else 0
//   cycle     Hl / Hr = the length of the first / last CIGAR operation when that is an H (Hr only when n_cigar > 1), else 0.  SEQ index
//             i was read at cycle c = Hl + i when f & 0x10 is clear, c = Hr + (l_seq - 1 - i) when it is set -- also for an unmapped
//             record, because SEQ is stored that way.  Bin = min(max(c, 0), BASEQC_CYCLES - 1): a capped value stands for itself.
// Every contributing record, mapped or not, with l_seq > 0
//   base[e][c][k]   k = A C G T N from the 4-bit code (1 2 4 8, anything else N); with f & 0x10, A<->T and C<->G are swapped: the table
//                   is in sequencing orientation
//   qual_sum[e][c] += QUAL[i], qual_n[e][c] += 1, unless the record's first QUAL byte is 0xff
//   read_gc[e][b] += 1, b = (200 * gc + n) / (2 * n) with n the A/C/G/T bases and gc the C/G bases of the read; nothing when n == 0
// Mapped primaries (f & 4 == 0): the CIGAR walked against the packed reference; the reference base at contig position p is the 2-bit
// code at ann_offset[refID] + p.  Inside .amb holes that is whatever the .pac holds, which is what NM was computed from.
//   M = X     aligned[e][c] += 1; mism[e][c] += 1 when the read's code is not exactly the reference base (a read N is a mismatch)
//   I         ins[e][c] += 1 per inserted base;  S: soft[e][c] += 1 per base
//   D         del_ev[e][c] += 1 once per operation, at the cycle of SEQ index i - 1, i the index of the next read base
//   N H P and the undefined operations 9..15 add nothing
// Errors: the whole call is refused and the accumulator stays exactly as it was
//   BASEQC_ERR_WALK    as in bam_qc.h: block_size values that do not chain, a record shorter than its own fields, l_seq < 0
//   BASEQC_ERR_CONTIG  refID >= n_contigs (any record)
//   BASEQC_ERR_CIGAR   a mapped primary with n_cigar == 0, or whose read-consuming lengths (M I S = X) do not sum to l_seq, or with an
//                      H that is not the first or the last operation
//   BASEQC_ERR_RANGE   a mapped primary with refID < 0, pos < 0 or pos + span > the contig's length (span: M D N = X)
//   k_bqc_check establishes all of this for every record before any kernel reads a reference byte.
// GC bias (window W = BASEQC_WINDOW = 100, Picard's default): the window of a mapped primary starts at s = pos (forward) or
// s = pos + span - W (reverse).  It is valid iff s >= 0, s + W <= the contig's length and [s, s + W) overlaps no .amb hole.
//   valid     g = the C/G among the window's reference bases; gcb_reads[g] += 1; with qualities gcb_qual_sum[g] += the sum of QUAL and
//             gcb_qual_n[g] += l_seq
//   invalid   gcb_skipped += 1
//   windows[g], the denominator, is a property of the index: the valid starts over all contigs with that GC count (k_gc_windows).  It is
//   not part of the block, of its sums or of the serialized form.
//
// The block: 64-bit words in the order of the BQ_W_* below -- the error word, a word the device uses for the longest contributing
// read of the call (0 in an accumulator), the counters, then the tables, a table [e][c] (base: [e][c][k]) flattened in that order.
//
// The steps (launch_bqc_*), over both layouts of a batch as bam_qc.h has them.  (a) k_bqc_check, one lane per item: every check
// above, records[], qcfail_skipped and the longest read.  Nothing else runs when it leaves an error.  (b) k_bqc_bases and
// (c) k_bqc_aligned, lane groups of G = 8 lanes per item (the wavefront when the longest read is above 1 000) on a fixed grid that
// strides over the items: the group finds its item's contributing records itself; (b) shares out QUAL in aligned 32-bit words
// and reads SEQ by bytes, (c) shares out the SEQ indices of every CIGAR operation, reads the reference 16 bases per 32-bit load and
// takes the window's GC as a masked popcount of the window's words.  The tables do not fit in LDS: a workgroup keeps 32-bit copies of
// the cycles below BASEQC_LDS_CYCLES, flushed once with one global add per non-zero word; cycles above go to HBM directly, except
// the capped last bin (where nearly every base of a 10 kb read lands), which a lane keeps in registers and adds once per record.
// Integer atomics only: the block is bitwise reproducible and equals the emulation build's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bam_sort.h"
#include "bam_qc.h"

#define BQ_HD static __host__ __device__ inline

enum { BASEQC_ERR_WALK = 1, BASEQC_ERR_CONTIG = 2, BASEQC_ERR_CIGAR = 4, BASEQC_ERR_RANGE = 8 };
enum { BASEQC_CYCLES = 1024, BASEQC_LDS_CYCLES = 256, BASEQC_ENDS = 3, BASEQC_BASES = 5, BASEQC_WINDOW = 100, BASEQC_GC_BINS = 101 };
enum { BQ_T = BASEQC_ENDS * BASEQC_CYCLES };      // words of one [e][c] table
enum { BQ_W_ERR = 0, BQ_W_MAX_LEN = 1, BQ_W_RECORDS = 2, BQ_W_QCFAIL = BQ_W_RECORDS + BASEQC_ENDS, BQ_W_GCB_SKIPPED, BQ_W_BASE = 8,
       BQ_W_QUAL_SUM = BQ_W_BASE + BQ_T * BASEQC_BASES, BQ_W_QUAL_N = BQ_W_QUAL_SUM + BQ_T, BQ_W_ALIGNED = BQ_W_QUAL_N + BQ_T, BQ_W_MISM = BQ_W_ALIGNED + BQ_T,
       BQ_W_INS = BQ_W_MISM + BQ_T, BQ_W_DEL = BQ_W_INS + BQ_T, BQ_W_SOFT = BQ_W_DEL + BQ_T, BQ_W_READ_GC = BQ_W_SOFT + BQ_T,
       BQ_W_GCB_READS = BQ_W_READ_GC + BASEQC_ENDS * BASEQC_GC_BINS, BQ_W_GCB_QUAL_SUM = BQ_W_GCB_READS + BASEQC_GC_BINS,
       BQ_W_GCB_QUAL_N = BQ_W_GCB_QUAL_SUM + BASEQC_GC_BINS, BQ_WORDS = BQ_W_GCB_QUAL_N + BASEQC_GC_BINS };
static_assert(BQ_W_GCB_SKIPPED < BQ_W_BASE, "the counters fit below the tables");

// an .amb hole in the coordinates of the packed reference: [off, end); the list is sorted and its members are disjoint
struct BqcHole { int64_t off, end; };

// what a record is to this reduction
struct BqcRec {
    uint32_t f;
    int32_t refid, pos, l_seq, n_cig, e;
    bool primary, counted, mapped, rev;          // counted: a primary without 0x200; mapped: counted and f & 4 == 0
    int64_t cig_off, seq_off, qual_off;          // from the record's first byte
    int64_t hl, hr;
    int64_t span;                                // of a mapped primary that passed bqc_mapped
};

// The record at rec (size bytes = 4 + block_size, >= BAMSORT_MIN_REC): its fields -> 0, or BASEQC_ERR_WALK / _CONTIG
BQ_HD int bqc_fields(const uint8_t* rec, int64_t size, int32_t n_contigs, BqcRec& r)
{
    r.refid = (int32_t)bamsort_ld32(rec + 4); r.pos = (int32_t)bamsort_ld32(rec + 8);
    r.n_cig = (int32_t)qc_ld16(rec + 16); r.f = qc_ld16(rec + 18); r.l_seq = (int32_t)bamsort_ld32(rec + 20);
    if (r.l_seq < 0) return BASEQC_ERR_WALK;
    r.cig_off = 36 + (int64_t)rec[12]; r.seq_off = r.cig_off + 4 * (int64_t)r.n_cig; r.qual_off = r.seq_off + ((int64_t)r.l_seq + 1) / 2;
    if (r.qual_off + r.l_seq > size) return BASEQC_ERR_WALK;
    if (r.refid >= n_contigs) return BASEQC_ERR_CONTIG;
    r.primary = !(r.f & 0x900); r.counted = r.primary && !(r.f & 0x200); r.mapped = r.counted && !(r.f & 4); r.rev = (r.f & 0x10) != 0;
    r.e = (r.f & 1) ? ((r.f & 0x40) ? 1 : (r.f & 0x80) ? 2 : 0) : 0;
    r.hl = r.hr = 0; r.span = 0;
    if (r.n_cig > 0) {
        const uint32_t a = bamsort_ld32(rec + r.cig_off), b = bamsort_ld32(rec + r.cig_off + 4 * (int64_t)(r.n_cig - 1));
        if ((a & 0xf) == 5) r.hl = (int64_t)(a >> 4);
        if (r.n_cig > 1 && (b & 0xf) == 5) r.hr = (int64_t)(b >> 4);
    }
    return 0;
}

// The CIGAR and the place of a mapped primary (every one, counted or not) against its contig -> 0 and r.span, or BASEQC_ERR_CIGAR / _RANGE
BQ_HD int bqc_mapped(const uint8_t* rec, const int32_t* ann_len, BqcRec& r)
{
    if (r.n_cig == 0) return BASEQC_ERR_CIGAR;
    int64_t read = 0, span = 0;
    for (int32_t c = 0; c < r.n_cig; ++c) {
        const uint32_t x = bamsort_ld32(rec + r.cig_off + 4 * (int64_t)c), op = x & 0xf;
        const int64_t len = (int64_t)(x >> 4);
        if (op == 0 || op == 7 || op == 8) { read += len; span += len; }
        else if (op == 1 || op == 4) read += len;
        else if (op == 2 || op == 3) span += len;
        else if (op == 5 && c != 0 && c != r.n_cig - 1) return BASEQC_ERR_CIGAR;
    }
    if (read != (int64_t)r.l_seq) return BASEQC_ERR_CIGAR;
    if (r.refid < 0 || r.pos < 0 || (int64_t)r.pos + span > (int64_t)ann_len[r.refid]) return BASEQC_ERR_RANGE;
    r.span = span;
    return 0;
}

// the bin of SEQ index i (i = -1: a D before the first read base)
BQ_HD int32_t bqc_bin(const BqcRec& r, int64_t i)
{
    const int64_t c = r.rev ? r.hr + ((int64_t)r.l_seq - 1 - i) : r.hl + i;
    return (int32_t)(c < 0 ? 0 : c < BASEQC_CYCLES - 1 ? c : BASEQC_CYCLES - 1);
}
// the base of SEQ index i as the reference would have it: 0..3 = A C G T, 4 = N; and its column of base[] (sequencing orientation)
BQ_HD int32_t bqc_code(const uint8_t* seq, int64_t i)
{
    const uint32_t nib = seq[i >> 1] >> ((~i & 1) << 2) & 0xf;
    return nib == 1 ? 0 : nib == 2 ? 1 : nib == 4 ? 2 : nib == 8 ? 3 : 4;
}
BQ_HD int32_t bqc_column(int32_t code, bool rev) { return rev && code < 4 ? 3 - code : code; }
BQ_HD int32_t bqc_read_gc_bin(uint64_t gc, uint64_t n) { return (int32_t)((200 * gc + n) / (2 * n)); }       // n > 0

// The packed reference by 32-bit words of 16 bases (little-endian loads: base k of a word sits in byte k / 4 at bits 7 - 2 (k % 4)):
// with the bytes swapped, base k is bits 31 - 2k and 30 - 2k
BQ_HD int32_t bqc_word_base(uint32_t v, int k) { return (int32_t)(__builtin_bswap32(v) >> (30 - 2 * k) & 3u); }
// the C/G among bases [a, b) of a word, 0 <= a <= b <= 16: C = 01 and G = 10, so the two bits of a base differ
BQ_HD int32_t bqc_word_gc(uint32_t v, int a, int b)
{
    const uint32_t s = __builtin_bswap32(v), x = (s ^ s >> 1) & 0x55555555u;
    const uint32_t from_a = a < 16 ? 0x55555555u >> (2 * a) : 0u, from_b = b < 16 ? 0x55555555u >> (2 * b) : 0u;
    return (int32_t)__builtin_popcount(x & from_a & ~from_b);
}

// the first hole that ends after g (n: none)
BQ_HD int32_t bqc_first_hole(const BqcHole* h, int32_t n, int64_t g)
{
    int32_t lo = 0, hi = n;
    while (lo < hi) { const int32_t mid = lo + (hi - lo) / 2; if (h[mid].end <= g) lo = mid + 1; else hi = mid; }
    return lo;
}
// [g, g + BASEQC_WINDOW) overlaps no hole
BQ_HD bool bqc_window_clear(const BqcHole* h, int32_t n, int64_t g)
{
    const int32_t k = bqc_first_hole(h, n, g);
    return k >= n || h[k].off >= g + BASEQC_WINDOW;
}

// what the kernels see
struct BqcView {
    const uint8_t* bam;           // the records
    const int64_t* off;           // [n_items + 1], as QcView
    int32_t n_items, grouped, n_contigs, n_holes;
    const uint8_t* pac;           // the packed reference, 4-byte aligned and readable to the end of the word of its last base
    const int64_t* ann_offset; const int32_t* ann_len;
    const BqcHole* holes;
    unsigned long long* blk;      // [BQ_WORDS], zeroed by the caller
};
// k_gc_windows: the valid windows of the whole index by GC count
struct GcWinView {
    const uint8_t* pac; int64_t l_pac, pac_bytes;      // pac_bytes: what may be read, a multiple of 4
    const int64_t* ann_offset; const int32_t* ann_len; int32_t n_contigs, n_holes;
    const BqcHole* holes;
    unsigned long long* out;      // [BASEQC_GC_BINS], zeroed by the caller
};
