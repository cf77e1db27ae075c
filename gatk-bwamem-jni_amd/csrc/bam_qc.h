// bam_qc.h -- alignment QC on the device (flagstat, idxstats, summary numbers, insert sizes): the rule, and the helpers the kernels
// (k_post.hip, next to the duplicate kernels) share with the host (pipeline.cpp, sam_writer.cpp).  Plain C++ that compiles for the
// device, the emulation build and the host.
//
// Scope: a reduction over BAM records.  Everything below is a function of the multiset of records alone, so it does not depend on
// their order (the same before and after the coordinate sort) and it adds across calls, devices and processes: the accumulator
// (bwamem_qc_t) is a block of integers, and adding two blocks is adding their words (min / max for the six extremes).  The
// definitions restate what samtools flagstat / idxstats / stats and Picard CollectInsertSizeMetrics document; parity with the
// output of those tools is not checked anywhere in this project (its machines have none of them): the checked contract is the rule
// below.  Per-cycle metrics and GC bias are a reduction of their own (bam_baseqc.h); per-base depth is not built.
//
// A record is block_size (int32) and block_size bytes of body; the fields sit where dup_end() (bam_dup.h) reads them: refID at 4,
// pos 8, l_read_name 12, mapq 13, n_cigar 16, flag 18, l_seq 20, next_refID 24, next_pos 28, tlen 32, then the name, the CIGAR,
// SEQ ((l_seq + 1) / 2 bytes), QUAL (l_seq bytes) and the aux fields.
//   f        flag;  w = 1 if f & 0x200 (the QC-fail column), else 0;  primary: f & 0x900 == 0;  mapped: f & 4 == 0
// Flagstat counters, a pair [w] each (QC_F_*, the order of bwamem_qc_counts_t)
//   total: every record.  f & 0x100: secondary.  Else f & 0x800: supplementary.  Else (primary): primary; mapped: primary_mapped;
//   f & 0x400: primary_duplicates; and if f & 1: paired; f & 2 and mapped: properly_paired; f & 0x40: read1; f & 0x80: read2;
//   f & 8 and mapped: singletons; neither f & 4 nor f & 8: both_mapped, and then refID != next_refID: mate_diff_chr, and then
//   mapq >= 5: mate_diff_chr_mapq5.  Every record: mapped (f & 4 == 0); duplicates (f & 0x400).
// Per contig
//   contig_mapped[refID] / contig_unmapped[refID] by f & 4, for refID >= 0; unplaced: refID < 0.  refID >= n_contigs is an error.
// Summary counters, over primary records
//   sequences; total_length (sum of l_seq); max_length; and over mapped primaries: reads_mq0 (mapq == 0), bases_mapped (l_seq),
//   bases_mapped_cigar (lengths of M, I, =, X), bases_soft_clipped (S), ins_events / ins_bases (I), del_events / del_bases (D),
//   mismatches (sum of NM), records_without_nm, mapq_hist[mapq].  NM of a record: the value of its FIRST aux field if that field's
//   tag is NM and its type one of c C s S i I, a negative value counting 0; otherwise (no aux area, another first field, another
//   type, or fewer bytes left than the field needs) the record adds 0 to mismatches and 1 to records_without_nm.  The aux area starts
//   at 36 + l_read_name + 4 * n_cigar + (l_seq + 1) / 2 + l_seq and is absent when that is the record's end.
//   qual_hist[min(q, 127)] over the QUAL bytes of primary records; a record whose first QUAL byte is 0xff contributes nothing.
// Insert sizes
//   a record contributes if f & 1, f & 0x40, f & 0xD0C == 0 (mapped, mate mapped, primary, no duplicate), refID == next_refID and
//   tlen != 0: once per template.  x = |tlen|.  Orientation, span = the reference span of the CIGAR (M D N = X): strand bits 0x10 and
//   0x20 equal: TANDEM; read forward: FR iff tlen > 0, else RF; read reverse: FR iff next_pos + 1 < pos + span, else RF.
//   isize_hist[o][min(x, BAMQC_ISIZE_BINS - 1)]; isize_min[o] / isize_max[o] of the uncapped x (UINT32_MAX / 0 when empty).
// Derived on the host from one orientation's histogram, a capped value standing for itself (qc_isize_stats)
//   n; median (the mean of the two middle values when n is even); MAD = the median of |v - median| by the same definition; mean and
//   sample standard deviation (n - 1; 0 below two values) over the values v <= median + 10 * MAD, accumulated in ascending bin order
//   with integer sums and turned into doubles at the end.
// Errors
//   block_size values that do not chain to the end of the stream; a record shorter than its own fields, or l_seq < 0; refID >=
//   n_contigs.  The call then returns non-zero with a message and the accumulator is exactly what it was: every call reduces into a
//   zeroed block of its own on the device, which the host adds to its totals only when the error word is clear.
//
// The steps (launch_qc_*).  Two layouts of a batch: grouped by read (off = bam_off[n_reads + 1], a lane walks its read's records
// along block_size) and one record per item (off = the per-record places the sort and the BAI kernels use, or the host's walk of a
// plain stream).  (a) k_qc_records, one lane per item, a fixed grid that strides over the items: the fields, the CIGAR and the first
// aux field of a record by its lane (qc_record); the flag counters by ballot and popcount, held by the lane whose number is the
// counter's; the sums added up over the wave; equal (refID, unmapped) combined within the wave before one global add per distinct
// value; mapq_hist and the insert sizes below BAMQC_ISIZE_LDS in LDS copies of the workgroup, flushed once per workgroup, larger
// insert sizes straight to HBM.  (b) k_qc_qual, lane groups as k_dup_scores: the group finds its item's primary records itself and
// shares out QUAL in aligned 32-bit words, into a workgroup's qual_hist in LDS, flushed once.  Integer adds only, so the block is
// bitwise reproducible.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "bam_sort.h"

#define QC_HD static __host__ __device__ inline

enum { BAMQC_ERR_WALK = 1,               // block_size values do not chain, a record is shorter than its own fields, or l_seq < 0
       BAMQC_ERR_CONTIG = 2 };           // refID >= n_contigs
enum { BAMQC_ISIZE_BINS = 16384, BAMQC_ISIZE_LDS = 1024, BAMQC_MAPQ_BINS = 256, BAMQC_QUAL_BINS = 128 };
enum { QC_FR = 0, QC_RF, QC_TANDEM, QC_ORIENTATIONS };
// the flagstat counters, in the order of bwamem_qc_counts_t
enum { QC_F_TOTAL = 0, QC_F_PRIMARY, QC_F_SECONDARY, QC_F_SUPPLEMENTARY, QC_F_DUPLICATES, QC_F_PRIMARY_DUPLICATES, QC_F_MAPPED, QC_F_PRIMARY_MAPPED, QC_F_PAIRED,
       QC_F_READ1, QC_F_READ2, QC_F_PROPERLY_PAIRED, QC_F_BOTH_MAPPED, QC_F_SINGLETONS, QC_F_MATE_DIFF_CHR, QC_F_MATE_DIFF_CHR_MAPQ5, QC_F_N };
// the single counters, in the order of bwamem_qc_counts_t (max_length is a maximum, the others are sums)
enum { QC_S_UNPLACED = 0, QC_S_SEQUENCES, QC_S_TOTAL_LENGTH, QC_S_MAX_LENGTH, QC_S_READS_MQ0, QC_S_BASES_MAPPED, QC_S_BASES_MAPPED_CIGAR, QC_S_BASES_SOFT_CLIPPED,
       QC_S_INS_EVENTS, QC_S_INS_BASES, QC_S_DEL_EVENTS, QC_S_DEL_BASES, QC_S_MISMATCHES, QC_S_RECORDS_WITHOUT_NM, QC_S_N };
// The block of 64-bit words, on the device (one call) and in the accumulator (the totals).  On the device QC_W_ERR holds the error
// flags and the extremes are kept for atomicMax on the low 32 bits of a zeroed word: max as x - 1, min as 0x7fffffff - (x - 1)
// (x in [1, 2^31]); a word means something only when its orientation's histogram of that call is not empty (qc_dev_min / _max).
enum { QC_W_ERR = 0, QC_W_FLAG = 2, QC_W_SUM = QC_W_FLAG + 2 * QC_F_N, QC_W_ISIZE_MIN = QC_W_SUM + QC_S_N, QC_W_ISIZE_MAX = QC_W_ISIZE_MIN + QC_ORIENTATIONS,
       QC_W_MAPQ = 64, QC_W_QUAL = QC_W_MAPQ + BAMQC_MAPQ_BINS, QC_W_ISIZE = QC_W_QUAL + BAMQC_QUAL_BINS, QC_W_CONTIG = QC_W_ISIZE + QC_ORIENTATIONS * BAMQC_ISIZE_BINS };
static_assert(QC_W_ISIZE_MAX + QC_ORIENTATIONS <= QC_W_MAPQ, "the counters fit below the histograms");
QC_HD size_t qc_words(int32_t n_contigs) { return (size_t)QC_W_CONTIG + 2 * (size_t)n_contigs; }      // contig c: mapped at 2c, unmapped at 2c + 1
QC_HD int32_t qc_dev_max_enc(uint32_t x) { return (int32_t)(x - 1); }
QC_HD int32_t qc_dev_min_enc(uint32_t x) { return (int32_t)(0x7fffffffu - (x - 1)); }
QC_HD uint64_t qc_dev_max(uint64_t word) { return (uint64_t)(uint32_t)word + 1; }
QC_HD uint64_t qc_dev_min(uint64_t word) { return (uint64_t)(0x7fffffffu - (uint32_t)word) + 1; }

QC_HD uint32_t qc_ld16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }

// what a record adds
struct QcRec {
    uint32_t fmask;              // bit k: counts QC_F_k
    int32_t w;                   // its column
    int32_t refid, l_seq, mapq;
    bool primary, mapped_primary, no_nm;
    int64_t qual_off;            // QUAL, from the record's first byte
    uint64_t m_cigar, soft, ins_ev, ins_b, del_ev, del_b, nm;     // of a mapped primary
    int32_t orient;              // QC_FR .. QC_TANDEM, or -1: no insert size
    uint32_t x;                  // |tlen|
};

// The record at rec (size bytes = 4 + block_size, >= BAMSORT_MIN_REC) -> 0, or BAMQC_ERR_*
QC_HD int qc_record(const uint8_t* rec, int64_t size, int32_t n_contigs, QcRec& q)
{
    const int32_t refid = (int32_t)bamsort_ld32(rec + 4), pos = (int32_t)bamsort_ld32(rec + 8);
    const int64_t l_name = rec[12], n_cig = qc_ld16(rec + 16);
    const int32_t mapq = rec[13], l_seq = (int32_t)bamsort_ld32(rec + 20);
    const uint32_t f = qc_ld16(rec + 18);
    const int32_t next_refid = (int32_t)bamsort_ld32(rec + 24), next_pos = (int32_t)bamsort_ld32(rec + 28), tlen = (int32_t)bamsort_ld32(rec + 32);
    if (l_seq < 0) return BAMQC_ERR_WALK;
    const int64_t qo = 36 + l_name + 4 * n_cig + ((int64_t)l_seq + 1) / 2, aux = qo + l_seq;
    if (aux > size) return BAMQC_ERR_WALK;
    if (refid >= n_contigs) return BAMQC_ERR_CONTIG;
    const bool mapped = !(f & 4), primary = !(f & 0x900);
    uint32_t m = 1u << QC_F_TOTAL;
    if (f & 0x100) m |= 1u << QC_F_SECONDARY;
    else if (f & 0x800) m |= 1u << QC_F_SUPPLEMENTARY;
    else {
        m |= 1u << QC_F_PRIMARY;
        if (mapped) m |= 1u << QC_F_PRIMARY_MAPPED;
        if (f & 0x400) m |= 1u << QC_F_PRIMARY_DUPLICATES;
        if (f & 1) {
            m |= 1u << QC_F_PAIRED;
            if ((f & 2) && mapped) m |= 1u << QC_F_PROPERLY_PAIRED;
            if (f & 0x40) m |= 1u << QC_F_READ1;
            if (f & 0x80) m |= 1u << QC_F_READ2;
            if ((f & 8) && mapped) m |= 1u << QC_F_SINGLETONS;
            if (!(f & 4) && !(f & 8)) {
                m |= 1u << QC_F_BOTH_MAPPED;
                if (refid != next_refid) {
                    m |= 1u << QC_F_MATE_DIFF_CHR;
                    if (mapq >= 5) m |= 1u << QC_F_MATE_DIFF_CHR_MAPQ5;
                }
            }
        }
    }
    if (mapped) m |= 1u << QC_F_MAPPED;
    if (f & 0x400) m |= 1u << QC_F_DUPLICATES;
    q.fmask = m; q.w = (f & 0x200) ? 1 : 0; q.refid = refid; q.l_seq = l_seq; q.mapq = mapq;
    q.primary = primary; q.mapped_primary = primary && mapped; q.qual_off = qo;
    q.m_cigar = q.soft = q.ins_ev = q.ins_b = q.del_ev = q.del_b = q.nm = 0; q.no_nm = false; q.orient = -1; q.x = 0;
    const bool isz = (f & 1) && (f & 0x40) && !(f & 0xD0C) && refid == next_refid && tlen != 0;
    if (!q.mapped_primary) return 0;                                   // (an insert size needs a mapped primary too)
    const uint8_t* cig = rec + 36 + l_name;
    int64_t span = 0;
    for (int64_t c = 0; c < n_cig; ++c) {
        const uint32_t x = bamsort_ld32(cig + 4 * c), op = x & 0xf;
        const uint64_t len = x >> 4;
        if (op == 0 || op == 7 || op == 8) { q.m_cigar += len; span += (int64_t)len; }
        else if (op == 1) { q.m_cigar += len; q.ins_ev += 1; q.ins_b += len; }
        else if (op == 2) { q.del_ev += 1; q.del_b += len; span += (int64_t)len; }
        else if (op == 3) span += (int64_t)len;
        else if (op == 4) q.soft += len;
    }
    q.no_nm = true;
    if (aux + 3 <= size && rec[aux] == 'N' && rec[aux + 1] == 'M') {
        const uint8_t t = rec[aux + 2];
        const uint8_t* v = rec + aux + 3;
        const int64_t left = size - aux - 3;
        if ((t == 'c' || t == 'C') && left >= 1) { q.no_nm = false; q.nm = t == 'C' ? (uint64_t)v[0] : (uint64_t)((int8_t)v[0] < 0 ? 0 : v[0]); }
        else if ((t == 's' || t == 'S') && left >= 2) { const uint32_t u = qc_ld16(v); q.no_nm = false; q.nm = t == 'S' ? (uint64_t)u : (uint64_t)((int16_t)u < 0 ? 0 : u); }
        else if ((t == 'i' || t == 'I') && left >= 4) { const uint32_t u = bamsort_ld32(v); q.no_nm = false; q.nm = t == 'I' ? (uint64_t)u : (uint64_t)((int32_t)u < 0 ? 0 : u); }
    }
    if (isz) {
        q.x = tlen < 0 ? 0u - (uint32_t)tlen : (uint32_t)tlen;
        const bool rev = (f & 0x10) != 0, mrev = (f & 0x20) != 0;
        if (rev == mrev) q.orient = QC_TANDEM;
        else if (!rev) q.orient = tlen > 0 ? QC_FR : QC_RF;
        else q.orient = (int64_t)next_pos + 1 < (int64_t)pos + span ? QC_FR : QC_RF;
    }
    return 0;
}

// one QUAL byte's bin
QC_HD uint32_t qc_qual_bin(uint32_t b) { return b < BAMQC_QUAL_BINS - 1 ? b : BAMQC_QUAL_BINS - 1; }

// what the kernels see
struct QcView {
    const uint8_t* bam;           // the records
    const int64_t* off;           // [n_items + 1] grouped != 0: the reads' records (bam_off); else the records' places
    int32_t n_items, grouped, n_contigs;
    unsigned long long* blk;      // [qc_words(n_contigs)], zeroed by the caller
};

// ---- host only: the numbers derived from one orientation's histogram
struct QcIsizeStats { uint64_t n; double median, mad, mean, sd; };
// the median of the multiset {value v, cnt[v] times}, v in [0, n_bins), n > 0 values in all
static inline double qc_hist_median(const uint64_t* cnt, size_t n_bins, uint64_t n)
{
    const uint64_t k0 = (n - 1) / 2, k1 = n / 2;                       // the two middle values (the same one when n is odd)
    uint64_t seen = 0; double a = 0, b = 0; bool has_a = false;
    for (size_t v = 0; v < n_bins; ++v) {
        if (!cnt[v]) continue;
        seen += cnt[v];
        if (!has_a && seen > k0) { a = (double)v; has_a = true; }
        if (seen > k1) { b = (double)v; break; }
    }
    return (a + b) / 2;
}
static inline QcIsizeStats qc_isize_stats(const uint64_t* h /* [BAMQC_ISIZE_BINS] */)
{
    QcIsizeStats s = { 0, 0, 0, 0, 0 };
    for (int v = 0; v < BAMQC_ISIZE_BINS; ++v) s.n += h[v];
    if (!s.n) return s;
    s.median = qc_hist_median(h, BAMQC_ISIZE_BINS, s.n);
    // |v - median| in half units (the median is a multiple of 1/2): an integer histogram again
    const int64_t m2 = (int64_t)(2 * s.median);
    uint64_t* dev = (uint64_t*)calloc(2 * BAMQC_ISIZE_BINS, sizeof(uint64_t));
    if (!dev) return s;
    for (int v = 0; v < BAMQC_ISIZE_BINS; ++v) if (h[v]) { const int64_t d = 2 * (int64_t)v - m2; dev[d < 0 ? -d : d] += h[v]; }
    s.mad = qc_hist_median(dev, 2 * BAMQC_ISIZE_BINS, s.n) / 2;
    free(dev);
    const double lim = s.median + 10 * s.mad;
    unsigned __int128 sum = 0, sq = 0; uint64_t m = 0;
    for (int v = 0; v < BAMQC_ISIZE_BINS; ++v) if (h[v] && (double)v <= lim) { m += h[v]; sum += (unsigned __int128)h[v] * (uint64_t)v; sq += (unsigned __int128)h[v] * (uint64_t)v * (uint64_t)v; }
    if (m) s.mean = (double)sum / (double)m;
    if (m >= 2) {
        // sum of squared deviations = (m * sq - sum^2) / m, exact in integers up to the division
        const unsigned __int128 num = (unsigned __int128)m * sq - sum * sum;
        const double var = (double)num / (double)m / (double)(m - 1);
        s.sd = var > 0 ? __builtin_sqrt(var) : 0;
    }
    return s;
}
