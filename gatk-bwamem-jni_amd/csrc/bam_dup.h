// bam_dup.h -- duplicate marking on the device, between the encoder and the coordinate sort: the rules, and the helpers the
// kernels (k_post.hip, next to the sort and BAI kernels) share with the host (pipeline.cpp).  Plain C++ that compiles for the
// device, the emulation build and the host.
//
// Scope: one logical call (one encoded batch) is marked within itself, as it is sorted within itself (bam_sort.h).  Duplicates
// across calls need the merge of runs that is not built.  No optical duplicates, one library, duplicates are flagged and not
// removed.  The rule restates what Picard MarkDuplicates documents; parity with Picard's own output is not checked anywhere in
// this project (its machines have neither a JVM nor Picard): the checked contract is the rule below, which is defined on the BAM
// records of the batch alone.
//
// Definitions
//   template        a read (paired == 0) or the reads 2i and 2i + 1 (paired != 0); an odd trailing read is a template of its own
//                   (the encoder gives it no record)
//   primary record  of a read: its record with flag & 0x900 == 0; a read with two of them is an error
//   end             of a mapped primary record (flag & 4 == 0): (refID, u, strand), strand = flag & 0x10, u = the unclipped 5'
//                   coordinate, 0-based.  Forward: u = pos - the lengths of the leading S and H operations.  Reverse:
//                   u = pos + the reference span of the CIGAR (M, D, N, =, X) - 1 + the lengths of the trailing S and H operations.
//                   As a key: refID << 33 | (u + 2^31) << 1 | (strand != 0).  refID outside [0, 2^30), pos < 0, or u + 2^31
//                   outside [0, 2^32) is an error and the call fails.
//   score           of a read: the sum of the bytes >= 15 of its primary record's QUAL, 0xff counting 0, capped at 16 383; of a
//                   template: the sum over its mapped primaries
//   fragment entry  one per mapped primary record: (end, is_paired, read score, template index); is_paired = flag 0x1 set and 0x8
//                   clear
//   pair entry      one per template with both primaries mapped: (end A, end B), the two end keys in ascending order -- by
//                   (refID, u), the forward end first on a tie.  Which read is first of the pair does not enter.
// Groups and keepers
//   groups          fragment entries with equal end; pair entries with equal (end A, end B)
//   pair group      the keeper is the highest template score, among equal scores the lowest template index; every other template
//                   of the group is a duplicate
//   fragment group  with a paired entry: every entry that is not paired is a duplicate, the paired entries are not decided here.
//                   Without one: the keeper is the highest score, then the lowest index; the rest are duplicates.
// Effect
//   a duplicate template gets 0x400 set on every record it has (primary, secondary, supplementary, the unmapped mate's); every
//   other record gets it cleared -- the bit of the input is ignored, so a second call changes nothing.  Secondary and supplementary
//   records create no entries; a template without a mapped primary is never a duplicate.  Only byte 19 of a record (the high
//   byte of flag) is ever written.
// Counts (bwamem_dup_counts_t, in this order; DUP_CNT_*)
//   unpaired reads examined (fragment entries that are not paired), read pairs examined (pair entries), secondary-or-supplementary
//   records, unmapped reads (primary records with flag & 4), unpaired read duplicates (fragment entries marked), read pair
//   duplicates (pair entries marked)
//
// The steps (launch_dup_*): (a) one lane per template walks its records along block_size and writes the end keys, the pair keys,
// is_paired, the place of QUAL and the counts; (b) lane groups add up QUAL; (c) the entries are sorted with the stable sort of
// bam_sort.h -- by the score key (fragments: is_paired above it, so paired entries come first), then pairs by end B and end A,
// fragments by the end -- the run starts are marked and scanned, and every entry looks at the head of its run: the head is the
// keeper (for fragments: the witness of a paired entry); (d) one lane per template rewrites byte 19 of its records.  Every output
// byte has one writer, and the result is a function of the records alone.  An absent entry has the key SORT_KEY_LAST: it is left
// out of the OR / AND of the keys, and only the last sort of a chain has to put it behind the others.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bam_sort.h"

#define DUP_HD static __host__ __device__ inline

enum { BAMDUP_ERR_WALK = 1,              // block_size values do not chain, or a record is shorter than its own fields
       BAMDUP_ERR_KEY = 2,               // refID, pos or the unclipped coordinate does not fit the key
       BAMDUP_ERR_PRIMARY = 4 };         // a read with more than one primary record
enum { DUP_SCORE_CAP = 16383, DUP_MIN_QUAL = 15 };
// the words of the device's counter block
enum { DUP_CNT_ERR = 0, DUP_CNT_MAX_LEN, DUP_CNT_UNPAIRED, DUP_CNT_PAIRS, DUP_CNT_SECONDARY, DUP_CNT_UNMAPPED, DUP_CNT_UNPAIRED_DUP, DUP_CNT_PAIR_DUP, DUP_CNT_N = 16 };
// the OR / AND words (SORT_BITS_N each) of the five key arrays
enum { DUP_BITS_FRAG_END = 0, DUP_BITS_PAIR_A, DUP_BITS_PAIR_B, DUP_BITS_FRAG_SCORE, DUP_BITS_PAIR_SCORE, DUP_BITS_SETS };

DUP_HD uint32_t dup_ld16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
DUP_HD int dup_templates(int n_reads, int paired) { return paired ? (n_reads + 1) / 2 : n_reads; }

// what the walk keeps of a mapped primary record
struct DupEnd { uint64_t key; int64_t qual_off; int32_t l_seq; int32_t flag; };

// The end of the mapped primary record at rec (size bytes, the first of them at byte rec_off of the stream) -> 0, or BAMDUP_ERR_*
DUP_HD int dup_end(const uint8_t* rec, int64_t size, int64_t rec_off, DupEnd& e)
{
    const int32_t refid = (int32_t)bamsort_ld32(rec + 4), pos = (int32_t)bamsort_ld32(rec + 8);
    const int64_t l_name = rec[12], n_cig = dup_ld16(rec + 16);
    const int32_t flag = (int32_t)dup_ld16(rec + 18), l_seq = (int32_t)bamsort_ld32(rec + 20);
    if (l_seq < 0) return BAMDUP_ERR_WALK;
    const int64_t q = 36 + l_name + 4 * n_cig + ((int64_t)l_seq + 1) / 2;
    if (q + l_seq > size) return BAMDUP_ERR_WALK;
    if (refid < 0 || refid >= (1 << 30) || pos < 0) return BAMDUP_ERR_KEY;
    const uint8_t* cig = rec + 36 + l_name;
    int64_t span = 0, lead = 0, trail = 0;
    bool in_lead = true;
    for (int64_t c = 0; c < n_cig; ++c) {
        const uint32_t x = bamsort_ld32(cig + 4 * c), op = x & 0xf;
        const int64_t len = x >> 4;
        if (op == 4 || op == 5) { if (in_lead) lead += len; else trail += len; }
        else {
            in_lead = false; trail = 0;
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) span += len;
        }
    }
    const int64_t u = (flag & 0x10) ? (int64_t)pos + span - 1 + trail : (int64_t)pos - lead;
    const int64_t ub = u + ((int64_t)1 << 31);
    if (ub < 0 || ub > 0xffffffffll) return BAMDUP_ERR_KEY;
    e.key = (uint64_t)refid << 33 | (uint64_t)ub << 1 | ((flag & 0x10) ? 1u : 0u);
    e.qual_off = rec_off + q; e.l_seq = l_seq; e.flag = flag;
    return 0;
}

// one QUAL byte's part of the score
DUP_HD int32_t dup_qual(uint32_t b) { return b >= DUP_MIN_QUAL && b != 0xff ? (int32_t)b : 0; }
DUP_HD int32_t dup_qual4(uint32_t w) { return dup_qual(w & 0xff) + dup_qual(w >> 8 & 0xff) + dup_qual(w >> 16 & 0xff) + dup_qual(w >> 24); }

// the first sort key of an entry: a higher score sorts first; fragments: the paired entries before all others
DUP_HD uint64_t dup_score_key(int32_t score, bool not_paired) { return (uint64_t)(not_paired ? 1 : 0) << 16 | (uint64_t)(0xffff - score); }

// the passes of a sort that does not have to place the absent entries (every sort of a chain but the last)
DUP_HD uint32_t dup_live_bytes_inner(const int32_t* w /* [SORT_BITS_N] */)
{
    int32_t v[SORT_BITS_N];
    for (int k = 0; k < SORT_BITS_N; ++k) v[k] = w[k];
    v[SORT_BITS_HAS_LAST] = 0;
    return sort_live_bytes(v);
}

// what the kernels see
struct DupView {
    uint8_t* bam;                 // the records, grouped by read ...
    const int64_t* bam_off;       // ... [n_reads + 1]
    int32_t n_reads, n_tmpl, paired;
    uint64_t* frag_end;           // [n_reads] the end key of the read's mapped primary, else SORT_KEY_LAST
    uint64_t* pair_a;             // [n_tmpl] the pair entry's two end keys in ascending order, else SORT_KEY_LAST both
    uint64_t* pair_b;
    int64_t* qual_off;            // [n_reads] QUAL of the mapped primary in bam ...
    int32_t* l_seq;               // ... and its length; 0 without one
    uint8_t* is_paired;           // [n_reads]
    int32_t* score;               // [n_reads]
    uint8_t* frag_dup;            // [n_reads] the fragment rule's verdict on the read's entry
    uint8_t* pair_dup;            // [n_tmpl] the pair rule's verdict
    int32_t* cnt;                 // [DUP_CNT_N]
};
