// bam_sort.h -- coordinate-sorted BAM and its BAI index on the device: the rules, and the helpers the kernels (k_post.hip, next
// to the BAM and BGZF kernels) share with the host (pipeline.cpp).  Plain C++ that compiles for the device, the emulation
// build and the host.
//
// Scope: one logical call (at most one jnibwa_createAlignments request, under 2 GiB of records) is sorted within itself.
// Merging the sorted runs of several calls is out of scope, and so are CSI indexes and the CG tag.
//
// The sort (launch_sort_*): a stable LSD radix sort of (64-bit key, 32-bit index) pairs with 8-bit digits.
//   tile          a workgroup of SORT_THREADS lanes owns SORT_TILE = SORT_THREADS * SORT_ITEMS consecutive elements; element
//                 j * SORT_THREADS + lane of the tile is item j of that lane, so the order of a tile is (item, wave, lane)
//   a pass        (1) the digit histogram of every tile, stored digit-major: hist[digit * n_tiles + tile]; (2) launch_scan over
//                 the 256 * n_tiles counts: the first output slot of every (digit, tile); (3) the scatter: the rank of an
//                 element among the equal digits of its tile is the count in earlier (item, wave) groups -- a table in LDS,
//                 each entry written by one lane, scanned per digit by one lane -- plus the count in earlier lanes of its own
//                 wave: the lanes with the same digit are the intersection of eight ballots, one per digit bit, and the rank
//                 is __popcll of that mask below the lane.  Every slot is written by exactly one lane.
//   skipped       a pass whose digit is the same for all keys moves nothing and is not run.  Which bytes vary is decided once,
//                 from the OR and the AND of the keys computed on the device (SortBits, sort_live_bytes): no read-back per
//                 pass.  The keys equal to SORT_KEY_LAST (all ones: an unplaced read) are all the same key, so they are left out
//                 of the OR / AND and one byte that separates them from every other key is added instead: with six contigs of
//                 less than 2^24 bases that is bytes 0..2 (pos), 4 (refID) and 7.
//   the result    a function of the input alone: ties keep input order, nothing depends on which lane or workgroup stores last.
//
// The sorted records (bwamem_hip_batch_sort_bam): the key of a record is (uint64)(uint32)refID << 32 | (uint32)pos, both
// read from the BAM record itself: an unplaced read (-1 / -1) sorts last, a placed unmapped mate at its mate's place; ties
// keep response order.  The records are found by walking each read's bytes along block_size (one lane per read), sorted as
// (key, record index), and gathered into a second buffer: every workgroup copies BAMSORT_CHUNK bytes of the destination whatever
// the sizes of the records in it, in dwords; a dword that straddles two records, and the tail, go byte by byte.
//
// The index (bwamem_hip_batch_index_bam), SAM specification 5.2, of the sorted and then compressed records:
//   virtual offset   of byte p of the record stream: (coffset0 + off[p / 0xff00]) << 16 | p % 0xff00, off = the n_blocks + 1 member
//                    offsets of the compressor, coffset0 = the file bytes in front of the first member (the compressed header)
//   header           magic "BAI\1", n_ref = the number of contigs
//   indexed records  those with refID >= 0; the interval is [pos, pos + span), span = the reference length of the record's own
//                    CIGAR (M, D, N, =, X), and 1 when that is 0 (a placed unmapped read has no CIGAR); the bin is the record's
//                    bin field.  A record that ends beyond 2^29 is an error.
//   bins             per reference in ascending bin number; a bin's chunks are the maximal runs of records at consecutive
//                    positions of the sorted stream that share (refID, bin), in file order, each (virtual offset of the first
//                    record's start, of the last record's end).  No pseudo-bin 37450.  The runs come from sorting
//                    (refID << 32 | bin, sorted index) with the same sort, marking the run starts, a scan and a compaction.
//   linear index     per reference n_intv = ((largest end - 1) >> 14) + 1, 0 without a record; the entry of a 16 384-base
//                    window is the start offset of the first record in file order that overlaps it (atomicMax of
//                    n_records - 1 - i per window: the smallest index); a window without a record takes the entry before it,
//                    or 0 when there is none
//   tail             n_no_coor (uint64) = the number of records with refID == -1
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SRT_HD static __host__ __device__ inline

enum { SORT_THREADS = 256, SORT_ITEMS = 8, SORT_TILE = SORT_THREADS * SORT_ITEMS, SORT_RADIX = 256 };
#define SORT_KEY_LAST 0xffffffffffffffffull

// OR / AND of the keys other than SORT_KEY_LAST, as int words the kernels OR into (the AND as the OR of the complements)
enum { SORT_BITS_OR_LO = 0, SORT_BITS_OR_HI, SORT_BITS_NAND_LO, SORT_BITS_NAND_HI, SORT_BITS_HAS_LAST, SORT_BITS_HAS_OTHER, SORT_BITS_N = 8 };

SRT_HD int64_t sort_n_tiles(int64_t n) { return (n + SORT_TILE - 1) / SORT_TILE; }
SRT_HD int sort_digit(uint64_t key, int byte) { return (int)(key >> (8 * byte) & 0xff); }

// one key into a lane's running words
SRT_HD void sort_bits_add(uint64_t key, int32_t* w /* [SORT_BITS_N] */)
{
    if (key == SORT_KEY_LAST) { w[SORT_BITS_HAS_LAST] = 1; return; }
    w[SORT_BITS_OR_LO] |= (int32_t)(uint32_t)key; w[SORT_BITS_OR_HI] |= (int32_t)(uint32_t)(key >> 32);
    w[SORT_BITS_NAND_LO] |= (int32_t)~(uint32_t)key; w[SORT_BITS_NAND_HI] |= (int32_t)~(uint32_t)(key >> 32);
    w[SORT_BITS_HAS_OTHER] = 1;
}

// The bytes (bit b = byte b of the key) whose passes must run.  Among the keys other than SORT_KEY_LAST a byte counts when
// some bit of it is set in one key and clear in another.  When SORT_KEY_LAST is present next to other keys, the highest byte
// in which no other key has 0xff (some bit is clear in all of them) is added: every other key is smaller there and not
// larger in the bytes above it that are sorted, so SORT_KEY_LAST lands behind them.  If there is no such byte, every byte
// that does not vary is 0xff in all keys, and the varying bytes alone order everything.
SRT_HD uint32_t sort_live_bytes(const int32_t* w /* [SORT_BITS_N] */)
{
    if (!w[SORT_BITS_HAS_OTHER]) return 0;
    const uint64_t o = (uint64_t)(uint32_t)w[SORT_BITS_OR_HI] << 32 | (uint32_t)w[SORT_BITS_OR_LO];
    const uint64_t a = ~((uint64_t)(uint32_t)w[SORT_BITS_NAND_HI] << 32 | (uint32_t)w[SORT_BITS_NAND_LO]);
    uint32_t live = 0;
    for (int b = 0; b < 8; ++b) if ((o ^ a) >> (8 * b) & 0xff) live |= 1u << b;
    if (w[SORT_BITS_HAS_LAST])
        for (int b = 7; b >= 0; --b) if ((o >> (8 * b) & 0xff) != 0xff) { live |= 1u << b; break; }
    return live;
}

// ---- BAM records as the sort and the index see them
enum { BAMSORT_ERR_WALK = 1,             // block_size values do not chain to the end of a read's bytes
       BAMSORT_ERR_END = 2,              // a record ends beyond 2^29
       BAMSORT_ERR_WINDOW = 4 };         // a record reaches beyond the windows of its contig
enum { BAMSORT_CHUNK = 16384,            // destination bytes per workgroup of the gather
       BAMSORT_MIN_REC = 36,             // bytes of the smallest record the walk accepts (block_size >= 32)
       BAMSORT_CHUNK_RECS = BAMSORT_CHUNK / BAMSORT_MIN_REC + 3,
       BAI_WINDOW_SHIFT = 14, BAI_MAX_END = 1 << 29 };

SRT_HD uint32_t bamsort_ld32(const uint8_t* p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
SRT_HD uint64_t bamsort_key(const uint8_t* rec) { return (uint64_t)bamsort_ld32(rec + 4) << 32 | bamsort_ld32(rec + 8); }
SRT_HD int64_t bai_n_windows(int64_t contig_len) { return (contig_len >> BAI_WINDOW_SHIFT) + 2; }

// the virtual offset of byte p of the record stream
SRT_HD uint64_t bai_voffset(const int64_t* member_off, int64_t coffset0, int64_t p)
{
    return (uint64_t)(coffset0 + member_off[p / 0xff00]) << 16 | (uint64_t)(p % 0xff00);
}

// one chunk of the index as the device leaves it: key = refID << 32 | bin (SORT_KEY_LAST: the run of unplaced records, dropped
// by the host)
struct BaiChunk { uint64_t key, beg, end; };

// what the per-record kernel of the index sees (k_post.hip: launch_bai_records)
struct BaiView {
    const uint8_t* bam;           // the sorted records ...
    const int64_t* rec_off;       // ... and their places, [n_rec + 1]
    int32_t n_rec, n_ref;
    const int32_t* win_base;      // [n_ref + 1]: the first window of every contig in win (bai_n_windows each)
    int32_t* win;                 // per window the largest n_rec - 1 - i of the records that overlap it, -1 = none
    uint64_t* keys;               // [n_rec] refID << 32 | bin, SORT_KEY_LAST for an unplaced record
    int32_t* n_no_coor;           // the number of unplaced records
    int32_t* err;                 // BAMSORT_ERR_* flags, OR-ed
};
