// kernels.h -- host-callable launchers of the HIP kernels (one translation unit per stage).
#pragma once
#include <hip/hip_runtime.h>
#include "bwamem_types.h"
#include "bam_encode.h"
#include "bam_sort.h"
#include "bam_dup.h"
#include "bam_qc.h"
#include "bam_baseqc.h"
#include "fastq_parse.h"
#include "bgzf_inflate.h"

void launch_build_occ64(hipStream_t st, const uint32_t* bwt, uint64_t n_blocks, uint4* occ);
// suffix array at every ix.sa_intv-th rank (lo/hi, (seq_len >> sa_shift) + 1 entries) from the image's sampling; *err: device int, OR-ed on failure
void launch_sa_densify(hipStream_t st, const DevIndex& ix, const uint64_t* sa_src, uint64_t n_src, int src_intv, uint32_t* lo, uint8_t* hi, int32_t* err);
void launch_encode(hipStream_t st, uint8_t* seq, int64_t n_bytes);
void launch_unpack_pac(hipStream_t st, const DevIndex& ix, int64_t start, int64_t n, uint8_t* dst);
void launch_seed(hipStream_t st, const DevIndex& ix, const MemOpt& opt, const TileView& tv);
// LDS plan of the persistent seeding grid (pure host arithmetic): the dynamic LDS one k_seed workgroup asks for, whether it
// stages its reads there, and how many workgroups go on a CU so that wpc * round_up(lds, granule) + reserve <= lds_per_cu.
// wpc is at least 1 (a reserve that one workgroup does not leave is cut down to what it leaves: `reserve` says what holds)
// and at most 16, the wave slots k_seed's registers allow.
struct SeedLdsPlan { size_t lds, reserve; int wpc; bool ldsq; };
SeedLdsPlan seed_lds_plan(size_t lds_per_cu, size_t granule, int max_len, bool narrow, int K, size_t reserve);
size_t scan_tmp_bytes(int64_t n);
void launch_scan(hipStream_t st, const int32_t* in, int64_t* out, int n, int64_t* tmp);   // tmp: scan_tmp_bytes(n), or null (one-workgroup form)
void launch_order(hipStream_t st, const int32_t* n_seeds, int n, int32_t* bins64, int32_t* order);   // TileView::order
size_t nul_tmp_bytes(int64_t n_bytes);
void launch_nul_offsets(hipStream_t st, const uint8_t* seq, int64_t n_bytes, int64_t* off, int64_t n_reads_max, int64_t* n_found, void* tmp);
void launch_sa(hipStream_t st, const DevIndex& ix, const MemOpt& opt, const TileView& tv, int64_t n_occ);
void launch_chain(hipStream_t st, const DevIndex& ix, const MemOpt& opt, const TileView& tv, Chain* chain_store);
// seed re-scoring (long reads): jobs/results sized by pe_rescue_bytes for `cap` >= the tile's seed count; first_num = 2 x n_reads ints, cnt = 1 int
bool rescore_needed(const MemOpt& opt, const TileView& tv);
void launch_rescore(hipStream_t st, const DevIndex& ix, const MemOpt& opt, const TileView& tv, void* jobs, void* results, int32_t* first_num, int32_t* cnt, int cap);
size_t extend_lds_bytes(const MemOpt& opt, int max_len);       // dynamic LDS k_extend asks for; the caller checks it against the device limit
void launch_extend(hipStream_t st, const DevIndex& ix, const MemOpt& opt, const TileView& tv);
void launch_post1(hipStream_t st, const DevIndex& ix, const MemOpt& opt, const TileView& tv);
void launch_final_prep(hipStream_t st, const DevIndex& ix, const MemOpt& opt, const TileView& tv);
size_t gcigar_slab_bytes(const MemOpt& opt, int max_len);      // traceback slab per resident workgroup of the wave form (long reads), 0 = none
int gcigar_slab_grid(const DevIndex& ix, int n_jobs);
void launch_gcigar(hipStream_t st, const DevIndex& ix, const MemOpt& opt, const TileView& tv, int n_jobs, const void* jobs, void* outs, uint32_t* cig_pool, int cig_cap,
                   uint8_t* zpool, unsigned long long zpool_cap, unsigned long long* zpool_cur, uint8_t* slabs, size_t slab_bytes, int* queue);
void launch_final_se(hipStream_t st, const DevIndex& ix, const MemOpt& opt, const TileView& tv, const void* job_out, const uint32_t* job_cig, int cig_cap);
void launch_pack(hipStream_t st, const TileView& tv, uint8_t* dst);
// BAM records of a tile's packed response (bam_encode.h): sizes per read, then -- after a launch_scan over the batch -- the records
void launch_bam_size(hipStream_t st, const BamTile& t);
void launch_bam_emit(hipStream_t st, const BamTile& t);
// With t.tags, both take the tagged forms, and the side text of SA / MC / MQ is made first: _tag_size for every tile of the batch
// (BamTagInfo and bytes per read), a launch_scan over the batch, then launch_bam_size; and _tag_text before launch_bam_emit
void launch_bam_tag_size(hipStream_t st, const BamTile& t);
void launch_bam_tag_text(hipStream_t st, const BamTile& t);
// Qualities and names of a batch: the qualities against the reads (a NUL where the read's is, else 33..126), and the names of the
// two reads of every pair against each other.  err: one int, zeroed by the caller; FASTQ_NO_ERROR - the smallest offending read
void launch_qual_check(hipStream_t st, const uint8_t* raw, const uint8_t* qual, const int64_t* raw_off, int n_reads, int32_t* err);
void launch_mate_names(hipStream_t st, const uint8_t* names, const int64_t* name_off, int n_pairs, int32_t* err);
// FASTQ text on the device (fastq_parse.h): _count the newlines of every chunk (fastq_n_chunks(n) ints), after a launch_scan
// _starts writes the line index, _records checks every record and writes its read's lengths (o.err: two ints, zeroed by the
// caller), and after two launch_scans _copy fills in bases, qualities and names (max_len: the longest read, o.err[1])
void launch_fastq_count(hipStream_t st, const uint8_t* text, int64_t n, int32_t* counts);
void launch_fastq_starts(hipStream_t st, const FastqText& t);
void launch_fastq_records(hipStream_t st, const FastqText& t, const FastqOut& o);
void launch_fastq_copy(hipStream_t st, const FastqText& t, const FastqOut& o, int max_len);
// BGZF members of src[0, n) (bgzf_deflate.h): member i of input [i * 0xff00, ...) into slots + i * BGZF_SLOT and its size into
// sizes[i], by `grid` = bgzf_grid(...) workgroups with bgzf_token_bytes(grid) of scratch; then -- after a launch_scan over the
// sizes -- the members packed into out at off[i], followed by the 28-byte EOF block at off[n_blocks] when asked for
int bgzf_grid(int n_cu, int64_t n_blocks);
size_t bgzf_token_bytes(int grid);
void launch_bgzf_deflate(hipStream_t st, const uint8_t* src, int64_t n, int n_blocks, int grid, uint8_t* slots, int32_t* sizes, uint32_t* tokens);
void launch_bgzf_gather(hipStream_t st, const uint8_t* slots, const int32_t* sizes, const int64_t* off, int n_blocks, bool with_eof, uint8_t* out);
// The reverse (bgzf_inflate.h): member m of the table mem[0, n_members) -- comp + coff, csize bytes -- inflated into text + uoff by one
// wavefront; comp is 16-byte aligned and padded by 16 bytes.  A refused member atomicMax-es BGZI_NO_ERROR - (member0 + m) into
// err[0] (zeroed by the caller)
void launch_bgzf_inflate(hipStream_t st, const uint8_t* comp, const BgzfMember* mem, int n_members, int member0, uint8_t* text, int32_t* err);
// Stable LSD radix sort of n (64-bit key, 32-bit index) pairs (bam_sort.h).  _bits: the OR / AND words of the keys into bits
// (SORT_BITS_N ints, zeroed by the caller; sort_live_bytes names the passes to run).  One pass over byte `byte`: _hist into hist
// (256 * sort_n_tiles(n) ints), launch_scan over them, _scatter from (keys, idx) to (keys_out, idx_out); idx == null: the identity.
void launch_sort_bits(hipStream_t st, const uint64_t* keys, int64_t n, int32_t* bits);
void launch_sort_hist(hipStream_t st, const uint64_t* keys, int64_t n, int byte, int32_t* hist);
void launch_sort_scatter(hipStream_t st, const uint64_t* keys, const uint32_t* idx, int64_t n, int byte, const int64_t* off, uint64_t* keys_out, uint32_t* idx_out);
// Coordinate-sorted records: _count the records of every read (and the OR / AND words of their keys), after a launch_scan _keys
// writes key, place and size of every record; after the sort _sizes permutes the sizes, and after their scan _gather copies the
// records to their places in dst (total bytes)
void launch_bamrec_count(hipStream_t st, const uint8_t* bam, const int64_t* bam_off, int n_reads, int32_t* counts, int32_t* bits, int32_t* err);
void launch_bamrec_keys(hipStream_t st, const uint8_t* bam, const int64_t* bam_off, int n_reads, const int64_t* first, uint64_t* keys, int64_t* src_off, int32_t* sizes);
void launch_bamrec_sizes(hipStream_t st, const uint32_t* idx, const int32_t* sizes, int n, int32_t* out);
void launch_bamrec_gather(hipStream_t st, const uint8_t* src, const int64_t* src_off, const uint32_t* idx, const int64_t* dst_off, int n_rec, int64_t total, uint8_t* dst);
// The BAI index: bin keys and windows per record; the chunk starts of the (refID, bin)-sorted list and -- after a launch_scan -- the
// chunks; the windows' first records as virtual offsets
void launch_bai_records(hipStream_t st, const BaiView& v);
void launch_bai_mark(hipStream_t st, const uint64_t* keys, const uint32_t* idx, int n, int32_t* start);
void launch_bai_chunks(hipStream_t st, const uint64_t* keys, const uint32_t* idx, int n, const int32_t* start, const int64_t* cid, const int64_t* rec_off,
                       const int64_t* member_off, int64_t coffset0, BaiChunk* out);
void launch_bai_windows(hipStream_t st, const int32_t* win, int n_win, int n_rec, const int64_t* rec_off, const int64_t* member_off, int64_t coffset0, uint64_t* out);
// Duplicate marking (bam_dup.h): _entries writes the keys, is_paired, the place of QUAL and the counts of every template (v.cnt
// zeroed by the caller); _scores the reads' scores (max_len: the longest QUAL, v.cnt[DUP_CNT_MAX_LEN]); _score_keys the first sort
// keys.  Between the sorts of a chain _gather takes the next key in the order of the last; after the last _decide writes the
// verdicts (dup zeroed by the caller), and _flags rewrites byte 19 of every record and counts the duplicates.
void launch_dup_entries(hipStream_t st, const DupView& v);
void launch_dup_scores(hipStream_t st, const DupView& v, int max_len);
void launch_dup_score_keys(hipStream_t st, const DupView& v, uint64_t* frag_key, uint64_t* pair_key);
void launch_dup_gather(hipStream_t st, const uint64_t* src, const uint32_t* idx, int n, uint64_t* out);
void launch_dup_decide(hipStream_t st, const uint64_t* keys, const uint32_t* idx, const uint64_t* second, int n, const uint8_t* is_paired, uint8_t* dup);
void launch_dup_flags(hipStream_t st, const DupView& v);
// Alignment QC (bam_qc.h): _records reduces everything but qual_hist into v.blk (zeroed by the caller) and leaves the errors in word
// QC_W_ERR and the longest primary read in QC_W_SUM + QC_S_MAX_LENGTH; when there is no error _qual adds qual_hist (max_len: that
// longest read).  Both run a fixed grid sized by the device's compute units.
void launch_qc_records(hipStream_t st, const QcView& v, int n_cu);
void launch_qc_qual(hipStream_t st, const QcView& v, int max_len, int n_cu);
// Base-level QC (bam_baseqc.h): _check does every check and leaves the errors in word BQ_W_ERR of v.blk (zeroed by the caller),
// records[], qcfail_skipped and the longest contributing read in BQ_W_MAX_LEN; when there is no error _bases and _aligned fill the
// tables (max_len: that longest read).  _gc_windows: windows[] of the whole index into v.out (zeroed by the caller).
void launch_bqc_check(hipStream_t st, const BqcView& v, int n_cu);
void launch_bqc_bases(hipStream_t st, const BqcView& v, int max_len, int n_cu);
void launch_bqc_aligned(hipStream_t st, const BqcView& v, int max_len, int n_cu);
void launch_gc_windows(hipStream_t st, const GcWinView& v, int n_cu);

// paired-end path (k_pe.hip)
void launch_pestat_cand(hipStream_t st, const DevIndex& ix, const MemOpt& opt, const TileView& tv, int8_t* cand_dir, int64_t* cand_is);
void launch_pe_caps(hipStream_t st, const MemOpt& opt, const TileView& tv, int32_t* caps);
void launch_pe_copy_regs(hipStream_t st, const TileView& tv, const AlnReg* src, const int64_t* src_off, AlnReg* dst, const int64_t* dst_off, const int32_t* n_regs);
void launch_pe_pair(hipStream_t st, const DevIndex& ix, const MemOpt& opt, const TileView& tv, AlnReg* regs, const int64_t* reg_off,
                    int32_t* n_regs, int32_t* ints, void* vpool, void* keys, uint8_t* scratch, int64_t scratch_per_pair, int cap_h, int cap_b, int cap_u, const MemPestat* pes, const PairTab& ptab, void* states,
                    void* rescue_jobs, void* rescue_res, int32_t* rescue_first, int32_t* rescue_num, int32_t* rescue_cnt, int rescue_cap);
size_t pe_rescue_bytes(int what, int cap);       // what = 0: SwJob[cap], 1: KswR[cap]
void launch_sw_jobs(hipStream_t st, const DevIndex& ix, const MemOpt& opt, const TileView& tv, const void* jobs, const int32_t* cnt, int cap, void* results, int cap_b, int max_qlen);
void launch_pe_out(hipStream_t st, const DevIndex& ix, const MemOpt& opt, const TileView& tv, AlnReg* regs, const int64_t* reg_off,
                   int32_t* n_regs, int32_t* ints, const MemPestat* pes, const void* states, const void* job_out, const uint32_t* job_cig, int cig_cap);
size_t pe_state_bytes(int n_reads);
