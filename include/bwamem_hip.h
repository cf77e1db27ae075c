/*
 * bwamem_hip.h -- C ABI of the MI355X-native BWA-MEM library (libbwamem_hip.so).
 *
 * The first block is the drop-in boundary: the same JNI-free entry points the reference's
 * JNI glue binds (reference: src/main/c/jnibwa.h:11-16, defined in src/main/c/jnibwa.c), with
 * identical argument meaning, ownership and error behaviour.  A maintainer of
 * broadinstitute/gatk-bwamem-jni links org_broadinstitute_hellbender_utils_bwa_BwaMemIndex.c
 * and init.c against this library instead of jnibwa.o + libbwa.a.
 * Handles are opaque; plain pointers and sizes only.
 */
#ifndef BWAMEM_HIP_H_
#define BWAMEM_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bwaidx_s bwaidx_t;      /* opaque; the jlong handle of BwaMemIndex.java:83 */
typedef struct mem_opt_s mem_opt_t;    /* 168 bytes, offsets pinned by BwaMemAligner.java:46-138 */
typedef struct mem_pestat_s mem_pestat_t; /* {int low, high, failed; double avg, std;}, 32 bytes x 4 orientations */

/* replaces bwa_idx_build() as called from ...BwaMemIndex.c:59 (declared, never defined, at jnibwa.h:11).
 * algo: "auto", "is", "rb2" select nothing here (one builder); any other name returns -1.  0 = ok. */
int jnibwa_createReferenceIndex(const char* refFileName, const char* indexPrefix, const char* algoName);

/* jnibwa.c:126-152: <prefix>.{amb,ann,bwt,pac,sa}[,alt] -> one contiguous image file.  0 ok, 2 I/O error. */
int jnibwa_createIndexFile(const char* refName, const char* imgName);

/* jnibwa.c:154-165: takes ownership of fd; mmaps the image read-only, uploads bwt/occ, SA and pac
 * to HBM.  Returns 0 on failure (Java then throws CouldNotReadImageException, BwaMemIndex.java:334). */
bwaidx_t* jnibwa_openIndex(int fd);

/* jnibwa.c:167-172 */
int jnibwa_destroyIndex(bwaidx_t* pIdx);

/* jnibwa.c:174-195: int32 n, then (int32 len, bytes) per contig; free with jnibwa_free */
void* jnibwa_getRefContigNames(bwaidx_t* pIdx, size_t* pBufSize);

/* jnibwa.c:197-235: pSeq = uint32 nSeqs + nSeqs NUL-terminated base strings (left untouched here; upstream
 * overwrites the bases with 0..4 codes, which Java never observes: BwaMemAligner.java:203-210); peStats = mem_pestat_t[4] or NULL (infer).  Returns a malloc'ed
 * int32 stream in the layout of ...BwaMemIndex.c:115-141, or NULL on any device error. */
void* jnibwa_createAlignments(bwaidx_t* pIdx, mem_opt_t* pOpts, mem_pestat_t* peStats, char* pSeq, size_t* pBufSize);

/* mem_opt_init() as wrapped at ...BwaMemIndex.c:89-92; free with jnibwa_free */
mem_opt_t* jnibwa_createDefaultOptions(void);

/* the one allocator behind destroyByteBuffer (...BwaMemIndex.c:157-160) */
void jnibwa_free(void* p);

/* ...BwaMemIndex.c:163-165 */
const char* jnibwa_getVersion(void);

/* ------------------------------------------------------------------------------------------------
 * Additive device-level entry points (bench, multi-GPU drivers).  Not part of the reference ABI. */

int bwamem_hip_set_device(int device);        /* indexes opened afterwards live on this one device (one process per GPU: bench.py's ranks) */
int bwamem_hip_device_count(void);
/* jnibwa_openIndex puts a replica of the index on every device named by BWAMEM_HIP_DEVICES ("all", or e.g. "0,1,2,3"; unset: the
 * device of bwamem_hip_set_device if that was called, else all visible devices); jnibwa_createAlignments (jnibwa.c:197-235: one
 * native call per batch) then cuts a large call across the replicas and sends small concurrent calls to them in turn.
 * -> the number of replicas behind the handle. */
int bwamem_hip_index_replicas(bwaidx_t* idx);

/* Tooling (bench.py --image): the contig lengths of an open index (returns the number of contigs; lens may be NULL), and
 * n bases of its packed reference from position start, one code 0..3 per byte, into DEVICE memory d_dst.  0 = ok. */
int bwamem_hip_index_contig_lengths(bwaidx_t* idx, int64_t* lens, int cap);
int bwamem_hip_index_unpack_pac(bwaidx_t* idx, int64_t start, int64_t n, void* d_dst);

/* Tooling (bench.py): an index image straight from base codes (0..3, one per byte, host memory) and a contig table, built on
 * the device (the same builder jnibwa_createReferenceIndex uses when a device is visible).  0 = ok. */
int bwamem_hip_build_image(const uint8_t* codes, int64_t l_pac, int32_t n_contigs, const char* const* names, const int64_t* lens, const char* img_path);

typedef struct bwamem_batch_s bwamem_batch_t; /* a request resident in HBM */

/* upload a request buffer (same wire format as pSeq above); the host buffer is left untouched */
bwamem_batch_t* bwamem_hip_batch_upload(bwaidx_t* idx, const char* pSeq, size_t nBytes);
/* the same for a payload that already lives in HBM: d_payload = the NUL-terminated base strings (without the
 * leading count), h_offsets = nReads+1 host offsets of the reads within it (h_offsets[nReads] = nBytes) */
bwamem_batch_t* bwamem_hip_batch_wrap_device(bwaidx_t* idx, const void* d_payload, size_t nBytes, uint32_t nReads, const int64_t* h_offsets);
/* run the whole hot path; results stay in HBM.  read_id0 = index of the first read within the
 * logical call (shards of one call must carry their global base index).  0 = ok. */
int bwamem_hip_batch_align(bwaidx_t* idx, const mem_opt_t* opt, const mem_pestat_t* pes, bwamem_batch_t* b, int64_t read_id0);
/* A paired-end call in two steps, for callers that shard ONE logical createAlignments call over several devices or
 * ranks (caveat 2).  With inferred insert-size statistics (pes == NULL at jnibwa.c:214) upstream's
 * mem_pestat is a reduction over all pairs of the call, between region finding and pairing; a shard must therefore
 * stop after phase 1, hand out its per-pair (orientation, insert size) candidates, and finish with the statistics
 * of the whole call:
 *   _pe_begin       phase 1 (seeding .. regions) of this shard's reads; opt must carry MEM_F_PE (0x2 at offset 60)
 *   _pe_candidates  n = pairs of the shard; dir[i] = orientation 0..3 or -1 (no candidate), isize[i] = insert size;
 *                   dir == NULL: just returns n
 *   bwamem_hip_pestat  upstream mem_pestat's reduction over candidates gathered from all shards (order-independent)
 *   _pe_finish      phase 2 (mate rescue, pairing, records) with those statistics; then download as usual
 * bwamem_hip_batch_align does the same in one call when the batch is the whole logical call. */
int bwamem_hip_batch_pe_begin(bwaidx_t* idx, const mem_opt_t* opt, bwamem_batch_t* b, int64_t read_id0);
size_t bwamem_hip_batch_pe_candidates(const bwamem_batch_t* b, int8_t* dir, int64_t* isize);
void bwamem_hip_pestat(const mem_opt_t* opt, const int8_t* dir, const int64_t* isize, size_t n, mem_pestat_t* pes /* [4] */);
int bwamem_hip_batch_pe_finish(bwaidx_t* idx, const mem_opt_t* opt, const mem_pestat_t* pes /* [4] */, bwamem_batch_t* b);
size_t bwamem_hip_batch_result_bytes(const bwamem_batch_t* b);
int bwamem_hip_batch_download(bwamem_batch_t* b, void* dst);
void bwamem_hip_batch_free(bwamem_batch_t* b);

/* SAM text on the native side (additive).  pSeq = the request handed to jnibwa_createAlignments,
 * response = what it returned.  One line per record, layout described in csrc/sam_writer.cpp; readNames = nSeqs names or NULL
 * ("r<index>", paired: "p<pair index>"); paired = the call carried MEM_F_PE.  Both return malloc'ed, NUL-terminated text (free
 * with jnibwa_free) or NULL when the response does not parse against the request. */
char* bwamem_hip_sam_header(bwaidx_t* idx, size_t* pBytes);
char* bwamem_hip_response_to_sam(bwaidx_t* idx, const char* pSeq, const void* response, size_t responseBytes, const char* const* readNames, int paired, size_t* pBytes);

/* BAM on the native side (additive).  The records are encoded on the device, straight from the results
 * resident after bwamem_hip_batch_align / _pe_finish; the host only frames BGZF.  A BAM record decodes to exactly the SAM
 * line bwamem_hip_response_to_sam writes for the same response record (rules: csrc/bam_encode.h).
 *   _keep_offsets   before _align / _pe_begin: keep each tile's per-read offsets (8 bytes per read) for the encoder.  Off by
 *                   default, and then the align path allocates and computes exactly what it did without this block.
 *   _encode_bam     uncompressed BAM alignment records (block_size-prefixed, SAM spec 4.2) in response order, into a device
 *                   buffer owned by the batch.  paired = the call carried MEM_F_PE.  names = all names back to back (host
 *                   memory), name_off = nReads + 1 offsets into it, each name 1..254 bytes; or both NULL: "r<index>",
 *                   paired "p<pair index>", the index counted from read_id0 of the align call.  An odd trailing read of a
 *                   paired call has no record.  Non-zero on error: no offsets kept, no finished alignment, a bad name, or a
 *                   record with more than 65 535 CIGAR operations (the CG-tag convention is not implemented); nothing is
 *                   produced then.
 *   _bam_bytes / _bam_download   size of those records, and their copy to host memory
 *   bwamem_hip_bam_header        the uncompressed BAM header: magic, the text of bwamem_hip_sam_header, the contig table
 *   bwamem_hip_bgzf_compress     BGZF blocks (at most 0xff00 input bytes each) by n_threads workers (<= 0 or more than 16:
 *                   16), with_eof: followed by the 28-byte EOF block.  level 0 = stored blocks, always available; levels
 *                   1..9 need libz.so.1 at run time (NULL without it).  The result does not depend on n_threads.
 *   bwamem_hip_align_to_bam      upload, align, encode, download, BGZF, write(fd): the header first when write_header is set, the
 *                   EOF block always last.  readNames = nSeqs names or NULL.  0 = ok.
 *   bwamem_hip_bam_record_bytes  tooling: the size of the BAM record of one response record (rec: n_words int32 words starting at
 *                   its flag/mapq word; k = its index within the read, l_read / l_name = lengths of the read and its name), or
 *                   a negative error (-1: more than 65 535 CIGAR operations, -2: does not parse). */
int    bwamem_hip_batch_keep_offsets(bwamem_batch_t* b, int on);
int    bwamem_hip_batch_encode_bam(bwamem_batch_t* b, int paired, const char* names, const int64_t* name_off);
size_t bwamem_hip_batch_bam_bytes(const bwamem_batch_t* b);
int    bwamem_hip_batch_bam_download(bwamem_batch_t* b, void* dst);
void*  bwamem_hip_bam_header(bwaidx_t* idx, size_t* pBytes);                 /* jnibwa_free */
void*  bwamem_hip_bgzf_compress(const void* src, size_t n, int level, int n_threads, int with_eof, size_t* pBytes);   /* jnibwa_free */
int    bwamem_hip_align_to_bam(bwaidx_t* idx, const mem_opt_t* opt, const mem_pestat_t* pes, const char* pSeq, size_t nBytes,
                               const char* const* readNames, int level, int fd, int write_header);
int64_t bwamem_hip_bam_record_bytes(const void* rec, size_t n_words, int k, int32_t l_read, int32_t l_name);

/* BGZF on the device (csrc/bgzf_deflate.h; additive): the members are compressed by HIP kernels -- LZ77 matching, dynamic Huffman
 * codes, CRC-32 -- one workgroup per block of at most 0xff00 input bytes, so only compressed bytes cross to the host, libz is not
 * needed and no host thread compresses.  The bytes are a function of the input alone.
 *   _compress_bam   after _encode_bam: the BGZF members of the records (with_eof: followed by the EOF block), in a device buffer
 *                   owned by the batch.  Non-zero (and 0 bytes) without encoded records.  _encode_bam and a new alignment of
 *                   the batch discard the members.
 *   _bgzf_bytes / _bgzf_download   their size, and their copy to host memory
 *   bwamem_hip_bgzf_compress_device   host bytes in, BGZF out (jnibwa_free): upload, the same kernels, download; idx selects the device
 *   bwamem_hip_align_to_bam_device    bwamem_hip_align_to_bam with the header block and the records compressed on the device */
int    bwamem_hip_batch_compress_bam(bwamem_batch_t* b, int with_eof);
size_t bwamem_hip_batch_bgzf_bytes(const bwamem_batch_t* b);
int    bwamem_hip_batch_bgzf_download(bwamem_batch_t* b, void* dst);
void*  bwamem_hip_bgzf_compress_device(bwaidx_t* idx, const void* src, size_t n, int with_eof, size_t* pBytes);
int    bwamem_hip_align_to_bam_device(bwaidx_t* idx, const mem_opt_t* opt, const mem_pestat_t* pes, const char* pSeq, size_t nBytes,
                                      const char* const* readNames, int fd, int write_header);

/* Coordinate-sorted BAM and its BAI index, sorted and indexed on the device (csrc/bam_sort.h; additive): while the records sit in
 * HBM next to the compressor they are sorted by (refID, pos) -- a stable radix sort of 8-byte keys and one gather -- and the index
 * is made where both the records' places and the members' offsets are known.  Sorted means sorted within the call (one
 * jnibwa_createAlignments request, under 2 GiB of records); merging the sorted runs of several calls is the caller's business.
 *   _sort_bam       after _encode_bam: the records ordered by (uint32)refID, then (uint32)pos, both read from the records -- unplaced
 *                   reads last, a placed unmapped mate at its mate's place, ties in response order.  From here _bam_bytes,
 *                   _bam_download and _compress_bam see the sorted records.  Non-zero, and the records as they were, without encoded
 *                   records; 0 and nothing done when they are sorted already.  Discards BGZF members; _encode_bam and a new
 *                   alignment of the batch discard the sorted state.
 *   _index_bam      after _sort_bam and then _compress_bam: the bytes of the .bai file (jnibwa_free) for a BAM file in which
 *                   coffset0 bytes (the compressed header) precede the first member of the records; the rules are at the top of
 *                   csrc/bam_sort.h.  NULL with a message when the batch is not sorted, has no members, or a record ends beyond
 *                   2^29.  A sorted batch without records gives the empty index.
 *   bwamem_hip_bam_header_sorted     bwamem_hip_bam_header with the first line "@HD\tVN:1.6\tSO:coordinate"
 *   bwamem_hip_align_to_sorted_bam   bwamem_hip_align_to_bam_device with _sort_bam between encode and compress and the sorted
 *                   header; fd_bai >= 0: the index is written there as well, which needs write_header (otherwise an error, and
 *                   nothing is written)
 *   bwamem_hip_sort_pairs_device     tooling: host keys in, the stable sorting permutation out (perm[i] = the index of the i-th
 *                   smallest key, ties in input order), through the same kernels; idx selects the device.  0 = ok. */
int    bwamem_hip_batch_sort_bam(bwamem_batch_t* b);
void*  bwamem_hip_batch_index_bam(bwamem_batch_t* b, int64_t coffset0, size_t* pBytes);   /* jnibwa_free */
void*  bwamem_hip_bam_header_sorted(bwaidx_t* idx, size_t* pBytes);                        /* jnibwa_free */
int    bwamem_hip_align_to_sorted_bam(bwaidx_t* idx, const mem_opt_t* opt, const mem_pestat_t* pes, const char* pSeq, size_t nBytes,
                                      const char* const* readNames, int fd, int fd_bai, int write_header);
int    bwamem_hip_sort_pairs_device(bwaidx_t* idx, const uint64_t* keys, size_t n, uint32_t* perm);

/* FASTQ in, base qualities and read groups out (csrc/fastq_parse.h, csrc/bam_encode.h; additive).  Qualities and read names never
 * touch the alignment; they only have to be resident when the records are written.  So FASTQ text is uploaded as it is and taken
 * apart by HIP kernels -- a line index, one lane per record to check it, a copy -- and the host never looks at its bytes.  Without
 * qualities, a read group or a FASTQ call every entry point above produces byte for byte what it did.
 *   _set_qualities  before _encode_bam: quals = nReads NUL-terminated Phred+33 strings in request order (host memory), the string of
 *                   read i exactly as long as read i, nBytes = their size -- the layout of the request's payload.  Checked on the
 *                   device (a NUL where each read's NUL is, every other byte in 33..126); non-zero with a message otherwise, and the
 *                   batch keeps the qualities it had.  quals == NULL removes them.  QUAL of a record: csrc/bam_encode.h.
 *   _set_read_group before _encode_bam: rg_line = one header line without its newline; it must begin with "@RG\t", contain an ID:
 *                   field of 1..254 bytes and no '\n' or '\r'; non-zero otherwise.  Every record, unmapped ones included, then ends
 *                   with the tag RG:Z:<ID> (after XA).  NULL removes the read group.
 *   bwamem_hip_bam_header_rg / bwamem_hip_sam_header_rg   bwamem_hip_bam_header (sorted != 0: _sorted) / bwamem_hip_sam_header with
 *                   rg_line after the last @SQ line (NULL: the header as it is); NULL when the line is refused.  jnibwa_free.
 *   bwamem_hip_response_to_sam_q   bwamem_hip_response_to_sam with the qualities (the format above, or NULL: '*') and a read group's
 *                   ID (or NULL: no tag).  A BAM record decodes to exactly this line, QUAL and RG:Z included.
 *   _upload_fastq   a batch from FASTQ text (rules: csrc/fastq_parse.h -- four lines per record, "\n" or "\r\n", names up to the first
 *                   blank with a trailing /1 or /2 removed).  text2 == NULL: single-end reads or one interleaved file (the paired flag
 *                   of _encode_bam decides); with both texts read 2i comes from text1 and read 2i + 1 from text2, and their names must
 *                   be equal.  The batch holds the payload and offsets bwamem_hip_batch_upload would have built from the same reads,
 *                   the reads' names and their qualities: _encode_bam(b, paired, NULL, NULL) then writes those names instead of
 *                   "r<index>" (paired: the names of the two reads of a pair must be equal, else non-zero).  Malformed input: NULL
 *                   with a message, and *bad_record = the smallest index of an offending read (see fastq_parse.h), or -1 for errors
 *                   of no single record (a line count that is no multiple of four, unequal record counts).
 *   bwamem_hip_align_fastq_to_bam   upload_fastq, align, encode, sort if asked, compress on the device, index if fd_bai >= 0 (needs
 *                   sort and write_header), write; rg_line (or NULL) goes into the header and onto every record.  0 = ok. */
int    bwamem_hip_batch_set_qualities(bwamem_batch_t* b, const char* quals, size_t nBytes);
int    bwamem_hip_batch_set_read_group(bwamem_batch_t* b, const char* rg_line);
void*  bwamem_hip_bam_header_rg(bwaidx_t* idx, int sorted, const char* rg_line, size_t* pBytes);   /* jnibwa_free */
char*  bwamem_hip_sam_header_rg(bwaidx_t* idx, const char* rg_line, size_t* pBytes);               /* jnibwa_free */
char*  bwamem_hip_response_to_sam_q(bwaidx_t* idx, const char* pSeq, const void* response, size_t responseBytes, const char* const* readNames, int paired,
                                    const char* quals, const char* rgId, size_t* pBytes);
bwamem_batch_t* bwamem_hip_batch_upload_fastq(bwaidx_t* idx, const char* text1, size_t n1, const char* text2, size_t n2, int64_t* bad_record);
int    bwamem_hip_align_fastq_to_bam(bwaidx_t* idx, const mem_opt_t* opt, const mem_pestat_t* pes, const char* text1, size_t n1, const char* text2, size_t n2,
                                     const char* rg_line, int sort, int fd, int fd_bai, int write_header);

/* Duplicates marked on the device, before the sort (csrc/bam_dup.h; additive).  Between _encode_bam and _sort_bam the records of a
 * read are contiguous and the two reads of a pair are neighbours, so marking is a few sorts of 8-byte keys and one flag byte per
 * record: it changes no record's size, place or sort key, and the sort, the compressor and the index do not know about it.  The
 * rule -- Picard MarkDuplicates' as documented, one library, no optical duplicates -- is at the top of csrc/bam_dup.h and is defined
 * on the records alone; parity with Picard's own output is not checked anywhere.  One call is marked within itself: duplicates
 * across calls are the caller's business, like merging the sorted runs.
 *   _mark_duplicates   after _encode_bam and before _sort_bam: sets 0x400 on every record of a duplicate template and clears it on
 *                   every other record (paired: reads 2i and 2i + 1 are a template, as for _encode_bam); counts (or NULL) receives
 *                   the six totals.  Non-zero with a message, and the records as they were, without encoded records or when the
 *                   batch is sorted already (the records are then no longer grouped by read).  0 with zero counts on a batch
 *                   without records.  Discards BGZF members; _encode_bam and a new alignment discard the marks with the records.
 *   bwamem_hip_mark_duplicates_device   tooling: host records grouped by read (read_off: nReads + 1 ascending offsets, the first
 *                   0 and the last nBytes) are uploaded, marked by the same kernels and handed back in place; idx selects the
 *                   device.  0 = ok; non-zero, and the records untouched, when they do not parse.
 *   bwamem_hip_align_to_marked_bam / bwamem_hip_align_fastq_to_marked_bam   bwamem_hip_align_to_sorted_bam (with `sort`: 0 leaves
 *                   response order and the plain header) / bwamem_hip_align_fastq_to_bam with _mark_duplicates between encode and
 *                   sort; fd_bai >= 0 needs sort and write_header. */
typedef struct {
    uint64_t unpaired_reads_examined, read_pairs_examined, secondary_or_supplementary, unmapped_reads, unpaired_read_duplicates, read_pair_duplicates;
} bwamem_dup_counts_t;
int    bwamem_hip_batch_mark_duplicates(bwamem_batch_t* b, int paired, bwamem_dup_counts_t* counts);
int    bwamem_hip_mark_duplicates_device(bwaidx_t* idx, void* records, size_t nBytes, const int64_t* read_off, size_t nReads, int paired,
                                         bwamem_dup_counts_t* counts);
int    bwamem_hip_align_to_marked_bam(bwaidx_t* idx, const mem_opt_t* opt, const mem_pestat_t* pes, const char* pSeq, size_t nBytes,
                                      const char* const* readNames, int sort, int fd, int fd_bai, int write_header, bwamem_dup_counts_t* counts);
int    bwamem_hip_align_fastq_to_marked_bam(bwaidx_t* idx, const mem_opt_t* opt, const mem_pestat_t* pes, const char* text1, size_t n1, const char* text2,
                                            size_t n2, const char* rg_line, int sort, int fd, int fd_bai, int write_header, bwamem_dup_counts_t* counts);

/* Compressed FASTQ in (csrc/bgzf_inflate.h; additive): .fastq.gz bytes are taken as they are.  A BGZF stream -- what bgzip and this
 * library's own compressor write: independent gzip members of at most 64 KiB of text -- is uploaded compressed and inflated in HBM,
 * one wavefront per member; the host only walks the member headers, and the parse kernels of _upload_fastq run on the resident
 * text.  A plain gzip stream (what gzip writes: no member sizes, nothing to cut) is inflated on the host through libz.so.1, loaded
 * at run time, and its text takes the plain-text path; without that library such a stream is refused with a message that says to
 * use bgzip.  The first member decides a stream's kind; the two streams of a call may differ in kind.  With BWAMEM_HIP_VERBOSE a
 * line per stream says which way it went.
 *   bwamem_hip_bgzf_inflate_device   host bytes in, inflated bytes out (jnibwa_free): the counterpart of
 *                   bwamem_hip_bgzf_compress_device; idx selects the device.  BGZF only.  The empty stream gives zero bytes (not
 *                   NULL).  NULL with *bad_member = the smallest offending member (-1 for errors of no single member: not BGZF,
 *                   2 GiB of text or more) when the stream is refused: the rules are at the top of csrc/bgzf_inflate.h, and what
 *                   they accept and refuse is what zlib accepts and refuses.
 *   _upload_fastq_gz   exactly the batch _upload_fastq yields for the inflated texts -- payload, offsets, names, qualities, and
 *                   *bad_record for malformed FASTQ inside good members; lines and records may straddle members anywhere.  gz2 ==
 *                   NULL: one stream.  *bad_member counts the members of the first stream, then of the second (-1: none, or a
 *                   damaged plain gzip stream).  "One request under 2 GiB" holds for the inflated texts and is checked before
 *                   anything is uploaded.
 *   bwamem_hip_align_fastq_gz_to_marked_bam   bwamem_hip_align_fastq_to_marked_bam with the texts replaced by such streams;
 *                   mark_dup == 0 leaves the marking out (counts, when given, is zeroed): bwamem_hip_align_fastq_to_bam. */
void*  bwamem_hip_bgzf_inflate_device(bwaidx_t* idx, const void* src, size_t n, size_t* pBytes, int64_t* bad_member);      /* jnibwa_free */
bwamem_batch_t* bwamem_hip_batch_upload_fastq_gz(bwaidx_t* idx, const void* gz1, size_t n1, const void* gz2, size_t n2, int64_t* bad_record,
                                                 int64_t* bad_member);
int    bwamem_hip_align_fastq_gz_to_marked_bam(bwaidx_t* idx, const mem_opt_t* opt, const mem_pestat_t* pes, const void* gz1, size_t n1, const void* gz2,
                                               size_t n2, const char* rg_line, int sort, int fd, int fd_bai, int write_header, int mark_dup,
                                               bwamem_dup_counts_t* counts);

/* SA, MC and MQ tags, built on the device (csrc/bam_encode.h, "SA, MC, MQ"; additive and off by default: with no tag asked for
 * every entry point above produces byte for byte what it did).  SA:Z links the records of a chimeric read; MC:Z and MQ:i are the
 * mate's CIGAR and mapping quality, what samtools fixmate adds.  All three are defined on the response alone.  The text of other
 * records comes from a per-read side buffer that kernels next to the encoder fill (sizes, a scan, the text) from the resident
 * response and the index's contig names, so the tags cost no transfer and no host pass; the tag order on a record is
 * NM MD AS XS XA SA MC MQ RG.  Mark-duplicates, the sort, the compressor and the index see larger records and nothing else.
 *   _set_tags       before _encode_bam: mask = BWAMEM_HIP_TAG_* OR-ed; 0 removes the tags.  Unknown bits: non-zero with a message,
 *                   and the batch keeps the mask it had.  A new alignment keeps the mask, as it keeps the read group.  MC and MQ
 *                   need the mate, so an unpaired _encode_bam ignores those two bits.
 *   bwamem_hip_response_to_sam_tags   bwamem_hip_response_to_sam_q plus the tags named by `tags`, written by host code of its own from
 *                   the response.  A BAM record decodes to exactly this line, SA, MC and MQ included.
 *   bwamem_hip_fastq_to_bam   the one-call entry point with its choices in a struct: plain or compressed FASTQ (a stream that begins
 *                   with 1f 8b is taken as compressed: BGZF or plain gzip as for _upload_fastq_gz) through align, encode with
 *                   o->tags, mark (o->mark_dup; counts as for bwamem_hip_align_fastq_gz_to_marked_bam), sort (o->sort), compress and
 *                   index on the device (fd_bai >= 0 needs sort and write_header).  o->size = sizeof(bwamem_bam_options_t) as the
 *                   caller compiled it: fields beyond it take their zero defaults, and a size this library does not know is
 *                   refused.  o == NULL: every field zero. */
enum { BWAMEM_HIP_TAG_SA = 1, BWAMEM_HIP_TAG_MC = 2, BWAMEM_HIP_TAG_MQ = 4 };
typedef struct {
    size_t size;                /* sizeof(bwamem_bam_options_t) */
    const char* rg_line;        /* as for _set_read_group, or NULL */
    int sort, mark_dup;
    unsigned tags;              /* BWAMEM_HIP_TAG_* */
    int write_header;
} bwamem_bam_options_t;
int    bwamem_hip_batch_set_tags(bwamem_batch_t* b, unsigned mask);
char*  bwamem_hip_response_to_sam_tags(bwaidx_t* idx, const char* pSeq, const void* response, size_t responseBytes, const char* const* readNames, int paired,
                                       const char* quals, const char* rgId, unsigned tags, size_t* pBytes);
int    bwamem_hip_fastq_to_bam(bwaidx_t* idx, const mem_opt_t* opt, const mem_pestat_t* pes, const void* in1, size_t n1, const void* in2, size_t n2,
                               const bwamem_bam_options_t* o, int fd, int fd_bai, bwamem_dup_counts_t* counts);

/* Alignment QC on the device (csrc/bam_qc.h; additive: without a QC object every entry point above writes byte for byte what it
 * did).  flagstat, idxstats, the summary numbers of `samtools stats` and the insert-size metrics of Picard, as a reduction over the
 * BAM records of a batch while they are in HBM.  The rule is at the top of csrc/bam_qc.h and is defined on the records alone; parity
 * with the output of samtools or Picard is not checked anywhere.  A bwamem_qc_t is an accumulator in host memory: it adds up any
 * number of calls, batches on any replica of the handle, and the serialized accumulators of other devices, ranks or runs.  A call
 * that fails leaves it exactly as it was.
 *   _qc_create      an empty accumulator for the contigs (names, lengths) of idx; idx must outlive it for _qc_add_records_device.
 *   _qc_add_batch   after _encode_bam; after _mark_duplicates to see 0x400; before or after _sort_bam (the result is the same).
 *                   Non-zero with a message without encoded records, for a batch of an index with another contig count, or when a
 *                   record does not parse.  0 and nothing added for a batch without records.
 *   _qc_add_records_device   tooling: host bytes, any stream of BAM records (block_size and body, no header), uploaded and reduced
 *                   by the same kernels on the device of the accumulator's index.
 *   _qc_counts      the counters; _qc_array: one array (BWAMEM_HIP_QC_*) into dst[0, cap), returns its length (dst may be NULL),
 *                   -1 for an unknown array.
 *   _qc_serialize   the accumulator as bytes (jnibwa_free): four 64-bit words -- a magic, the version, n_contigs, the word count --
 *                   and the words.  _qc_add_serialized adds such a blob; it refuses another version or n_contigs, and then changes
 *                   nothing.
 *   _qc_report      plain text, '\n' line ends, NUL-terminated (jnibwa_free); *pBytes without the NUL.  _FLAGSTAT: the sixteen lines of
 *                   samtools flagstat; _IDXSTATS: name, length, mapped, unmapped per contig and the '*' line; _SUMMARY: key<TAB>value
 *                   for every single counter and the derived numbers; _INSERT_SIZE: the metrics per orientation and the histogram.
 *                   The formats are in csrc/sam_writer.cpp.
 *   bwamem_hip_fastq_to_bam_qc   bwamem_hip_fastq_to_bam with the batch added to qc after mark-duplicates (when asked for) and
 *                   before the sort -- only if the whole call returns 0.  qc == NULL: bwamem_hip_fastq_to_bam. */
typedef struct bwamem_qc_s bwamem_qc_t;
typedef struct {
    uint64_t total[2], primary[2], secondary[2], supplementary[2], duplicates[2], primary_duplicates[2], mapped[2], primary_mapped[2], paired[2], read1[2], read2[2],
             properly_paired[2], both_mapped[2], singletons[2], mate_diff_chr[2], mate_diff_chr_mapq5[2];       /* [0] QC-passed, [1] QC-failed (0x200) */
    uint64_t unplaced, sequences, total_length, max_length, reads_mq0, bases_mapped, bases_mapped_cigar, bases_soft_clipped, ins_events, ins_bases, del_events,
             del_bases, mismatches, records_without_nm;
    uint64_t isize_min[3], isize_max[3];        /* FR, RF, TANDEM; UINT32_MAX and 0 when empty */
} bwamem_qc_counts_t;
enum { BWAMEM_HIP_QC_MAPQ = 0, BWAMEM_HIP_QC_QUAL, BWAMEM_HIP_QC_ISIZE_FR, BWAMEM_HIP_QC_ISIZE_RF, BWAMEM_HIP_QC_ISIZE_TANDEM, BWAMEM_HIP_QC_CONTIG_MAPPED,
       BWAMEM_HIP_QC_CONTIG_UNMAPPED };
enum { BWAMEM_HIP_QC_FLAGSTAT = 0, BWAMEM_HIP_QC_IDXSTATS, BWAMEM_HIP_QC_SUMMARY, BWAMEM_HIP_QC_INSERT_SIZE };
bwamem_qc_t* bwamem_hip_qc_create(bwaidx_t* idx);
void   bwamem_hip_qc_free(bwamem_qc_t* q);
int    bwamem_hip_qc_add_batch(bwamem_qc_t* q, bwamem_batch_t* b);
int    bwamem_hip_qc_add_records_device(bwamem_qc_t* q, const void* records, size_t nBytes);
int    bwamem_hip_qc_counts(const bwamem_qc_t* q, bwamem_qc_counts_t* out);
int64_t bwamem_hip_qc_array(const bwamem_qc_t* q, int which, uint64_t* dst, size_t cap);
void*  bwamem_hip_qc_serialize(const bwamem_qc_t* q, size_t* pBytes);                      /* jnibwa_free */
int    bwamem_hip_qc_add_serialized(bwamem_qc_t* q, const void* blob, size_t n);
char*  bwamem_hip_qc_report(const bwamem_qc_t* q, int kind, size_t* pBytes);               /* jnibwa_free */
int    bwamem_hip_fastq_to_bam_qc(bwaidx_t* idx, const mem_opt_t* opt, const mem_pestat_t* pes, const void* in1, size_t n1, const void* in2, size_t n2,
                                  const bwamem_bam_options_t* o, int fd, int fd_bai, bwamem_dup_counts_t* counts, bwamem_qc_t* qc);

/* Base-level QC on the device (csrc/bam_baseqc.h; additive like the QC above, and apart from it: bwamem_qc_t, its blob and its reports
 * are what they were).  Quality, base composition, mismatches, insertions, deletions and soft clips per sequencing cycle and end, the
 * reads' GC histograms, and GC bias over 100-base reference windows: what Picard MeanQualityByCycle, BaseDistributionByCycle and
 * CollectGcBiasMetrics and the mismatch / indel / GC sections of `samtools stats` report, as a reduction over the records of a batch in
 * HBM against the resident packed reference (no MD parsing, no FASTA).  The rule is at the top of csrc/bam_baseqc.h; parity with the
 * output of those tools is not checked anywhere.  A bwamem_baseqc_t adds up calls, replicas and serialized accumulators like a
 * bwamem_qc_t; a call that fails leaves it exactly as it was.
 *   _baseqc_create     an empty accumulator for idx, which must outlive it.
 *   _baseqc_add_batch  after _encode_bam; before or after _mark_duplicates and _sort_bam, with the same result.  Non-zero with a
 *                      message without encoded records, for a batch of an index with another contig count, or when a record is refused
 *                      (it does not parse; a mapped primary's CIGAR does not cover l_seq or has an inner H; it lies outside its
 *                      contig).  0 and nothing added for a batch without records.
 *   _baseqc_add_records_device   tooling: host bytes, any stream of BAM records, uploaded and reduced by the same kernels.
 *   _baseqc_counts     the counters; _baseqc_array: one table (BWAMEM_HIP_BASEQC_*) into dst[0, cap), returns its length (dst may be
 *                      NULL), -1 for an unknown table.  A table [e][c] has 3 x 1024 words, end e (0 unpaired or neither, 1 first, 2
 *                      second) times cycle c, flattened in that order; _BASE is [e][c][k], k = A C G T N; _READ_GC is [e][101]; the
 *                      _GCB_* have 101 words, one per GC count of the window.
 *   _baseqc_serialize  as _qc_serialize (another magic); _baseqc_add_serialized refuses another version, n_contigs or size and then
 *                      changes nothing.  windows[] is a property of the index and not part of the blob.
 *   _baseqc_report     plain text as _qc_report.  _CYCLES: per end with records a header and one row per cycle up to the last non-zero
 *                      one; _GC: per GC count the windows, the reads, the normalized coverage and the mean base quality, then the
 *                      reads' GC histograms.  The formats are in csrc/sam_writer.cpp.
 *   bwamem_hip_index_gc_windows   windows[g]: the number of 100-base windows of the index, over all contigs, that touch no .amb hole and
 *                      hold g C/G bases (the denominator of GC bias); computed on the device once per handle.
 *   bwamem_hip_fastq_to_bam_metrics   bwamem_hip_fastq_to_bam_qc with the batch also added to bq, at the same point and only if the whole
 *                      call returns 0.  Either accumulator may be NULL. */
typedef struct bwamem_baseqc_s bwamem_baseqc_t;
typedef struct { uint64_t records[3], qcfail_skipped, gcb_skipped; } bwamem_baseqc_counts_t;
enum { BWAMEM_HIP_BASEQC_BASE = 0, BWAMEM_HIP_BASEQC_QUAL_SUM, BWAMEM_HIP_BASEQC_QUAL_N, BWAMEM_HIP_BASEQC_ALIGNED, BWAMEM_HIP_BASEQC_MISM, BWAMEM_HIP_BASEQC_INS,
       BWAMEM_HIP_BASEQC_DEL, BWAMEM_HIP_BASEQC_SOFT, BWAMEM_HIP_BASEQC_READ_GC, BWAMEM_HIP_BASEQC_GCB_READS, BWAMEM_HIP_BASEQC_GCB_QUAL_SUM,
       BWAMEM_HIP_BASEQC_GCB_QUAL_N };
enum { BWAMEM_HIP_BASEQC_CYCLES = 0, BWAMEM_HIP_BASEQC_GC };
bwamem_baseqc_t* bwamem_hip_baseqc_create(bwaidx_t* idx);
void   bwamem_hip_baseqc_free(bwamem_baseqc_t* q);
int    bwamem_hip_baseqc_add_batch(bwamem_baseqc_t* q, bwamem_batch_t* b);
int    bwamem_hip_baseqc_add_records_device(bwamem_baseqc_t* q, const void* records, size_t nBytes);
int    bwamem_hip_baseqc_counts(const bwamem_baseqc_t* q, bwamem_baseqc_counts_t* out);
int64_t bwamem_hip_baseqc_array(const bwamem_baseqc_t* q, int which, uint64_t* dst, size_t cap);
void*  bwamem_hip_baseqc_serialize(const bwamem_baseqc_t* q, size_t* pBytes);              /* jnibwa_free */
int    bwamem_hip_baseqc_add_serialized(bwamem_baseqc_t* q, const void* blob, size_t n);
char*  bwamem_hip_baseqc_report(const bwamem_baseqc_t* q, int kind, size_t* pBytes);       /* jnibwa_free */
int    bwamem_hip_index_gc_windows(bwaidx_t* idx, uint64_t out[101]);
int    bwamem_hip_fastq_to_bam_metrics(bwaidx_t* idx, const mem_opt_t* opt, const mem_pestat_t* pes, const void* in1, size_t n1, const void* in2, size_t n2,
                                       const bwamem_bam_options_t* o, int fd, int fd_bai, bwamem_dup_counts_t* counts, bwamem_qc_t* qc, bwamem_baseqc_t* bq);

typedef struct {
    /* algorithmic counters */
    uint64_t n_reads, n_ext, n_lf, n_sa, n_dp_cells;
    /* accumulated device time per kernel, ms, and launch counts (HIP events on the launch stream) */
    double ms_encode, ms_seed, ms_sa, ms_chain, ms_extend, ms_post, ms_final, ms_pack, ms_other;
    uint64_t n_launch_seed, n_launch_sa, n_launch_extend;
    uint64_t n_tiles, n_retries;
} bwamem_stats_t;

/* Tooling (tests): the LDS plan of the persistent seeding grid, pure host arithmetic (csrc/kernels.h: seed_lds_plan).  For a CU
 * with lds_per_cu bytes of LDS handed out in blocks of `granule` bytes, reads of up to max_len bases, the narrow (narrow != 0) or
 * wide candidate rings of K entries (a power of two) and `reserve` bytes per CU to be left free: *lds_bytes = what one workgroup
 * asks for, *wpc = workgroups per CU, 1..16, with wpc * round_up(lds_bytes, granule) + reserve <= lds_per_cu.  0 = ok; 1 = the
 * reserve was cut to what one workgroup leaves; -1 = bad arguments. */
int bwamem_hip_seed_lds_plan(int64_t lds_per_cu, int64_t granule, int max_len, int narrow, int K, int64_t reserve, int64_t* lds_bytes, int* wpc);

void bwamem_hip_stats_enable(int on);          /* per-kernel HIP-event timing (off by default) */
void bwamem_hip_stats_reset(void);
void bwamem_hip_stats_get(bwamem_stats_t* out);

#ifdef __cplusplus
}
#endif
#endif
