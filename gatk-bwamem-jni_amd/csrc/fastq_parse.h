// fastq_parse.h -- FASTQ text taken apart on the device: the format rules, the line index, and the check of one record.  Shared by
// the parse kernels next to the BAM kernels (k_post.hip) and by the host, so it compiles for both, like bam_encode.h.
//
// The text is uploaded as it is; the host never looks at its bytes.  The rules:
//   records     exactly four lines each.  Sequences wrapped over several lines are not supported: a wrapped file fails the
//               '@' / '+' / length checks below and is an error.
//   lines       end in "\n" or "\r\n" (the '\r' is dropped).  The last line may lack its newline.  A text whose line count is not
//               a multiple of four is an error (of no single record: bad_record = -1).  An empty text holds no record.
//   line 1      begins with '@'.  The name is the bytes after it up to the first space or tab; the rest (the comment) is dropped.
//               A trailing "/1" or "/2" of a name longer than two bytes is removed (bwa: trim_readno).  The name then has
//               1..254 bytes.
//   line 2      the bases; it may be empty (a read of length 0).  The bytes go into the payload unchanged: case is kept, and
//               any non-ACGT byte is N downstream.
//   line 3      begins with '+'; the rest is ignored.
//   line 4      as many bytes as line 2, each in 33..126 (Phred+33).
//   kinds       lines are classified by number, never by content: a quality line may begin with '@' or '+'.
//   pairs       two texts: equal record counts (else bad_record = -1); read 2i comes from the first, read 2i + 1 from the second,
//               and their trimmed names must be equal.  One interleaved text: bwamem_hip_batch_encode_bam(paired = 1) makes the
//               same name check.  bad_record counts reads of the batch: the record's index in a single text, 2i or 2i + 1 for
//               two texts, the first read of a pair whose names differ.
// Compressed FASTQ comes in through bwamem_hip_batch_upload_fastq_gz: BGZF members are inflated on the device into the place the
// text would have been copied to (bgzf_inflate.h), and everything below runs on that text unchanged.  Cutting a file larger than
// one call is out of scope (one request under 2 GiB of text, as everywhere).
//
// The line index.  A text of n bytes has a newline at p when text[p] == '\n', and one more at p == n when n > 0 and the last
// byte is no '\n' (the last line lacks its newline).  Line k (from 0) starts at start[k] and ends before start[k + 1] - 1, with
// start[0] = 0 and start[j] = p + 1 for the j-th newline p (from 1).  The newlines are counted per chunk of FASTQ_CHUNK bytes
// (chunks cover the positions 0..n, so there are n / FASTQ_CHUNK + 1 of them), the counts are scanned, and every newline's
// number is its chunk's base plus its rank within the chunk: the index is a function of the text alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define FQ_HD static __host__ __device__ inline

#define FASTQ_CHUNK 4096                       // bytes of text per workgroup of the counting and the line-start kernels
#define FASTQ_LANE_BYTES 16                    // one 16-byte load per lane: FASTQ_CHUNK / FASTQ_LANE_BYTES lanes per workgroup
#define FASTQ_THREADS (FASTQ_CHUNK / FASTQ_LANE_BYTES)
#define FASTQ_NAME_MAX 254
#define FASTQ_NO_ERROR 0x7fffffff              // an error word holds FASTQ_NO_ERROR - the smallest offending read (by atomicMax), 0 = none

FQ_HD int64_t fastq_n_chunks(int64_t n) { return n / FASTQ_CHUNK + 1; }

// is there a newline at position p (0 <= p <= n)?
FQ_HD bool fastq_newline_at(const uint8_t* text, int64_t n, int64_t p)
{
    return p < n ? text[p] == '\n' : (p == n && n > 0 && text[n - 1] != '\n');
}

// the bits of a 32-bit word of text whose bytes are '\n': 0x80 in each such byte
FQ_HD uint32_t fastq_newline_bits(uint32_t w)
{
    const uint32_t x = w ^ 0x0a0a0a0au;
    return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);
}

// One record: the places of its name, bases and qualities in the text.
struct FastqRec { int64_t name, seq, qual; int32_t l_name, l_seq; };

// Checks record i (lines 4i .. 4i + 3 of the index `start`) against the rules above.  -> true, and R filled in
FQ_HD bool fastq_record(const uint8_t* text, const int64_t* start, int64_t i, FastqRec& R)
{
    int64_t b[4], e[4];
    for (int k = 0; k < 4; ++k) {
        b[k] = start[4 * i + k]; e[k] = start[4 * i + k + 1] - 1;
        if (e[k] > b[k] && text[e[k] - 1] == '\r') --e[k];
    }
    if (e[0] <= b[0] || text[b[0]] != '@') return false;
    if (e[2] <= b[2] || text[b[2]] != '+') return false;
    int64_t ne = b[0] + 1;
    while (ne < e[0] && text[ne] != ' ' && text[ne] != '\t') ++ne;
    int64_t l_name = ne - (b[0] + 1);
    if (l_name > 2 && text[ne - 2] == '/' && (text[ne - 1] == '1' || text[ne - 1] == '2')) l_name -= 2;
    if (l_name < 1 || l_name > FASTQ_NAME_MAX) return false;
    const int64_t l_seq = e[1] - b[1];
    if (e[3] - b[3] != l_seq || l_seq >= 0x7fffffff) return false;
    for (int64_t q = b[3]; q < e[3]; ++q) if (text[q] < 33 || text[q] > 126) return false;
    R.name = b[0] + 1; R.l_name = (int32_t)l_name; R.seq = b[1]; R.qual = b[3]; R.l_seq = (int32_t)l_seq;
    return true;
}

// What the parse kernels see of one text (k_post.hip: launch_fastq_*).  Reads of the batch: read = stride * record + phase.
struct FastqText {
    const uint8_t* text;          // n bytes, 16-byte aligned (no load goes beyond n)
    int64_t n;
    const int64_t* chunk_base;    // [n_chunks + 1] the scan of the chunks' newline counts
    int64_t* start;               // [n_lines + 1] the line index
    int64_t n_lines;
    int32_t n_rec, stride, phase;
};

// The reads of a batch as the copy kernel fills them in: bases + NUL and qualities + NUL at the same offsets, and the names.
struct FastqOut {
    int32_t* len1;                // [n_reads] l_seq + 1
    int32_t* l_name;              // [n_reads]
    const int64_t* seq_off;       // [n_reads + 1] their scans
    const int64_t* name_off;
    uint8_t *seq, *qual, *names;
    int32_t* err;                 // [0]: FASTQ_NO_ERROR - the smallest offending read index (atomicMax), 0 = none; [1]: the longest read
};
