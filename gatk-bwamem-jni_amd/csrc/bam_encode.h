// bam_encode.h -- BAM alignment records (SAM specification section 4.2) from the records of a response: the parse of one
// response record, the size of its BAM record, and the byte at position i of that record.  Shared by the size / emit
// kernels next to k_pack (k_post.hip) and by the host (sam_writer.cpp), so it compiles for both.
//
// One rule defines the content: a BAM record decodes to exactly the SAM line bwamem_hip_response_to_sam (sam_writer.cpp)
// writes for the same response record.  What follows from it:
//   refID / pos      the record's own; an unmapped read with a mapped mate sits at its mate's place; else -1 / -1
//   next_*, tlen     the three cases of RNEXT / PNEXT / TLEN there ("=" is the numeric id)
//   bin              reg2bin(pos, pos + reference span of the CIGAR) (a span of 0 counts as 1, as in the specification's
//                    5.3); a placed unmapped read reg2bin(pos, pos + 1); an unplaced one 4680 = reg2bin(-1, 0)
//   CIGAR            the response's words (len << 4 | op, already BAM's numbering); S becomes H on a read's second and
//                    later mapped records; none on unmapped records.  n_cigar_op is 16 bits wide: a record with more than
//                    65 535 operations is an error (the CG-tag convention for longer CIGARs is not implemented)
//   SEQ              4-bit codes of "=ACMGRSVTWYHKDBN" from the request's ASCII (either case; any other byte is N), reverse-
//                    complemented (A<->T, C<->G, the other codes stay, as the SAM writer's comp()) when flag 0x10 is set,
//                    trimmed to the unclipped part on hard-clipped records
//   QUAL             l_seq bytes of 0xFF when the batch carries no qualities (bwamem_hip_batch_set_qualities, or a batch made
//                    from FASTQ text); else byte q is qual[i] - 33 with i the index bam_seq_code uses for SEQ base q: reversed
//                    where SEQ is reverse-complemented, trimmed where SEQ is hard-clipped
//   tags             NM, MD (if non-empty), AS, XS (if >= 0), XA (if non-empty); integers in the smallest type that holds
//                    the value (C S I for non-negative ones, c s i for negative ones), strings as Z.  With a read group
//                    (bwamem_hip_batch_set_read_group) RG:Z:<ID> comes last on every record, unmapped ones included
//   read names       the caller's (1..254 bytes each), else "r<index>" / "p<pair index>" with the index counted over the
//                    whole logical call (read_id0 of the align call + the index within the batch)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define BAM_HD static __host__ __device__ inline

enum { BAM_ERR_CIGAR_OPS = 1, BAM_ERR_PARSE = 2, BAM_ERR_SPAN = 4 };
#define BAM_MAX_CIGAR_OPS 65535

// SAM specification 5.3: the bin of the zero-based half-open interval [beg, end)
BAM_HD int bam_reg2bin(int64_t beg, int64_t end)
{
    --end;
    if (beg >> 14 == end >> 14) return (int)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (int)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (int)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (int)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (int)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

// the 4-bit code of a base as sent ("=ACMGRSVTWYHKDBN")
BAM_HD int bam_base_code(uint8_t c)
{
    switch (c & 0xdf) {                                   // letters: upper case
        case 'A': return 1; case 'C': return 2; case 'M': return 3; case 'G': return 4; case 'R': return 5; case 'S': return 6;
        case 'V': return 7; case 'T': return 8; case 'W': return 9; case 'Y': return 10; case 'H': return 11; case 'K': return 12;
        case 'D': return 13; case 'B': return 14;
    }
    return c == '=' ? 0 : 15;
}
// A<->T, C<->G; every other code stays (sam_writer.cpp: comp)
BAM_HD int bam_comp_code(int c) { return c == 1 ? 8 : c == 8 ? 1 : c == 2 ? 4 : c == 4 ? 2 : c; }

// bytes of an integer tag's value, and its type letter
BAM_HD int bam_int_width(int32_t v) { return v >= 0 ? (v <= 0xff ? 1 : v <= 0xffff ? 2 : 4) : (v >= -128 ? 1 : v >= -32768 ? 2 : 4); }
BAM_HD uint8_t bam_int_type(int32_t v) { const int w = bam_int_width(v); return (uint8_t)(v >= 0 ? (w == 1 ? 'C' : w == 2 ? 'S' : 'I') : (w == 1 ? 'c' : w == 2 ? 's' : 'i')); }

BAM_HD int bam_dec_digits(uint64_t v) { int n = 1; while (v >= 10) { v /= 10; ++n; } return n; }

// One response record (layout of jnibwa.c:43-98, as sam_writer.cpp walks it) and the layout of its BAM record.
struct BamRec {
    const uint32_t* cig; const uint8_t* md; const uint8_t* xa;          // into the response
    int32_t flag, mapq, nm, as, xs, n_cig, n_md, n_xa;
    int32_t words;                                                       // response words the record takes
    int32_t refid, pos, next_refid, next_pos, tlen, bin, n_cigar_op;     // BAM fields
    int32_t hard, seq_b, l_seq, l_read;                                  // SEQ = bases [seq_b, seq_b + l_seq) of the (reverse-complemented) read
    int32_t mapped;
    // the name
    const uint8_t* name; int32_t l_name; uint64_t name_idx; uint8_t name_letter;     // name == null: name_letter + decimal name_idx
    // offsets of the sections within the BAM record (block_size at 0, the fixed fields up to 36)
    int32_t o_cigar, o_seq, o_qual, o_nm, o_md, o_as, o_xs, o_xa, o_rg, total;
    // the read group's ID (null: no RG tag); bam_parse leaves none, bam_name sets the tile's
    const uint8_t* rg; int32_t l_rg;
};

// Parses the k-th record of a read (k counts from 0: later mapped records are hard-clipped) at p, of at most n_avail words; l_read =
// the read's length.  n_seqs bounds the contig ids.  The name fields of R must be set by the caller before bam_layout.
// -> 0, or BAM_ERR_* (R is then unusable).
BAM_HD int bam_parse(const uint32_t* p, int64_t n_avail, int k, int32_t l_read, int32_t n_seqs, BamRec& R)
{
    R.rg = 0; R.l_rg = 0;
    if (n_avail < 1) return BAM_ERR_PARSE;
    const uint32_t fm = p[0];
    int64_t at = 1;
    R.flag = (int32_t)(fm >> 16 & 0xffff); R.mapq = (int32_t)(fm & 0xff);
    R.mapped = !(R.flag & 4);
    int32_t rid = -1, pos = -1;
    R.nm = R.as = R.xs = R.n_cig = R.n_md = R.n_xa = 0; R.cig = 0; R.md = R.xa = 0;
    if (R.mapped) {
        if (n_avail < at + 6) return BAM_ERR_PARSE;
        rid = (int32_t)p[at]; pos = (int32_t)p[at + 1]; R.nm = (int32_t)p[at + 2]; R.as = (int32_t)p[at + 3]; R.xs = (int32_t)p[at + 4]; R.n_cig = (int32_t)p[at + 5];
        at += 6;
        if (R.n_cig < 0 || n_avail < at + (int64_t)R.n_cig + 1) return BAM_ERR_PARSE;
        R.cig = p + at; at += R.n_cig;
        R.n_md = (int32_t)p[at++];
        if (R.n_md < 0 || n_avail < at + (((int64_t)R.n_md + 3) >> 2) + 1) return BAM_ERR_PARSE;
        R.md = (const uint8_t*)(p + at); at += ((int64_t)R.n_md + 3) >> 2;
        R.n_xa = (int32_t)p[at++];
        if (R.n_xa < 0 || n_avail < at + (((int64_t)R.n_xa + 3) >> 2)) return BAM_ERR_PARSE;
        R.xa = (const uint8_t*)(p + at); at += ((int64_t)R.n_xa + 3) >> 2;
        if (rid < 0) return BAM_ERR_PARSE;
    }
    int32_t mrid = -1, mpos = -1, tlen = 0;
    const bool has_mate = (R.flag & 9) == 1;
    if (has_mate) {
        if (n_avail < at + 3) return BAM_ERR_PARSE;
        mrid = (int32_t)p[at]; mpos = (int32_t)p[at + 1]; tlen = (int32_t)p[at + 2]; at += 3;
    }
    if (rid >= n_seqs || mrid >= n_seqs) return BAM_ERR_PARSE;
    if (at > 0x7fffffff) return BAM_ERR_PARSE;
    R.words = (int32_t)at;
    if (R.n_cig > BAM_MAX_CIGAR_OPS) return BAM_ERR_CIGAR_OPS;
    // where the record sits, and its mate (sam_writer.cpp, "the line")
    if (rid >= 0) { R.refid = rid; R.pos = pos; }
    else if (has_mate && mrid >= 0) { R.refid = mrid; R.pos = mpos; }
    else { R.refid = -1; R.pos = -1; }
    if (has_mate && mrid >= 0) { R.next_refid = mrid; R.next_pos = mpos; }
    else if (has_mate && rid >= 0) { R.next_refid = rid; R.next_pos = pos; }
    else { R.next_refid = -1; R.next_pos = -1; }
    R.tlen = has_mate && rid >= 0 && mrid >= 0 ? tlen : 0;
    // the CIGAR: reference span and clips
    R.hard = k > 0 && R.mapped;
    R.n_cigar_op = R.n_cig;
    int64_t span = 0; uint32_t clip5 = 0, clip3 = 0;
    for (int32_t c = 0; c < R.n_cig; ++c) {
        const uint32_t v = R.cig[c], op = v & 0xf, len = v >> 4;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) span += len;
        if (op == 4 || op == 5) { if (c == 0) clip5 = len; else clip3 = len; }
    }
    if (R.refid < 0) R.bin = 4680;
    else if (!R.mapped) R.bin = bam_reg2bin(R.pos, (int64_t)R.pos + 1);
    else R.bin = bam_reg2bin(R.pos, (int64_t)R.pos + (span > 0 ? span : 1));
    R.l_read = l_read;
    int64_t b = 0, e = l_read;
    if (R.hard) { b = clip5; e = (int64_t)l_read - (int64_t)clip3; if (b > e) { b = 0; e = l_read; } }
    R.seq_b = (int32_t)b; R.l_seq = (int32_t)(e - b);
    return 0;
}

// the default name of a read: 'r' + its index in the call, or 'p' + its pair's
BAM_HD void bam_default_name(BamRec& R, int paired, uint64_t read_index)
{
    R.name = 0; R.name_letter = paired ? 'p' : 'r'; R.name_idx = paired ? read_index >> 1 : read_index;
    R.l_name = 1 + bam_dec_digits(R.name_idx);
}

// the section offsets and the total size (block_size included) of the record; needs the parse and the name
BAM_HD int32_t bam_layout(BamRec& R)
{
    int64_t o = 36 + (int64_t)R.l_name + 1;
    R.o_cigar = (int32_t)o; o += 4 * (int64_t)R.n_cigar_op;
    R.o_seq = (int32_t)o;   o += ((int64_t)R.l_seq + 1) >> 1;
    R.o_qual = (int32_t)o;  o += R.l_seq;
    R.o_nm = (int32_t)o;    if (R.mapped) o += 3 + bam_int_width(R.nm);
    R.o_md = (int32_t)o;    if (R.mapped && R.n_md > 0) o += 3 + (int64_t)R.n_md + 1;
    R.o_as = (int32_t)o;    if (R.mapped) o += 3 + bam_int_width(R.as);
    R.o_xs = (int32_t)o;    if (R.mapped && R.xs >= 0) o += 3 + bam_int_width(R.xs);
    R.o_xa = (int32_t)o;    if (R.mapped && R.n_xa > 0) o += 3 + (int64_t)R.n_xa + 1;
    R.o_rg = (int32_t)o;    if (R.rg) o += 3 + (int64_t)R.l_rg + 1;
    R.total = o > 0x7fffffff ? -1 : (int32_t)o;
    return R.total;
}

BAM_HD uint8_t bam_int_tag_byte(char a, char b, int32_t v, int t)
{
    return t == 0 ? (uint8_t)a : t == 1 ? (uint8_t)b : t == 2 ? bam_int_type(v) : (uint8_t)((uint32_t)v >> (8 * (t - 3)));
}
BAM_HD uint8_t bam_str_tag_byte(char a, char b, const uint8_t* s, int32_t n, int t)
{
    return t == 0 ? (uint8_t)a : t == 1 ? (uint8_t)b : t == 2 ? (uint8_t)'Z' : t - 3 < n ? s[t - 3] : (uint8_t)0;
}

// base q of SEQ as a 4-bit code; raw = the read's ASCII as uploaded
BAM_HD int bam_seq_code(const BamRec& R, const uint8_t* raw, int32_t q)
{
    if (q >= R.l_seq) return 0;
    const int32_t i = R.seq_b + q;
    return R.flag & 0x10 ? bam_comp_code(bam_base_code(raw[R.l_read - 1 - i])) : bam_base_code(raw[i]);
}

// byte q of QUAL; qual = the read's Phred+33 string, laid out like raw
BAM_HD uint8_t bam_qual_byte(const BamRec& R, const uint8_t* qual, int32_t q)
{
    const int32_t i = R.seq_b + q;
    return (uint8_t)(qual[R.flag & 0x10 ? R.l_read - 1 - i : i] - 33);
}

// the byte at position i (0 <= i < R.total) of the BAM record; qual = the read's qualities, or null (none: 0xFF)
BAM_HD uint8_t bam_byte(const BamRec& R, const uint8_t* raw, int32_t i, const uint8_t* qual = 0)
{
    if (i < 36) {
        uint32_t w;
        switch (i >> 2) {
            case 0: w = (uint32_t)(R.total - 4); break;
            case 1: w = (uint32_t)R.refid; break;
            case 2: w = (uint32_t)R.pos; break;
            case 3: w = (uint32_t)(R.l_name + 1) | (uint32_t)R.mapq << 8 | (uint32_t)R.bin << 16; break;
            case 4: w = (uint32_t)R.n_cigar_op | (uint32_t)R.flag << 16; break;
            case 5: w = (uint32_t)R.l_seq; break;
            case 6: w = (uint32_t)R.next_refid; break;
            case 7: w = (uint32_t)R.next_pos; break;
            default: w = (uint32_t)R.tlen; break;
        }
        return (uint8_t)(w >> (8 * (i & 3)));
    }
    if (i < R.o_cigar) {
        const int32_t j = i - 36;
        if (j >= R.l_name) return 0;
        if (R.name) return R.name[j];
        if (j == 0) return R.name_letter;
        uint64_t v = R.name_idx;
        for (int32_t d = R.l_name - 1 - j; d > 0; --d) v /= 10;
        return (uint8_t)('0' + (int)(v % 10));
    }
    if (i < R.o_seq) {
        const int32_t j = i - R.o_cigar;
        uint32_t v = R.cig[j >> 2];
        if (R.hard && (v & 0xf) == 4) v = (v & ~0xfu) | 5u;
        return (uint8_t)(v >> (8 * (j & 3)));
    }
    if (i < R.o_qual) {
        const int32_t q = 2 * (i - R.o_seq);
        return (uint8_t)(bam_seq_code(R, raw, q) << 4 | bam_seq_code(R, raw, q + 1));
    }
    if (i < R.o_nm) return qual ? bam_qual_byte(R, qual, i - R.o_qual) : (uint8_t)0xff;
    if (i < R.o_md) return bam_int_tag_byte('N', 'M', R.nm, i - R.o_nm);
    if (i < R.o_as) return bam_str_tag_byte('M', 'D', R.md, R.n_md, i - R.o_md);
    if (i < R.o_xs) return bam_int_tag_byte('A', 'S', R.as, i - R.o_as);
    if (i < R.o_xa) return bam_int_tag_byte('X', 'S', R.xs, i - R.o_xs);
    if (i < R.o_rg) return bam_str_tag_byte('X', 'A', R.xa, R.n_xa, i - R.o_xa);
    return bam_str_tag_byte('R', 'G', R.rg, R.l_rg, i - R.o_rg);
}

// A read group's header line (bwamem_hip_batch_set_read_group): one line that begins with "@RG\t", has an ID: field of 1..254
// bytes and holds no '\n', '\r' or NUL (the last by construction: the line is a C string).  -> the ID's place in the line and its
// length, or 0 when the line is refused.
BAM_HD int bam_rg_id(const char* line, const char** id)
{
    if (!line || line[0] != '@' || line[1] != 'R' || line[2] != 'G' || line[3] != '\t') return 0;
    const char* found = 0; int l_found = 0;
    for (const char* p = line + 3; *p; ) {                               // p at a tab: a field follows
        const char* f = ++p;
        while (*p && *p != '\t') { if (*p == '\n' || *p == '\r') return 0; ++p; }
        if (!found && p - f >= 3 && f[0] == 'I' && f[1] == 'D' && f[2] == ':') { found = f + 3; l_found = (int)(p - f - 3); if (p - f - 3 > 254) return 0; }
    }
    if (!found || l_found < 1) return 0;
    *id = found;
    return l_found;
}

// What the size and emit kernels see of one tile of a batch (k_post.hip: launch_bam_size / launch_bam_emit).
struct BamTile {
    const uint8_t* resp;          // the tile's packed response (TileOut.d)
    const int64_t* resp_off;      // [n_reads + 1] offsets of the reads within it (the copy kept on request)
    int32_t n_reads, max_len;
    const uint8_t* raw;           // the request as uploaded (ASCII) ...
    const int64_t* raw_off;       // ... and the offsets of this tile's reads in it, [n_reads + 1]
    int64_t read_index0;          // index of the tile's first read within the logical call (default names)
    int32_t paired, n_seqs;
    const uint8_t* names;         // caller's names (device) and the offsets of this tile's, [n_reads + 1]; or both null
    const int64_t* name_off;
    const uint8_t* qual;          // the batch's qualities (device), laid out like raw; or null
    const uint8_t* rg;            // the read group's ID (device), l_rg bytes; or null
    int32_t l_rg;
    int32_t* sizes;               // [n_reads] BAM bytes of each read's records (size kernel)
    const int64_t* out_off;       // [n_reads + 1] their places in out (after the scan)
    uint8_t* out;
    int32_t* err;                 // BAM_ERR_* flags, OR-ed
};

// names the record of read r of the tile
BAM_HD void bam_name(const BamTile& t, int r, BamRec& R)
{
    if (t.names) { R.name = t.names + t.name_off[r]; R.l_name = (int32_t)(t.name_off[r + 1] - t.name_off[r]); R.name_idx = 0; R.name_letter = 0; }
    else bam_default_name(R, t.paired, (uint64_t)(t.read_index0 + r));
    R.rg = t.rg; R.l_rg = t.l_rg;
}
