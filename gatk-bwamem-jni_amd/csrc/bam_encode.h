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
//   SA, MC, MQ       on request only (bwamem_hip_batch_set_tags; BAM_TAG_*), between XA and RG: NM MD AS XS XA SA MC MQ RG.  Like
//                    everything above they are defined on the response alone.  For a read with records 0..n-1 in response order:
//                    SA:Z goes on record k when k is mapped and has no 0x100 and at least one other record j of the read is
//                    mapped and has no 0x100; its value is one entry "rname,pos,strand,CIGAR,mapQ,NM;" for each such j != k,
//                    in response order: rname the contig's @SQ name, pos 1-based, strand + or - from j's 0x10, CIGAR j's response
//                    words as text (clips stay S, whatever j's own line shows; "*" for none), mapQ and NM j's (mem_aln2sam's rule,
//                    in the SAM tags specification's format).  Records with 0x100 carry no SA and are listed in none.
//                    MC:Z / MQ:i exist only in a paired encode: they go on every record of read 2i / 2i+1, mapped or not, whose
//                    mate's record 0 is mapped (the record the response's mate fields come from): MC is that record's CIGAR as
//                    text (clips S), MQ its mapping quality in the smallest integer type.  An unpaired encode ignores both bits.
//                    A record the tags push past 2^31 - 1 bytes is refused like any other (BAM_ERR_SPAN)
// The text of other records does not fit bam_byte's shape (a pure function of record and position), so the tagged forms read it
// from a per-read side buffer made by the same three steps as the records: sizes (BamTagInfo), a scan, and the text (bam_put_sa_entry, bam_put_cigar).
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
// bytes of v's decimal text, and the text itself at dst: the digits come out of a register, last one first
BAM_HD int bam_dec_len(int64_t v) { return v < 0 ? 1 + bam_dec_digits(0 - (uint64_t)v) : bam_dec_digits((uint64_t)v); }
BAM_HD void bam_put_dec(uint8_t* dst, int64_t v)
{
    const int neg = v < 0, n = bam_dec_len(v);
    uint64_t u = neg ? 0 - (uint64_t)v : (uint64_t)v;
    if (neg) dst[0] = '-';
    for (int d = n - 1; d >= neg; --d) { dst[d] = (uint8_t)('0' + (int)(u % 10)); u /= 10; }
}

// the optional tags (bwamem_hip_batch_set_tags; the values of BWAMEM_HIP_TAG_*)
enum { BAM_TAG_SA = 1, BAM_TAG_MC = 2, BAM_TAG_MQ = 4, BAM_TAG_ALL = 7 };

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
    // the tagged forms only (TAGS): the bytes of the CIGAR as text, and the values of SA and MC in the read's and its mate's side
    // text (bam_tags sets them; a length of 0: no tag).  SA's value is sa[0, l_sa + sa_cut_len) without [sa_cut, sa_cut + sa_cut_len),
    // the record's own entry
    int32_t l_cigtxt;
    const uint8_t* sa; const uint8_t* mc;
    int32_t l_sa, sa_cut, sa_cut_len, l_mc, has_mq, mq;
    int32_t o_sa, o_mc, o_mq;
};

// Parses the k-th record of a read (k counts from 0: later mapped records are hard-clipped) at p, of at most n_avail words; l_read =
// the read's length.  n_seqs bounds the contig ids.  The name fields of R must be set by the caller before bam_layout.
// -> 0, or BAM_ERR_* (R is then unusable).  TAGS: also the length of the CIGAR's text, and no SA / MC / MQ until bam_tags says so;
// the forms without TAGS never touch those fields.
template <bool TAGS = false>
BAM_HD int bam_parse(const uint32_t* p, int64_t n_avail, int k, int32_t l_read, int32_t n_seqs, BamRec& R)
{
    R.rg = 0; R.l_rg = 0;
    if (TAGS) { R.l_cigtxt = 0; R.sa = R.mc = 0; R.l_sa = R.sa_cut = R.sa_cut_len = R.l_mc = R.has_mq = R.mq = 0; }
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
        if (TAGS) R.l_cigtxt += bam_dec_digits(len) + 1;
    }
    if (TAGS && R.n_cig == 0) R.l_cigtxt = 1;                            // "*" (at most 65 535 operations of 11 bytes: no overflow)
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

// the section offsets and the total size (block_size included) of the record; needs the parse and the name (TAGS: and bam_tags)
template <bool TAGS = false>
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
    if (TAGS) {
        R.o_sa = (int32_t)o; if (R.l_sa > 0) o += 3 + (int64_t)R.l_sa + 1;
        R.o_mc = (int32_t)o; if (R.l_mc > 0) o += 3 + (int64_t)R.l_mc + 1;
        R.o_mq = (int32_t)o; if (R.has_mq) o += 3 + bam_int_width(R.mq);
    }
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

// byte t of SA:Z: the side text without the record's own entry
BAM_HD uint8_t bam_sa_tag_byte(const BamRec& R, int t)
{
    if (t < 3) return (uint8_t)(t == 0 ? 'S' : t == 1 ? 'A' : 'Z');
    t -= 3;
    return t >= R.l_sa ? (uint8_t)0 : R.sa[t < R.sa_cut ? t : t + R.sa_cut_len];
}

// the byte at position i (0 <= i < R.total) of the BAM record; qual = the read's qualities, or null (none: 0xFF)
template <bool TAGS = false>
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
    if (TAGS) {
        if (i < R.o_sa) return bam_str_tag_byte('X', 'A', R.xa, R.n_xa, i - R.o_xa);
        if (i < R.o_mc) return bam_sa_tag_byte(R, i - R.o_sa);
        if (i < R.o_mq) return bam_str_tag_byte('M', 'C', R.mc, R.l_mc, i - R.o_mc);
        if (i < R.o_rg) return bam_int_tag_byte('M', 'Q', R.mq, i - R.o_mq);
        return bam_str_tag_byte('R', 'G', R.rg, R.l_rg, i - R.o_rg);
    }
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

// What a read contributes to the optional tags (k_bam_tag_size): record 0 as its mate sees it (0x100 | mapQ when mapped, else 0), and
// the read's side text: the SA entries of its listed records back to back (l_sa bytes; 0 unless SA is asked for and n_sa >= 2), then
// record 0's CIGAR as text (l_mc bytes; 0 unless the call is paired, MC is asked for and record 0 is mapped).
struct BamTagInfo { int32_t mate, l_mc, n_sa, l_sa; };

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
    // The tagged forms only (tags != 0).  These arrays span the batch and are indexed by read0 + r, so a read finds its mate's entry
    // wherever the tiles were cut (a paired alignment never splits a pair -- plan_tiles and produce_streamed in pipeline.cpp -- but
    // `paired` here is the encode call's own argument, so nothing is assumed).
    uint32_t tags;                // BAM_TAG_*
    int32_t read0, n_batch;       // the tile's first read within the batch, and the batch's reads
    const int32_t* ctg_name_off;  // the contigs' names as in @SQ (DevIndex::ann_name_off / names: NUL-terminated, [n_seqs + 1] offsets)
    const uint8_t* ctg_names;
    BamTagInfo* tag_info;         // [n_batch]
    int32_t* tag_sizes;           // [n_batch] bytes of each read's side text
    const int64_t* tag_off;       // [n_batch + 1] their places in tag_text (after the scan)
    uint8_t* tag_text;            // null in the size kernels
};

// names the record of read r of the tile
BAM_HD void bam_name(const BamTile& t, int r, BamRec& R)
{
    if (t.names) { R.name = t.names + t.name_off[r]; R.l_name = (int32_t)(t.name_off[r + 1] - t.name_off[r]); R.name_idx = 0; R.name_letter = 0; }
    else bam_default_name(R, t.paired, (uint64_t)(t.read_index0 + r));
    R.rg = t.rg; R.l_rg = t.l_rg;
}

// ---- SA / MC / MQ (the rule at the top).  A record is listed in SA when it is mapped and not secondary.
BAM_HD bool bam_sa_listed(const BamRec& R) { return R.mapped && !(R.flag & 0x100); }
BAM_HD int32_t bam_ctg_name_len(const BamTile& t, int32_t rid) { return t.ctg_name_off[rid + 1] - t.ctg_name_off[rid] - 1; }
// bytes of R's entry "rname,pos,strand,CIGAR,mapQ,NM;" (R parsed with TAGS)
BAM_HD int64_t bam_sa_entry_len(const BamTile& t, const BamRec& R)
{
    return (int64_t)bam_ctg_name_len(t, R.refid) + 1 + bam_dec_len((int64_t)R.pos + 1) + 3 + (int64_t)R.l_cigtxt + 1 + bam_dec_len(R.mapq) + 1 + bam_dec_len(R.nm) + 1;
}
BAM_HD uint8_t bam_cigar_letter(uint32_t op) { return op < 8 ? (uint8_t)(0x3d5048534e44494dull >> (8 * op)) : op == 8 ? (uint8_t)'X' : (uint8_t)'?'; }   // "MIDNSHP=" X

// R's CIGAR as text (l_cigtxt bytes; clips as the response has them: S) at dst.  Lane sub of G writes operations sub, sub + G, ...;
// every lane adds up the places itself, as every lane parses the record itself.
BAM_HD void bam_put_cigar(uint8_t* dst, const BamRec& R, int sub, int G)
{
    if (R.n_cig == 0) { if (sub == 0) dst[0] = '*'; return; }
    int64_t o = 0;
    for (int32_t c = 0; c < R.n_cig; ++c) {
        const uint32_t v = R.cig[c], len = v >> 4;
        const int nd = bam_dec_digits(len);
        if (c % G == sub) { bam_put_dec(dst + o, len); dst[o + nd] = bam_cigar_letter(v & 0xf); }
        o += nd + 1;
    }
}
// R's SA entry (bam_sa_entry_len bytes) at dst, by lane sub of G
BAM_HD void bam_put_sa_entry(uint8_t* dst, const BamTile& t, const BamRec& R, int sub, int G)
{
    const uint8_t* rname = t.ctg_names + t.ctg_name_off[R.refid];
    const int32_t l_rname = bam_ctg_name_len(t, R.refid);
    for (int32_t i = sub; i < l_rname; i += G) dst[i] = rname[i];
    int64_t o = l_rname;
    const int n_pos = bam_dec_len((int64_t)R.pos + 1);
    if (sub == 0) { dst[o] = ','; bam_put_dec(dst + o + 1, (int64_t)R.pos + 1); dst[o + 1 + n_pos] = ','; dst[o + 2 + n_pos] = R.flag & 0x10 ? '-' : '+'; dst[o + 3 + n_pos] = ','; }
    o += n_pos + 4;
    bam_put_cigar(dst + o, R, sub, G);
    o += R.l_cigtxt;
    if (sub == G - 1) {
        const int n_q = bam_dec_len(R.mapq);
        dst[o] = ','; bam_put_dec(dst + o + 1, R.mapq); dst[o + 1 + n_q] = ','; bam_put_dec(dst + o + 2 + n_q, R.nm); dst[o + 2 + n_q + bam_dec_len(R.nm)] = ';';
    }
}

// SA, MC and MQ of record R (parsed with TAGS) of the tile's read r, before bam_layout.  sa_at: the bytes of the read's listed records
// before R.  -> the bytes of R's own entry (0: not listed), for the caller to add to sa_at.
BAM_HD int64_t bam_tags(const BamTile& t, int r, BamRec& R, int64_t sa_at)
{
    const int64_t g = (int64_t)t.read0 + r;
    int64_t own = 0;
    if (bam_sa_listed(R)) {
        own = bam_sa_entry_len(t, R);
        const int32_t l_all = t.tag_info[g].l_sa;
        if (l_all > 0) { R.l_sa = (int32_t)(l_all - own); R.sa_cut = (int32_t)sa_at; R.sa_cut_len = (int32_t)own; if (t.tag_text) R.sa = t.tag_text + t.tag_off[g]; }
    }
    const int64_t m = g ^ 1;
    if (t.paired && (t.tags & (BAM_TAG_MC | BAM_TAG_MQ)) && m < t.n_batch) {
        const BamTagInfo mate = t.tag_info[m];
        if (mate.mate & 0x100) {
            if (t.tags & BAM_TAG_MC) { R.l_mc = mate.l_mc; if (t.tag_text) R.mc = t.tag_text + t.tag_off[m] + mate.l_sa; }
            if (t.tags & BAM_TAG_MQ) { R.has_mq = 1; R.mq = mate.mate & 0xff; }
        }
    }
    return own;
}
