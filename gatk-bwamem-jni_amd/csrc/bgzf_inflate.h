// bgzf_inflate.h -- the format side of BGZF decompression on the device: which streams are BGZF, the member table the host builds
// from the headers, canonical Huffman decoding (RFC 1951), and the checks that refuse a member.  Used by k_bgzf_inflate next to
// k_bgzf_deflate (k_post.hip) and by the host (pipeline.cpp); plain C++ that compiles for the device, the emulation build and the
// host.  Symbol tables, the token format (dfl_tok_*) and the CRC-32 arithmetic are bgzf_deflate.h's.
//
// The rules, binding for the kernel and the host:
//   stream kind   a member is BGZF when bytes 0..3 are 1f 8b 08 04 and its extra field (XLEN bytes from byte 12) holds a subfield
//                 'B' 'C' of length 2; the subfields are walked, others are skipped, XLEN may exceed 6.  If the first member of a
//                 stream is BGZF every member must be; otherwise the stream is plain gzip and is inflated on the host (libz).
//   member table  before the upload the host walks the BSIZE chain: coff[m], csize[m] = BSIZE + 1, the header length 12 + XLEN,
//                 ISIZE from the member's last four bytes, and uoff[m] = the sum of the ISIZEs before it.  The size of the text is
//                 known with no device wait; "one request under 2 GiB" is checked on the host.  Errors at the walk (bad_member =
//                 the member's index): ISIZE over 65 536, a BSIZE that runs past the data or is too small for header and trailer,
//                 a truncated last member, a bad magic in mid-stream.  Members with ISIZE 0 (the EOF block, anywhere) are legal,
//                 produce nothing, and still go through the kernel: their deflate data and CRC are checked.
//   deflate       all of RFC 1951: any number of blocks; stored blocks (LEN / NLEN checked), empty ones included; fixed codes;
//                 dynamic codes up to 15 bits; repeat codes running from the literal/length lengths into the distance lengths; one
//                 distance code of length 1 (incomplete, legal); no distance code at all.
//   refusals      BTYPE 3; an over-subscribed code; an incomplete code other than a single code of length 1 in the literal/length
//                 or distance alphabet; a repeat with no previous length; a repeat overrunning HLIT + HDIST; HLIT over 286 or
//                 HDIST over 30; no code for end-of-block; the symbols 286 / 287 and the distance symbols 30 / 31 (fixed codes);
//                 a bit pattern that is no code; a distance reaching before the member's first output byte; output beyond ISIZE
//                 or short of it; input exhausted before the final block's end-of-block; whole unused bytes between the end of
//                 the final block and the trailer; a CRC-32 mismatch.  The judge is zlib: the deflate area through
//                 inflate(-15) is valid when it ends the stream with no byte left over, the right length and CRC-32.
//   safety        every loop of the kernel is bounded by bits consumed (at most 8 * csize) or bytes produced (at most ISIZE); no
//                 load leaves [coff, coff + csize) apart from whole aligned 16-byte words inside the padded buffer (bytes outside the
//                 deflate area are zeroed before any lane looks at them); no store leaves [uoff, uoff + isize), whatever the bytes
//                 say: every token is checked against both ends before it is written.  A refused member atomicMax-es
//                 BGZI_NO_ERROR - m into the error word (k_fastq_records' form) and returns: the smallest offending member is
//                 reported whatever order the errors arrive in.
//   determinism   the text is a function of the compressed bytes alone: no lane order and no atomic decides a byte.
#pragma once
#include "bgzf_deflate.h"

#define BGZI_NO_ERROR 0x7fffffff               // the error word holds BGZI_NO_ERROR - the smallest refused member, 0 = none
enum { BGZI_THREADS = 64,                      // one wavefront per member
       BGZI_WIN = 2048, BGZI_WIN_DW = BGZI_WIN / 4,      // bytes of compressed data staged in LDS per turn
       BGZI_TOK = 256,                         // tokens decoded per turn: at most 48 bits each, 1 536 bytes < BGZI_WIN - 16 - 8
       BGZI_LL_PB = 10, BGZI_D_PB = 8,         // bits of the primary decode tables
       BGZI_MAX_ISIZE = 65536, BGZI_COOP_LEN = 32 };     // matches longer than this are copied by the whole wavefront
enum { BGZI_CODES = 0, BGZI_LENS = 1, BGZI_DISTS = 2 };

struct BgzfMember { int64_t coff, uoff; int32_t csize, hlen, isize, pad; };    // hlen = 12 + XLEN: the deflate area is [hlen, csize - 8)

// The header of the member at p[0, n): -> 12 + XLEN and *bsize when it is a BGZF member's, 0 otherwise
BGZ_HD int bgzf_member_header(const uint8_t* p, size_t n, int* bsize)
{
    if (n < 12 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || p[3] != 4) return 0;
    const size_t end = 12 + ((size_t)p[10] | (size_t)p[11] << 8);
    if (end > n) return 0;
    int found = -1;
    for (size_t at = 12; at + 4 <= end; ) {
        const size_t slen = (size_t)p[at + 2] | (size_t)p[at + 3] << 8;
        if (at + 4 + slen > end) return 0;
        if (p[at] == 'B' && p[at + 1] == 'C' && slen == 2 && found < 0) found = (int)p[at + 4] | (int)p[at + 5] << 8;
        at += 4 + slen;
    }
    if (found < 0) return 0;
    *bsize = found;
    return (int)end;
}

// One step of the walk: the member at p[at, n) into *m (coff = at; uoff is the caller's prefix sum).  0 = ok, 1 = no BGZF header,
// 2 = BSIZE runs past the data or leaves no room for header and trailer (a truncated member too), 3 = ISIZE over 65 536
BGZ_HD int bgzf_walk_member(const uint8_t* p, size_t n, size_t at, BgzfMember* m)
{
    int bsize = 0;
    const int hlen = bgzf_member_header(p + at, n - at, &bsize);
    if (!hlen) return 1;
    const size_t csize = (size_t)bsize + 1;
    if (csize > n - at || csize < (size_t)hlen + BGZF_TAIL) return 2;
    const uint8_t* t = p + at + csize - 4;
    const uint32_t isize = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
    if (isize > BGZI_MAX_ISIZE) return 3;
    m->coff = (int64_t)at; m->csize = (int32_t)csize; m->hlen = hlen; m->isize = (int32_t)isize; m->uoff = 0; m->pad = 0;
    return 0;
}

// ---- canonical codes (RFC 1951 3.2.2).  A code is count[1..15] (codes per length) and sym[] (the symbols sorted by length, then
// by value).  The next bits of the stream, first bit lowest, are walked one length at a time: the codes of a length are
// consecutive, and the first code of the next length is twice the one past the last.
// -> symbol | length << 12, or 0 when no code of at most max_len bits begins these bits
BGZ_HD uint32_t dfl_decode_walk(uint32_t bits, const uint16_t* count, const uint16_t* sym, int max_len)
{
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= max_len; ++len) {
        code |= (int)(bits & 1u); bits >>= 1;
        const int c = count[len];
        if (code - c < first) return (uint32_t)sym[index + (code - first)] | (uint32_t)len << 12;
        index += c; first += c; first <<= 1; code <<= 1;
    }
    return 0;
}

// count[0..15] and sym[] of the lengths len[0, n) (offs: 16 entries of scratch).  One lane.  -> false when the code is refused:
// over-subscribed, or incomplete (zlib's rule: a literal/length or distance code may be incomplete when its longest code has one
// bit, i.e. it is a single code of length 1; a code with no symbol at all is taken and refuses whatever is decoded with it)
BGZ_HD bool dfl_canonical(const uint8_t* len, int n, int kind, uint16_t* count, uint16_t* sym, uint16_t* offs)
{
    for (int b = 0; b <= 15; ++b) count[b] = 0;
    for (int s = 0; s < n; ++s) ++count[len[s] & 15];
    int left = 1, max = 0;
    for (int b = 1; b <= 15; ++b) { left = (left << 1) - (int)count[b]; if (left < 0) return false; if (count[b]) max = b; }
    if (left > 0 && max != 0 && (kind == BGZI_CODES || max != 1)) return false;
    offs[1] = 0;
    for (int b = 1; b < 15; ++b) offs[b + 1] = (uint16_t)(offs[b] + count[b]);
    for (int s = 0; s < n; ++s) if (len[s] & 15) sym[offs[len[s] & 15]++] = (uint16_t)s;
    count[0] = 0;
    return true;
}

// the lengths of the fixed codes (RFC 1951 3.2.6): 288 literal/length symbols, 32 distance symbols of 5 bits
BGZ_HD int dfl_fixed_ll_len(int s) { return s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8; }
// the smallest length of a length symbol 257..285, the smallest distance of a distance symbol 0..29
BGZ_HD int dfl_len_base(int sym)
{
    if (sym < 265) return sym - 257 + DFL_MIN_MATCH;
    if (sym == 285) return DFL_MAX_MATCH;
    return DFL_MIN_MATCH + ((4 + ((sym - 265) & 3)) << dfl_len_extra_bits(sym));
}
BGZ_HD int dfl_dist_base(int sym) { return sym < 4 ? sym + 1 : 1 + ((2 + (sym & 1)) << dfl_dist_extra_bits(sym)); }
