// bgzf_deflate.h -- the format side of BGZF compression on the device: DEFLATE (RFC 1951) symbol tables, length-limited
// Huffman code construction, the run-length coding of code lengths, bit order, and CRC-32 arithmetic (RFC 1952).  Used by
// k_bgzf_deflate / k_bgzf_gather next to the BAM kernels (k_post.hip); everything here is plain C++ that compiles for the
// device, the emulation build and the host.
//
// A BGZF file (SAM specification 4.1) is a series of gzip members, each of at most 0xff00 input bytes and at most 64 KiB:
//   bytes 0..17   1f 8b 08 04, MTIME 0, XFL 0, OS ff, XLEN 6, 'B' 'C' 02 00, BSIZE = member size - 1 (16 bits)
//   deflate data  one block with BFINAL set
//   CRC-32 of the input, ISIZE = number of input bytes (both little-endian)
// The rules the kernels are bound to:
//   block cut     member i holds input [i * 0xff00, min(n, (i + 1) * 0xff00)): the host framer's cut (sam_writer.cpp)
//   matches       length 3..258, distance 1..32 768, never reaching before the member's first byte (members stand alone)
//   tokens        32 bits each: a literal is its byte; a match is 1 << 31 | (length - 3) << 15 | (distance - 1)
//   block type    dynamic Huffman (BTYPE 2) when it is smaller than a stored block (BTYPE 0, n + 5 bytes), else stored: a
//                 member is never larger than n + 31 bytes.  The size of the dynamic block is computed exactly first.
//   code lengths  Huffman lengths from the two-queue construction over the symbols sorted by (frequency, symbol); lengths over
//                 the limit (15; 7 for the code-length alphabet) are folded to the limit and the Kraft sum is repaired by
//                 lengthening the deepest shorter code, one unit at a time; the sorted symbols then take the lengths longest
//                 first.  An alphabet with fewer than two used symbols gets two (symbols 0 and 1), so every code is complete.
//   codes         canonical (RFC 1951 3.2.2), stored bit-reversed: Huffman codes go into the stream most significant bit
//                 first, everything else least significant bit first
//   CRC-32        reflected polynomial 0xEDB88320.  A slice's register is advanced over the bytes that follow it by a
//                 multiplication with x^(8 * bytes) mod P, so slices are computed independently and combined by XOR.
// Nothing in the result depends on the order in which lanes run: the bytes are a function of the input alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define BGZ_HD static __host__ __device__ inline

enum { BGZF_IN = 0xff00,                 // input bytes per member at most
       BGZF_SLOT = 0xff00 + 32,          // bytes of the fixed slot a member is written into (>= n + 31, a multiple of 4)
       BGZF_HEAD = 18, BGZF_TAIL = 8, BGZF_EOF_BYTES = 28 };
enum { DFL_NLL = 286, DFL_ND = 30, DFL_NCL = 19, DFL_EOB = 256, DFL_MIN_MATCH = 3, DFL_MAX_MATCH = 258, DFL_MAX_DIST = 32768,
       DFL_LL_BITS = 15, DFL_CL_BITS = 7 };
#define DFL_TOK_MATCH 0x80000000u

// the EOF block: an empty member (a fixed-Huffman block holding only the end-of-block symbol)
BGZ_HD uint8_t bgzf_eof_byte(int i)
{
    switch (i) { case 0: return 0x1f; case 1: return 0x8b; case 2: return 8; case 3: return 4; case 9: return 0xff; case 10: return 6;
                 case 12: return 'B'; case 13: return 'C'; case 14: return 2; case 16: return 0x1b; case 18: return 3; }
    return 0;
}

BGZ_HD uint32_t dfl_tok_match(int len, int dist) { return DFL_TOK_MATCH | (uint32_t)(len - DFL_MIN_MATCH) << 15 | (uint32_t)(dist - 1); }
BGZ_HD int dfl_tok_len(uint32_t t) { return (int)(t >> 15 & 0xff) + DFL_MIN_MATCH; }
BGZ_HD int dfl_tok_dist(uint32_t t) { return (int)(t & 0x7fff) + 1; }

BGZ_HD int dfl_log2(uint32_t v) { return 31 - __builtin_clz(v); }        // v > 0

// RFC 1951 3.2.5: the length symbol (257..285) of a match length, the number of its extra bits and their value
BGZ_HD int dfl_len_sym(int len)
{
    const int l = len - DFL_MIN_MATCH;
    if (l < 8) return 257 + l;
    if (len == DFL_MAX_MATCH) return 285;
    const int eb = dfl_log2((uint32_t)l) - 2;
    return 257 + 4 * eb + 4 + (l >> eb & 3);
}
BGZ_HD int dfl_len_extra_bits(int sym) { return sym < 265 || sym == 285 ? 0 : (sym - 261) >> 2; }
BGZ_HD int dfl_len_extra(int len, int eb) { return (len - DFL_MIN_MATCH) & ((1 << eb) - 1); }
// the distance symbol (0..29) of a distance, its extra bits and their value
BGZ_HD int dfl_dist_sym(int dist)
{
    const int d = dist - 1;
    if (d < 4) return d;
    const int k = dfl_log2((uint32_t)d);
    return 2 * k + (d >> (k - 1) & 1);
}
BGZ_HD int dfl_dist_extra_bits(int sym) { return sym < 4 ? 0 : (sym >> 1) - 1; }
BGZ_HD int dfl_dist_extra(int dist, int eb) { return (dist - 1) & ((1 << eb) - 1); }

// the order in which the lengths of the code-length alphabet are sent (RFC 1951 3.2.7)
// (i = 0..2: 16, 17, 18; i = 3..18: 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15 as nibbles of the constant, lowest first)
BGZ_HD int dfl_cl_order(int i) { return i < 3 ? 16 + i : (int)(0xf1e2d3c4b5a69780ull >> (4 * (i - 3)) & 15); }

BGZ_HD uint32_t dfl_reverse(uint32_t code, int len)
{
    uint32_t r = 0;
    for (int i = 0; i < len; ++i) r |= (code >> i & 1u) << (len - 1 - i);
    return r;
}

// position of symbol s among the used symbols sorted by (frequency, symbol); any lane may compute any symbol's
BGZ_HD int dfl_rank(const int* freq, int n, int s)
{
    const int f = freq[s];
    int r = 0;
    for (int t = 0; t < n; ++t) { const int g = freq[t]; r += g > 0 && (g < f || (g == f && t < s)); }
    return r;
}

// Code lengths of the m >= 2 used symbols order[0..m) (ascending by frequency) into len[] (the unused ones are zeroed by the
// caller), none longer than max_bits; count[1..max_bits] receives the number of codes of each length.  One lane.
// w: m words, par: 2 m entries of scratch.
BGZ_HD void dfl_code_lengths(const int* freq, const uint16_t* order, int m, int max_bits, uint8_t* len, int* count, uint32_t* w, uint16_t* par)
{
    // two queues: the sorted leaves and the internal nodes, which are created in ascending order of weight
    int li = 0, ni = 0;
    for (int j = 0; j < m - 1; ++j) {
        uint32_t sum = 0;
        for (int k = 0; k < 2; ++k) {
            if (li < m && (ni >= j || (uint32_t)freq[order[li]] <= w[ni])) { sum += (uint32_t)freq[order[li]]; par[li++] = (uint16_t)j; }
            else { sum += w[ni]; par[m + ni++] = (uint16_t)j; }
        }
        w[j] = sum;
    }
    // depths from the root down (w now holds depths), leaves folded to the limit
    for (int b = 0; b <= max_bits; ++b) count[b] = 0;
    w[m - 2] = 0;
    for (int j = m - 3; j >= 0; --j) w[j] = w[par[m + j]] + 1;
    for (int i = 0; i < m; ++i) { int d = (int)w[par[i]] + 1; if (d > max_bits) d = max_bits; ++count[d]; }
    // repair the Kraft sum: in units of 2^-max_bits it must be 2^max_bits
    uint32_t total = 0;
    for (int b = 1; b <= max_bits; ++b) total += (uint32_t)count[b] << (max_bits - b);
    while (total > 1u << max_bits) {
        --count[max_bits];
        for (int b = max_bits - 1; b > 0; --b) if (count[b]) { --count[b]; count[b + 1] += 2; break; }
        --total;
    }
    // the rarest symbols take the longest codes
    int at = 0;
    for (int b = max_bits; b >= 1; --b) for (int k = 0; k < count[b]; ++k) len[order[at++]] = (uint8_t)b;
}

// canonical codes of len[0..n) into tab[s] = bit-reversed code | length << 16 (0 for unused symbols).  One lane.
BGZ_HD void dfl_assign_codes(const uint8_t* len, int n, int max_bits, const int* count, uint32_t* tab)
{
    uint32_t next[16];
    uint32_t code = 0;
    next[0] = 0;
    for (int b = 1; b <= max_bits; ++b) { code = (code + (b > 1 ? (uint32_t)count[b - 1] : 0u)) << 1; next[b] = code; }
    for (int s = 0; s < n; ++s) { const int l = len[s]; tab[s] = l ? dfl_reverse(next[l]++, l) | (uint32_t)l << 16 : 0u; }
}

// RFC 1951 3.2.7: the lengths seq[0..total) as symbols of the code-length alphabet, greedily: 18 (11..138 zeros), 17 (3..10
// zeros), 16 (the previous length 3..6 more times), else the length itself.  out[k] = symbol | extra value << 8 -> the number
// of symbols.  One lane; out has room for total entries.
BGZ_HD int dfl_rle_lengths(const uint8_t* seq, int total, uint16_t* out)
{
    int k = 0, i = 0;
    while (i < total) {
        const int v = seq[i];
        int run = 1;
        while (i + run < total && seq[i + run] == v) ++run;
        i += run;
        if (v == 0) {
            while (run >= 11) { const int r = run < 138 ? run : 138; out[k++] = (uint16_t)(18 | (r - 11) << 8); run -= r; }
            if (run >= 3) { out[k++] = (uint16_t)(17 | (run - 3) << 8); run = 0; }
        } else {
            out[k++] = (uint16_t)v; --run;
            while (run >= 3) { const int r = run < 6 ? run : 6; out[k++] = (uint16_t)(16 | (r - 3) << 8); run -= r; }
        }
        for (; run > 0; --run) out[k++] = (uint16_t)v;
    }
    return k;
}
BGZ_HD int dfl_cl_extra_bits(int sym) { return sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0; }

// ---- CRC-32, reflected: bit 31 of a word is the coefficient of x^0
#define BGZ_CRC_POLY 0xEDB88320u
BGZ_HD uint32_t bgz_crc_table_entry(uint32_t i) { for (int k = 0; k < 8; ++k) i = i & 1 ? BGZ_CRC_POLY ^ (i >> 1) : i >> 1; return i; }
BGZ_HD uint32_t bgz_crc_mul(uint32_t a, uint32_t b)                   // a * b mod P
{
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) { if (a & (0x80000000u >> i)) p ^= b; b = b & 1 ? (b >> 1) ^ BGZ_CRC_POLY : b >> 1; }
    return p;
}
BGZ_HD uint32_t bgz_crc_xpow8(uint32_t n_bytes)                       // x^(8 * n_bytes) mod P
{
    uint32_t r = 0x80000000u, b = 0x00800000u;                        // 1, x^8
    for (; n_bytes; n_bytes >>= 1) { if (n_bytes & 1) r = bgz_crc_mul(r, b); b = bgz_crc_mul(b, b); }
    return r;
}
