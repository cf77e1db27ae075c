"""Compressed FASTQ in: BGZF members inflated on the device (csrc/bgzf_inflate.h, k_bgzf_inflate in csrc/k_post.hip, the calls
bwamem_hip_bgzf_inflate_device / bwamem_hip_batch_upload_fastq_gz / bwamem_hip_align_fastq_gz_to_marked_bam, BwaMemAligner's mirror).
Nothing has a tolerance.  Python's zlib is the judge: every member the tests build is first put to zlib.decompressobj(-15); what it
accepts must come out byte-identical to gzip.decompress, what it refuses must be refused with the smallest offending member.  The
streams zlib would never emit are written by a small bit-writer here.  Through the gz entry a FASTQ text gives exactly the batch
bwamem_hip_batch_upload_fastq gives for the plain text.
CPU suite: the emulation build runs the kernel, and a stand-alone driver runs the same cases under AddressSanitizer + UBSan.  GPU suite
(-m gpu): the same on the device, the medium genome, and the device's bytes against the emulation build's."""
import ctypes
import gzip
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import bwalib as B
from test_bam_dup import DupCounts, bindd
from test_bam_quals import RG_LINE, Batch
from test_bam_writer import EOF_BLOCK, _take, bgzf as host_bgzf, have_zlib
from test_bgzf_device import fibonacci_block, zdev
from test_fastq_device import fastq_text, pair_set, small_set, upload

CUTS = (1, 7, 317, 4096, 0xff00)


# ------------------------------------------------------------------------------------------ bindings
def bindgz(lib):
    d = bindd(lib)
    if getattr(d, "_gz_bound", False):
        return d
    vp, sz, cp, ci, i64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_int, ctypes.c_int64
    d.bwamem_hip_bgzf_inflate_device.restype = vp
    d.bwamem_hip_bgzf_inflate_device.argtypes = [vp, cp, sz, ctypes.POINTER(sz), ctypes.POINTER(i64)]
    d.bwamem_hip_batch_upload_fastq_gz.restype = vp
    d.bwamem_hip_batch_upload_fastq_gz.argtypes = [vp, cp, sz, cp, sz, ctypes.POINTER(i64), ctypes.POINTER(i64)]
    d.bwamem_hip_align_fastq_gz_to_marked_bam.argtypes = [vp, vp, vp, cp, sz, cp, sz, cp, ci, ci, ci, ci, ci, ctypes.POINTER(DupCounts)]
    d._gz_bound = True
    return d


def inflate(lib, h, z):
    """-> (bytes or None, bad_member)"""
    d = bindgz(lib)
    sz, bad = ctypes.c_size_t(77), ctypes.c_int64(-7)
    p = d.bwamem_hip_bgzf_inflate_device(h, z, len(z), ctypes.byref(sz), ctypes.byref(bad))
    if not p:
        assert sz.value == 0
        return None, bad.value
    return _take(lib, p, sz.value), bad.value


def upload_gz(lib, h, z1, z2=None):
    d = bindgz(lib)
    bad, bm = ctypes.c_int64(-7), ctypes.c_int64(-7)
    b = d.bwamem_hip_batch_upload_fastq_gz(h, z1, len(z1), z2, len(z2) if z2 is not None else 0, ctypes.byref(bad), ctypes.byref(bm))
    return b, bad.value, bm.value


# ------------------------------------------------------------------------------------------ members, by zlib and by hand
def member(deflate, data=None, extra=b"", crc=None, isize=None):
    """a BGZF member around a deflate area; extra: subfields in front of BC"""
    crc = zlib.crc32(data) if crc is None else crc
    isize = len(data) if isize is None else isize
    xlen = len(extra) + 6
    size = 12 + xlen + len(deflate) + 8
    assert size <= 65536
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", xlen) + extra + b"BC\x02\x00" + struct.pack("<H", size - 1) + deflate
            + struct.pack("<II", crc & 0xffffffff, isize))


def deflate_of(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=(), flush=zlib.Z_SYNC_FLUSH):
    o = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    out, at = b"", 0
    for f in flush_at:
        out += o.compress(data[at:f]) + o.flush(flush)
        at = f
    return out + o.compress(data[at:]) + o.flush()


def zmember(data, level=6, **kw):
    return member(deflate_of(data, level, **kw), data)


def bgzf_cut(text, cut, level=6, eof=True):
    return b"".join(zmember(text[at:at + cut], level) for at in range(0, len(text), cut)) + (EOF_BLOCK if eof else b"")


def zlib_verdict(m):
    """zlib's verdict on one member: the inflated bytes, or None when it is refused (the rule of csrc/bgzf_inflate.h)"""
    xlen, = struct.unpack_from("<H", m, 10)
    area = m[12 + xlen:len(m) - 8]
    crc, isize = struct.unpack_from("<II", m, len(m) - 8)
    o = zlib.decompressobj(-15)
    try:
        raw = o.decompress(area)
    except zlib.error:
        return None
    if not o.eof or o.unused_data != b"" or len(raw) != isize or zlib.crc32(raw) != crc:
        return None
    return raw


class Bits:
    """a deflate bit stream: values lowest bit first, Huffman codes highest bit first"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, nb):
        self.acc |= (v & ((1 << nb) - 1)) << self.n
        self.n += nb
        while self.n >= 8:
            self.out.append(self.acc & 0xff)
            self.acc >>= 8
            self.n -= 8
        return self

    def code(self, c):
        code, length = c
        return self.put(int(format(code, "0%db" % length)[::-1], 2), length)

    def align(self):
        return self.put(0, (8 - self.n) & 7)

    def raw(self, data):
        assert self.n == 0
        self.out += data
        return self

    def bytes(self):
        return bytes(self.align().out)


def canon(lens):
    """{symbol: (code, length)} of the canonical code, complete or not"""
    out, code = {}, 0
    for length in range(1, 16):
        for s, l in enumerate(lens):
            if l == length:
                out[s] = (code, length)
                code += 1
        code <<= 1
    return out


FIXED_LL = canon([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_D = canon([5] * 32)
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0] * 4 + [e for e in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_LENS = [4] * 13 + [5] * 6                         # a complete code over all 19 symbols: 13 / 16 + 6 / 32


def put_tokens(bits, tokens, ll, dd):
    """tokens: a byte value, ('m', length, distance), ('ll', symbol) or ('d', symbol) for a bare code; then nothing is appended"""
    for t in tokens:
        if isinstance(t, int):
            bits.code(ll[t])
        elif t[0] == "ll":
            bits.code(ll[t[1]])
        elif t[0] == "d":
            bits.code(dd[t[1]])
        else:
            _, length, dist = t
            ls = max(i for i in range(29) if LEN_BASE[i] <= length and (i < 28 or length == 258))
            bits.code(ll[257 + ls]).put(length - LEN_BASE[ls], LEN_EXTRA[ls])
            ds = max(i for i in range(30) if DIST_BASE[i] <= dist)
            bits.code(dd[ds]).put(dist - DIST_BASE[ds], DIST_EXTRA[ds])
    return bits


def rle(seq):
    """the lengths as (symbol, extra value, extra bits) of the code-length alphabet; runs are coded over the whole sequence, so a
    repeat may run from the literal/length lengths into the distance lengths"""
    out, i = [], 0
    while i < len(seq):
        v, run = seq[i], 1
        while i + run < len(seq) and seq[i + run] == v:
            run += 1
        i += run
        if v == 0:
            while run >= 11:
                r = min(run, 138); out.append((18, r - 11, 7)); run -= r
            if run >= 3:
                out.append((17, run - 3, 3)); run = 0
        else:
            out.append((v, 0, 0)); run -= 1
            while run >= 3:
                r = min(run, 6); out.append((16, r - 3, 2)); run -= r
        out += [(v, 0, 0)] * run
    return out


def dyn_header(bits, final, ll_lens, d_lens, syms=None, hlit=None, hdist=None):
    """BFINAL, BTYPE 2 and the code lengths; syms: the code-length symbols to send instead of rle(ll_lens + d_lens)"""
    hlit = len(ll_lens) if hlit is None else hlit
    hdist = len(d_lens) if hdist is None else hdist
    bits.put(final, 1).put(2, 2).put(hlit - 257, 5).put(hdist - 1, 5).put(19 - 4, 4)
    for s in CL_ORDER:
        bits.put(CL_LENS[s], 3)
    cl = canon(CL_LENS)
    for s, extra, nb in (rle(list(ll_lens) + list(d_lens)) if syms is None else syms):
        bits.code(cl[s]).put(extra, nb)
    return bits


def dyn_block(tokens, ll_lens, d_lens, final=1, eob=True, **kw):
    bits = dyn_header(Bits(), final, ll_lens, d_lens, **kw)
    ll, dd = canon(ll_lens), canon(d_lens)
    put_tokens(bits, tokens, ll, dd)
    if eob:
        bits.code(ll[256])
    return bits.bytes()


def fixed_block(tokens, final=1, eob=True, into=None):
    """into: a bit stream to go on with (the next block begins at the next bit); it is returned instead of the bytes"""
    bits = put_tokens((into or Bits()).put(final, 1).put(1, 2), tokens, FIXED_LL, FIXED_D)
    if eob:
        bits.code(FIXED_LL[256])
    return bits if into is not None else bits.bytes()


def ll_lens_of(d, n=258):
    lens = [0] * n
    for s, l in d.items():
        lens[s] = l
    return lens


AB = {97: 2, 98: 2, 256: 2, 257: 2}                  # a complete literal/length code: a, b, end of block, length 3


def hand_built_valid():
    """(name, member, data): streams zlib would never emit, all valid"""
    rng = np.random.default_rng(11)
    r = rng.integers(0, 256, size=32768, dtype=np.uint8).tobytes()
    far = Bits().put(0, 1).put(0, 2).align().put(32768, 16).put(32768 ^ 0xffff, 16).raw(r).bytes() + fixed_block([("m", 10, 32768)])
    out = [("distance_32768", member(far, r + r[:10]), r + r[:10]),
           ("match_reaching_the_first_byte", member(fixed_block([97, 98, 99, ("m", 3, 3), ("m", 258, 6)]), b"abc" * 2 + (b"abc" * 86)), b"abc" * 88),
           ("one_distance_code", member(dyn_block([97, ("m", 3, 1), 98], ll_lens_of(AB), [1]), b"aaaab"), b"aaaab"),
           ("no_distance_code", member(dyn_block([97, 98, 98, 97], ll_lens_of(AB), [0]), b"abba"), b"abba"),
           ("repeat_16_into_the_distance_lengths", member(dyn_block([97, 98, ("m", 3, 2), ("m", 3, 4)], ll_lens_of(AB), [2, 2, 2, 2]), b"abababab"), b"abababab"),
           ("empty_fixed_block_then_stored", member(fixed_block([], final=0, into=Bits()).put(1, 1).put(0, 2).align().put(2, 16).put(0xfffd, 16).raw(b"hi").bytes(), b"hi"), b"hi"),
           ("only_end_of_block_code", member(dyn_block([], ll_lens_of({256: 1}, 257), [0]), b""), b"")]
    syms = rle(ll_lens_of(AB) + [2, 2, 2, 2])
    assert syms[-1] == (16, 2, 2) and syms[-2][0] == 2, "the repeat must start in the literal/length lengths and end in the distance lengths"
    for name, m, data in out:
        assert zlib_verdict(m) == data, "fixture drifted: zlib must accept " + name
    return out


def defective_members():
    """{rule: member}: one member per refusal rule of csrc/bgzf_inflate.h, each refused by zlib"""
    good = b"acgtacgtacgtnnnn" * 9
    dfl = deflate_of(good)
    stored = Bits().put(1, 1).put(0, 2).align().put(4, 16).put(0xfffb, 16).raw(b"abcd").bytes()
    no_prev = [(16, 0, 2)] + rle(ll_lens_of(AB)[3:] + [1, 1])
    overrun = rle(ll_lens_of(AB) + [1])[:-1] + [(18, 0, 7)]
    d = {"btype_3": member(Bits().put(1, 1).put(3, 2).bytes(), b""),
         "over_subscribed": member(dyn_block([97], ll_lens_of({97: 1, 98: 1, 256: 1}, 257), [1, 1]), b"a"),
         "incomplete_literal_code": member(dyn_block([97], ll_lens_of({97: 2, 98: 2, 256: 2}, 257), [1, 1]), b"a"),
         "incomplete_distance_code": member(dyn_block([97], ll_lens_of(AB), [2, 2, 2]), b"a"),
         "repeat_with_no_previous_length": member(dyn_block([97], ll_lens_of(AB), [1, 1], syms=no_prev), b"a"),
         "repeat_overruns_the_lengths": member(dyn_block([97], ll_lens_of(AB), [1], syms=overrun), b"a"),
         "no_end_of_block_code": member(dyn_block([97], ll_lens_of({97: 1, 98: 1}, 257), [1, 1], eob=False), b"a"),
         "hlit_287": member(dyn_block([97], ll_lens_of(AB, 287), [1, 1]), b"a"),
         "symbol_286": member(fixed_block([97, ("ll", 286)]), b"a"),
         "distance_symbol_30": member(fixed_block([97, ("ll", 257), ("d", 30)]), b"aaaa"),
         "distance_before_the_first_byte": member(fixed_block([97, ("m", 3, 2)]), b"aaaa"),
         "output_beyond_isize": member(dfl, good[:-1]),
         "output_short_of_isize": member(dfl, good + b"a", crc=zlib.crc32(good)),
         "input_exhausted": member(dfl[:-2], good),
         "unused_byte_before_the_trailer": member(dfl + b"\0", good),
         "crc_mismatch": member(dfl, good, crc=zlib.crc32(good) ^ 0x100),
         "stored_len_nlen": member(stored[:3] + b"\xfa" + stored[4:], b"abcd"),
         "bad_code_of_a_one_code_alphabet": member(dyn_block([97, ("ll", 257)], ll_lens_of(AB), [1], eob=False) + b"\xff\xff", b"aaaa")}
    assert zlib_verdict(member(stored, b"abcd")) == b"abcd"
    for rule, m in d.items():
        assert zlib_verdict(m) is None, "fixture drifted: zlib must refuse " + rule
    return d


_valid_cache = {}


def valid_set(lib, h):
    """(name, stream, expected text): about 200 members in all.  The library's own compressors make part of it, so it takes a
    library; their output does not depend on which build made it (test_bgzf_device.py)."""
    if "set" in _valid_cache:
        return _valid_cache["set"]
    rng = np.random.default_rng(7)
    reads = [bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=150)) for _ in range(700)]
    quals = [bytes(rng.choice(np.frombuffer(b"#5AF", dtype=np.uint8), size=150, p=[0.05, 0.15, 0.3, 0.5])) for _ in reads]
    fq = fastq_text(reads, ["M01:%d:FC:%d:%d" % (i % 8, 1000 + 7 * i, 3 * i) for i in range(len(reads))], quals)
    noise = rng.integers(0, 256, size=70000, dtype=np.uint8).tobytes()
    full = (fq * 2)[:65536]
    out = [("empty_stream", b""), ("eof_alone", EOF_BLOCK), ("one_byte", zmember(b"x")), ("one_byte_and_eof", zmember(b"x") + EOF_BLOCK),
           ("eof_between_members", zmember(b"ab") + EOF_BLOCK + zmember(b"cd") + EOF_BLOCK + EOF_BLOCK + zmember(b"e")),
           ("exactly_65536", zmember(full) + EOF_BLOCK), ("equal_bytes_65536", zmember(b"\x41" * 65536)), ("fibonacci", zmember(fibonacci_block(), 9)),
           ("fixed_codes", b"".join(zmember(fq[at:at + 20000], 6, strategy=zlib.Z_FIXED) for at in range(0, 60000, 20000))),
           ("sync_flushes", zmember(fq[:30000], 6, flush_at=(1, 5000, 5000, 17000))),
           ("full_flushes", zmember(fq[:30000], 1, flush_at=(100, 9000, 29999), flush=zlib.Z_FULL_FLUSH)),
           ("foreign_subfield", member(deflate_of(fq[:5000]), fq[:5000], extra=b"XY\x03\x00abc") + member(deflate_of(b"z"), b"z", extra=b"BC\x01\x00q" + b"AB\0\0")),
           ("noise", bgzf_cut(noise, 0xff00, 6)), ("own_device", zdev(lib, h, fq[:200000] + noise[:3000], True)), ("own_device_empty", zdev(lib, h, b"", True))]
    for level in (0, 1, 6, 9):
        out.append(("level_%d" % level, bgzf_cut(fq[:250000], 0xff00 if level == 0 else 8000 + 1111 * level, level)))
    out.append(("stored_ff00", bgzf_cut(fq[1000:1000 + 0xff00], 0xff00, 0, eof=False)))
    if have_zlib():
        out += [("own_host_level_%d" % lv, host_bgzf(lib, fq[:150000] + noise[:2000], lv, 2, True)) for lv in (0, 1)]
    out += [("small_cuts_%d" % c, bgzf_cut(fq[:40 * c if c < 4096 else 3 * c + 5], c, 6)) for c in (1, 7, 317)]
    out += [("hand_" + name, m) for name, m, _ in hand_built_valid()]
    out.append(("hand_all", b"".join(m for _, m, _ in hand_built_valid()) + EOF_BLOCK))
    res = [(name, z, gzip.decompress(z)) for name, z in out]
    n_members = sum(z.count(b"\x1f\x8b\x08\x04") for _, z, _ in res)
    assert 150 <= n_members <= 400, n_members
    _valid_cache["set"] = res
    return res


def refusal_streams():
    """(what, stream, bad_member)"""
    good = [zmember(b"member %d\n" % i * (50 + i)) for i in range(5)]
    out = []
    bad = defective_members()
    for rule, m in bad.items():
        out.append((rule + " as member 2 of 5", b"".join(good[:2] + [m] + good[3:]), 2))
        out.append((rule + " as member 0", b"".join([m] + good[1:]) + EOF_BLOCK, 0))
    a, b = bad["crc_mismatch"], bad["distance_before_the_first_byte"]
    out += [("two defective members", b"".join([good[0], a, good[2], b, good[4]]), 1), ("two defective members, the other way round", b"".join([good[0], b, good[2], a, good[4]]), 1),
            ("the last of many", bgzf_cut(b"0123456789" * 3000, 100, 1, eof=False) + a, 300)]
    # errors at the walk
    g = b"".join(good)
    big = member(deflate_of(b""), b"", isize=65537)
    out += [("ISIZE over 65536", good[0] + big + good[1], 1), ("a BSIZE that runs past the data", good[0] + good[1][:-1], 1), ("a truncated last member", g + good[0][:20], 5),
            ("a truncated header", g + good[0][:9], 5), ("a bad magic in mid-stream", good[0] + b"\x1f\x8b\x08\x00" + good[1][4:], 1), ("text in mid-stream", good[0] + b"@read\n", 1),
            ("a plain gzip member in mid-stream", good[0] + gzip.compress(b"x"), 1)]
    return out


# ------------------------------------------------------------------------------------------ the checks
def check_valid(lib, h):
    """A: every stream inflates to what gzip makes of it, twice -> {name: bytes}"""
    got = {}
    for name, z, want in valid_set(lib, h):
        raw, bad = inflate(lib, h, z)
        assert raw is not None and bad == -1, (name, bad)
        assert raw == want, name
        assert inflate(lib, h, z)[0] == raw, "two runs differ: " + name
        got[name] = raw
    return got


def check_refusals(lib, h):
    """B"""
    for what, z, want in refusal_streams():
        raw, bad = inflate(lib, h, z)
        assert raw is None and bad == want, (what, bad)
    raw, bad = inflate(lib, h, gzip.compress(b"plain gzip"))
    assert raw is None and bad == -1, "a plain gzip stream is no BGZF"
    raw, bad = inflate(lib, h, b"@text\n")
    assert raw is None and bad == -1
    d = bindgz(lib)
    assert not d.bwamem_hip_bgzf_inflate_device(None, EOF_BLOCK, 28, None, None)
    p = d.bwamem_hip_bgzf_inflate_device(h, EOF_BLOCK, 28, None, None)
    assert p, "pBytes and bad_member may be NULL"
    lib._free(p)


def gz_path(lib, h, opts, z1, z2, paired, pes, rg=None):
    b, bad, bm = upload_gz(lib, h, z1, z2)
    assert b and bad == -1 and bm == -1, "upload_fastq_gz refused the streams (bad_record %d, bad_member %d)" % (bad, bm)
    bt = Batch(lib, h, opts, None, pes, b=b)
    try:
        if rg is not None:
            assert bt.set_rg(rg) == 0
        return bt.resp, bt.encode(paired)
    finally:
        bt.free()


_plain_cache = {}


def plain_path(lib, h, opts, t1, t2, paired, pes, rg=None):
    key = (lib.path, h, t1, t2, paired, rg)
    if key not in _plain_cache:
        b, bad = upload(lib, h, t1, t2)
        assert b
        bt = Batch(lib, h, opts, None, pes, b=b)
        try:
            if rg is not None:
                assert bt.set_rg(rg) == 0
            _plain_cache[key] = (bt.resp, bt.encode(paired))
        finally:
            bt.free()
    return _plain_cache[key]


def texts(seqs):
    reads, names, quals = small_set(seqs)
    pairs, pnames, pquals = pair_set(seqs)
    po_suffix = [(b"/1", b"/2")[i & 1] for i in range(len(pairs))]
    return {"se": fastq_text(reads, names, quals), "se_crlf": fastq_text(reads, names, quals, eol=b"\r\n", final=False, plus=[b"x" * (i % 3) for i in range(len(reads))]),
            "inter": fastq_text(pairs, pnames, pquals, suffix=po_suffix), "p1": fastq_text(pairs[0::2], pnames[0::2], pquals[0::2]),
            "p2": fastq_text(pairs[1::2], pnames[1::2], pquals[1::2], eol=b"\r\n"),
            "bad_plus": fastq_text(reads, names, quals).replace(b"\n+\n", b"\n-\n"), "bad_lines": fastq_text(reads, names, quals)[:-80],
            "bad_qual": fastq_text(reads[:3], names[:3], [quals[0], quals[1][:-1], quals[2]])}


def pe_opts(lib):
    return B.set_opt(lib.default_options(), flag=B.MEM_F_PE), B.pack_pestat(150, 450, 300.0, 30.0)


def check_fastq_cuts(lib, h, seqs, cuts=CUTS):
    """C: single-end, interleaved and two files, cut into members at every size; names, '+' lines and CR LFs straddle members"""
    t = texts(seqs)
    so = lib.default_options()
    po, pes = pe_opts(lib)
    for cut in cuts:
        for name in ("se", "se_crlf"):
            assert gz_path(lib, h, so, bgzf_cut(t[name], cut), None, False, None) == plain_path(lib, h, so, t[name], None, False, None), (name, cut)
        assert gz_path(lib, h, po, bgzf_cut(t["inter"], cut, eof=False), None, True, pes) == plain_path(lib, h, po, t["inter"], None, True, pes), cut
        other = CUTS[(CUTS.index(cut) + 2) % len(CUTS)]
        assert gz_path(lib, h, po, bgzf_cut(t["p1"], cut), bgzf_cut(t["p2"], other), True, pes) == plain_path(lib, h, po, t["p1"], t["p2"], True, pes), cut
    b, bad, bm = upload_gz(lib, h, b"")
    assert b and bad == -1 and bm == -1, "an empty stream holds no record"
    bindgz(lib).bwamem_hip_batch_free(b)
    b, bad, bm = upload_gz(lib, h, EOF_BLOCK, EOF_BLOCK)
    assert b, "two empty texts"
    bindgz(lib).bwamem_hip_batch_free(b)


def check_fastq_errors(lib, h, seqs):
    """C: bad_record as for the plain text; bad_member counts the first stream's members, then the second's"""
    t = texts(seqs)
    for name in ("bad_plus", "bad_lines", "bad_qual"):
        b0, want = upload(lib, h, t[name])
        assert not b0
        for cut in (317, 0xff00):
            b, bad, bm = upload_gz(lib, h, bgzf_cut(t[name], cut))
            assert not b and bad == want and bm == -1, (name, cut, bad, bm)
    b0, want = upload(lib, h, t["p1"], t["p2"].replace(b"\r\n+\r\n", b"\r\n-\r\n", 3).replace(b"\r\n-\r\n", b"\r\n+\r\n", 2))
    b, bad, bm = upload_gz(lib, h, bgzf_cut(t["p1"], 317), bgzf_cut(t["p2"].replace(b"\r\n+\r\n", b"\r\n-\r\n", 3).replace(b"\r\n-\r\n", b"\r\n+\r\n", 2), 7))
    assert not b0 and not b and bad == want == 5 and bm == -1
    broken = defective_members()["crc_mismatch"]
    z1 = bgzf_cut(t["p1"], 317)
    n1 = z1.count(b"\x1f\x8b\x08\x04")
    z2 = bgzf_cut(t["p2"], 317, eof=False)
    size0 = size_of(z2, 0)
    assert n1 > 3
    b, bad, bm = upload_gz(lib, h, z1[:size_of(z1, 0)] + broken + z1[size_of(z1, 0):], z2)
    assert not b and bad == -1 and bm == 1, bm
    b, bad, bm = upload_gz(lib, h, z1, broken + z2[size0:])
    assert not b and bad == -1 and bm == n1, ("the first stream's member count offsets the second's", bm, n1)
    b, bad, bm = upload_gz(lib, h, z1, z2[:size0] + broken)
    assert not b and bm == n1 + 1
    b, bad, bm = upload_gz(lib, h, z1, z2[:-3])
    assert not b and bad == -1 and bm == n1 + z2.count(b"\x1f\x8b\x08\x04") - 1, ("a truncated member at the walk", bm)
    d = bindgz(lib)
    assert not d.bwamem_hip_batch_upload_fastq_gz(None, z1, len(z1), None, 0, None, None)
    b = d.bwamem_hip_batch_upload_fastq_gz(h, z1, len(z1), None, 0, None, None)
    assert b, "bad_record and bad_member may be NULL"
    d.bwamem_hip_batch_free(b)


def size_of(z, at):
    return struct.unpack_from("<H", z, at + 16)[0] + 1


def check_plain_gzip(lib, h, seqs):
    """C: gzip's own streams go through the host's libz and give the same batch"""
    if not have_zlib():
        return False                                                  # (no libz.so.1 on this machine: the caller says so)
    t = texts(seqs)
    so = lib.default_options()
    po, pes = pe_opts(lib)
    want = plain_path(lib, h, so, t["se"], None, False, None)
    assert gz_path(lib, h, so, gzip.compress(t["se"]), None, False, None) == want
    half = t["se"].index(b"\n", len(t["se"]) // 2) - 3
    assert gz_path(lib, h, so, gzip.compress(t["se"][:half], 1) + gzip.compress(t["se"][half:], 9), None, False, None) == want, "two concatenated gzip members"
    assert gz_path(lib, h, po, gzip.compress(t["p1"]), bgzf_cut(t["p2"], 317), True, pes) == plain_path(lib, h, po, t["p1"], t["p2"], True, pes), "one stream of each kind"
    z = gzip.compress(t["se"])
    for what, broken in (("truncated", z[:-5]), ("a flipped bit", z[:40] + bytes([z[40] ^ 4]) + z[41:]), ("garbage behind it", z + b"@x\n")):
        b, bad, bm = upload_gz(lib, h, broken)
        assert not b and bad == -1 and bm == -1, what
    b, bad, bm = upload_gz(lib, h, gzip.compress(t["bad_qual"]))
    assert not b and bad == 1 and bm == -1
    b, bad, bm = upload_gz(lib, h, t["se"])
    assert not b and bad == -1 and bm == -1, "plain text is not taken by the gz entry"
    return True


def marked_file(lib, h, opts, fn, a1, a2, rg, sort, tmpdir, tag, pes, tail):
    """tail: what follows write_header in fn's parameters, with the counts in the place of True"""
    d = bindgz(lib)
    ob = ctypes.create_string_buffer(bytes(opts), B.OPT_SIZE)
    pb = ctypes.create_string_buffer(pes, len(pes)) if pes is not None else None
    path, bpath = os.path.join(tmpdir, tag + ".bam"), os.path.join(tmpdir, tag + ".bai")
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    fb = os.open(bpath, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644) if sort else -1
    counts = DupCounts()
    try:
        rc = fn(h, ob, pb, a1, len(a1), a2, len(a2) if a2 is not None else 0, rg, 1 if sort else 0, fd, fb, 1, *[ctypes.byref(counts) if x is True else x for x in tail])
    finally:
        os.close(fd)
        if fb >= 0:
            os.close(fb)
    return rc, open(path, "rb").read(), open(bpath, "rb").read() if sort else None, bytes(counts)


def check_file_call(lib, h, seqs, tmpdir):
    """C: the file call writes the two files of the plain-text call, byte for byte"""
    d = bindgz(lib)
    t = texts(seqs)
    so = lib.default_options()
    po, pes = pe_opts(lib)
    for tag, opts, t1, t2, p in (("se", so, t["se"], None, None), ("pe", po, t["p1"], t["p2"], pes)):
        for sort in (True, False):
            z1, z2 = bgzf_cut(t1, 317), bgzf_cut(t2, 4096) if t2 is not None else None
            want = marked_file(lib, h, opts, d.bwamem_hip_align_fastq_to_marked_bam, t1, t2, RG_LINE, sort, tmpdir, "plain", p, (True,))
            got = marked_file(lib, h, opts, d.bwamem_hip_align_fastq_gz_to_marked_bam, z1, z2, RG_LINE, sort, tmpdir, "gz", p, (1, True))
            assert want[0] == 0 and got == want, (tag, sort)
        want = marked_file(lib, h, opts, d.bwamem_hip_align_fastq_to_bam, t1, t2, None, True, tmpdir, "plain", p, ())[:3]
        got = marked_file(lib, h, opts, d.bwamem_hip_align_fastq_gz_to_marked_bam, z1, z2, None, True, tmpdir, "gz", p, (0, None))[:3]
        assert want[0] == 0 and got == want, "marking off, counts NULL: the plain _to_bam case"
    rc, bam, _, _ = marked_file(lib, h, so, d.bwamem_hip_align_fastq_gz_to_marked_bam, bgzf_cut(t["se"], 317)[:-40], None, None, False, tmpdir, "gz", None, (1, True))
    assert rc != 0 and bam == b"", "a damaged stream writes nothing"


def run_small_cases(lib, h, seqs, tmpdir):
    check_fastq_cuts(lib, h, seqs)
    check_fastq_errors(lib, h, seqs)
    check_file_call(lib, h, seqs, tmpdir)
    check_plain_gzip(lib, h, seqs)


# ------------------------------------------------------------------------------------------ CPU suite (emulation build)
@pytest.fixture(scope="module")
def emu_index(small_genome):
    B.build_emu()
    emu = B.product_lib(emu=True)
    seqs, img = small_genome
    h = emu.open_index(img)
    yield emu, h, seqs
    emu.destroy_index(h)


def test_inflate_valid_streams(emu_index):
    emu, h, _ = emu_index
    assert len(hand_built_valid()) >= 5 and len(defective_members()) >= 13       # (each fixture is put to zlib where it is built)
    check_valid(emu, h)


def test_inflate_refuses_what_zlib_refuses(emu_index):
    emu, h, _ = emu_index
    check_refusals(emu, h)


def test_fastq_gz_member_cuts(emu_index):
    check_fastq_cuts(*emu_index)


def test_fastq_gz_errors(emu_index):
    check_fastq_errors(*emu_index)


def test_fastq_gz_plain_gzip(emu_index):
    if not check_plain_gzip(*emu_index):
        pytest.skip("no libz.so.1 on this machine")


def test_fastq_gz_file_call(emu_index, tmp_path):
    emu, h, seqs = emu_index
    check_file_call(emu, h, seqs, str(tmp_path))


def test_fastq_gz_python_mirror(emu_index, small_genome, tmp_path):
    """BwaMemAligner.alignFastqToBam with compressed bytes and with a path, and inflateBgzf, over the emulation build in a child process"""
    emu, h, seqs = emu_index
    _, img = small_genome
    t = texts(seqs)
    z = bgzf_cut(t["se"], 317)
    fq = str(tmp_path / "in.fastq.gz")
    with open(fq, "wb") as f:
        f.write(z)
    p = {k: str(tmp_path / k) for k in ("a.bam", "b.bam", "c.bam", "plain.bam")}
    r = subprocess.run([sys.executable, "-c", (
        "import sys; sys.path.insert(0, %r); import bwamem\n"
        "ix = bwamem.BwaMemIndex(%r); al = bwamem.BwaMemAligner(ix)\n"
        "z, text, p = %r, %r, %r\n"
        "al.alignFastqToBam(%r, p['a.bam'])\n"
        "al.alignFastqToBam(z, p['b.bam'])\n"
        "counts = al.alignFastqToBam(z, p['c.bam'], mark_duplicates=True)\n"
        "assert counts['unpaired_reads_examined'] > 0\n"
        "al.alignFastqToBam(text, p['plain.bam'])\n"
        "assert al.inflateBgzf(z) == text\n"
        "try:\n    al.inflateBgzf(z[:-30])\nexcept ValueError:\n    print('inflate-checked')\n"
        "try:\n    al.alignFastqToBam(z[:-30], p['a.bam'] + 'x')\nexcept RuntimeError:\n    print('gz-checked')\n"
        "al.close(); ix.close()\n") % (B.PKG, img, z, t["se"], p, fq)],
        env=dict(os.environ, LIBBWA_PATH=B.EMU_LIB), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "inflate-checked" in r.stdout and "gz-checked" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
    plain = open(p["plain.bam"], "rb").read()
    assert len(plain) > 100 and open(p["a.bam"], "rb").read() == plain and open(p["b.bam"], "rb").read() == plain
    assert len(gzip.decompress(open(p["c.bam"], "rb").read())) == len(gzip.decompress(plain))


def test_fastq_gz_sanitizers(emu_index, small_genome, tmp_path):
    """D: the A, B and C cases under AddressSanitizer + UBSan: a stand-alone driver (tests/bgzf_inflate_sanitized_driver.cpp), compiled
    here with the sanitizers and linked against the sanitized emulation build (tests/emu `make asan`), run as a program"""
    emu, h, seqs = emu_index
    B.make(os.path.join(B.ROOT, "tests", "emu"), "asan")
    _, img = small_genome
    files, manifest = {}, []

    def add(kind, data, second, val):
        name = "f%03d.bin" % len(files)
        files[name] = data
        other = "-"
        if second is not None:
            other = "g%03d.bin" % len(files)
            files[other] = second
        manifest.append("%s %s %s %d" % (kind, name, other, val))
    for name, z, want in valid_set(emu, h):
        if len(z) < 12000 or name == "hand_distance_32768":
            add("inflate", z, want, 0)
        elif name in ("exactly_65536", "equal_bytes_65536", "fibonacci", "stored_ff00", "noise", "own_device", "fixed_codes", "sync_flushes"):
            add("inflate1", z, want, 0)                              # the largest offsets, a full ISIZE, many windows: once (this build is slow)
    for what, z, want in refusal_streams():
        add("refuse", z, None, want)
    t = texts(seqs)
    for cut in (317, 0xff00):
        add("fq", bgzf_cut(t["se_crlf"], cut), t["se_crlf"], 0)
    two = b"\n".join(t["se"].split(b"\n")[:8]) + b"\n"                   # (two records, one of them with the 254-byte name)
    add("fq", bgzf_cut(two, 1), two, 0)
    add("fq2", bgzf_cut(t["p1"], 7), bgzf_cut(t["p2"], 317), 1)
    add("fq", bgzf_cut(t["inter"], 4096, eof=False), t["inter"], 1)
    if have_zlib():
        add("fq", gzip.compress(t["se"]), t["se"], 0)
    add("badrec", bgzf_cut(t["bad_plus"], 317), None, 0)
    add("badrec", bgzf_cut(t["bad_lines"], 7), None, -1)
    add("badrec", bgzf_cut(t["bad_qual"], 0xff00), None, 1)
    add("badmem2", bgzf_cut(t["p1"], 317), defective_members()["input_exhausted"] + bgzf_cut(t["p2"], 317), bgzf_cut(t["p1"], 317).count(b"\x1f\x8b\x08\x04"))
    for k, v in files.items():
        with open(str(tmp_path / k), "wb") as f:
            f.write(v)
    with open(str(tmp_path / "manifest.txt"), "w") as f:
        f.write("\n".join(manifest) + "\n")
    emu_dir = os.path.join(B.ROOT, "tests", "emu", "_build")
    exe = str(tmp_path / "bgzf_inflate_sanitized_driver")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(B.ROOT, "include"), os.path.join(B.ROOT, "tests", "bgzf_inflate_sanitized_driver.cpp"), "-o", exe,
                    "-L", emu_dir, "-lbwamem_emu_asan", "-Wl,-rpath," + emu_dir], check=True)
    r = subprocess.run([exe, img, str(tmp_path)], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0"),
                       capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "sanitized-ok %d cases" % len(manifest) in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


# ------------------------------------------------------------------------------------------ GPU suite
@pytest.mark.gpu
def test_gpu_inflate_valid_and_equals_emulation(hip_lib, small_genome):
    """A on the device, and the device's bytes are the emulation build's"""
    B.build_emu()
    emu = B.product_lib(emu=True)
    seqs, img = small_genome
    h, he = hip_lib.open_index(img), emu.open_index(img)
    try:
        got = check_valid(hip_lib, h)
        for name, z, _ in valid_set(hip_lib, h):
            assert inflate(emu, he, z)[0] == got[name], name
    finally:
        hip_lib.destroy_index(h)
        emu.destroy_index(he)


@pytest.mark.gpu
def test_gpu_inflate_refusals(hip_lib, small_genome):
    """B on the device (after the same streams have passed the sanitized driver on the CPU)"""
    seqs, img = small_genome
    h = hip_lib.open_index(img)
    try:
        check_refusals(hip_lib, h)
    finally:
        hip_lib.destroy_index(h)


@pytest.mark.gpu
def test_gpu_fastq_gz_small_cases(hip_lib, small_genome, tmp_path):
    seqs, img = small_genome
    h = hip_lib.open_index(img)
    try:
        run_small_cases(hip_lib, h, seqs, str(tmp_path))
    finally:
        hip_lib.destroy_index(h)


@pytest.mark.gpu
def test_gpu_fastq_gz_medium_single_and_paired(hip_lib, medium_genome):
    """20 000 x 150 bp, single-end and as 10 000 pairs from two streams: records equal to the plain-text path's"""
    from test_bam_quals import rand_quals
    seqs, img = medium_genome
    h = hip_lib.open_index(img)
    try:
        reads = B.simulate_reads(seqs, 19998, length=150, seed=21, sub=0.02, indel=0.003) + [b"", b"ACGT" * 30]
        names = ["M%05d:%d:FC:%d" % (i, i % 8, i * 7) for i in range(len(reads))]
        t = fastq_text(reads, names, rand_quals(reads, 2), comments=[b" 1:N:0"] * len(reads))
        so = hip_lib.default_options()
        want = plain_path(hip_lib, h, so, t, None, False, None)
        assert len(want[1]) > 20000 * 200
        assert gz_path(hip_lib, h, so, bgzf_cut(t, 0xff00), None, False, None) == want
        pairs = B.simulate_pairs(seqs, 10000, length=150, seed=22, ins_mean=400, ins_sd=40)
        pn = ["F%05d" % (i >> 1) for i in range(20000)]
        pq = rand_quals(pairs, 4)
        t1, t2 = fastq_text(pairs[0::2], pn[0::2], pq[0::2], suffix=[b"/1"] * 10000), fastq_text(pairs[1::2], pn[1::2], pq[1::2], suffix=[b"/2"] * 10000, final=False)
        po = B.set_opt(hip_lib.default_options(), flag=B.MEM_F_PE)
        assert gz_path(hip_lib, h, po, bgzf_cut(t1, 0xff00), bgzf_cut(t2, 50000, 1), True, None) == plain_path(hip_lib, h, po, t1, t2, True, None)
    finally:
        hip_lib.destroy_index(h)
