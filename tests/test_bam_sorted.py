"""Coordinate-sorted BAM and its BAI index, sorted and indexed on the device (csrc/bam_sort.h, the k_sort_* / k_bamrec_* / k_bai_*
kernels in csrc/k_post.hip, the calls bwamem_hip_batch_sort_bam / _index_bam, bwamem_hip_bam_header_sorted,
bwamem_hip_align_to_sorted_bam, bwamem_hip_sort_pairs_device).  Nothing has a tolerance: the permutation is numpy's stable
argsort, the sorted stream is Python's stable sort of the parsed records, the index bytes are those of a builder written here from
the rules at the top of bam_sort.h, and -- independently of that builder -- the index is followed as the SAM specification 5.1.1 /
5.3 has it and must find exactly the records a scan finds.
CPU suite: the emulation build runs the kernels.  GPU suite (-m gpu): the same on the device, the medium and ALT genomes, long
reads, and the device's bytes against the emulation build's."""
import ctypes
import gzip
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

import bwalib as B
from test_bam_writer import CIG_OPS, EOF_BLOCK, _names_arg, _take, batch_bam, parse_header, parse_records, reg2bin, sam_writer_requests
from test_bgzf_device import BLOCK, batch_bgzf, bindz, members

LAST = 0xffffffffffffffff
_src = open(os.path.join(B.PKG, "csrc", "bam_sort.h")).read()
TILE = int(re.search(r"SORT_THREADS = (\d+)", _src).group(1)) * int(re.search(r"SORT_ITEMS = (\d+)", _src).group(1))


# ------------------------------------------------------------------------------------------ bindings
def binds(lib):
    d = bindz(lib)
    if getattr(d, "_sorted_bound", False):
        return d
    vp, sz, i64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int64
    d.bwamem_hip_batch_sort_bam.argtypes = [vp]
    d.bwamem_hip_batch_index_bam.restype = vp; d.bwamem_hip_batch_index_bam.argtypes = [vp, i64, ctypes.POINTER(sz)]
    d.bwamem_hip_bam_header_sorted.restype = vp; d.bwamem_hip_bam_header_sorted.argtypes = [vp, ctypes.POINTER(sz)]
    d.bwamem_hip_align_to_sorted_bam.argtypes = [vp, vp, vp, ctypes.c_char_p, sz, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    d.bwamem_hip_sort_pairs_device.argtypes = [vp, vp, sz, vp]
    d._sorted_bound = True
    return d


def sort_perm(lib, h, keys):
    d = binds(lib)
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    perm = np.full(max(keys.size, 1), 0xdeadbeef, dtype=np.uint32)
    assert d.bwamem_hip_sort_pairs_device(h, keys.ctypes.data, keys.size, perm.ctypes.data) == 0
    return perm[:keys.size]


# ------------------------------------------------------------------------------------------ test 1: the sort alone
def key_sets(n, rng):
    u64 = lambda a: np.asarray(a, dtype=np.uint64)
    r8 = lambda: rng.integers(0, 256, size=n, dtype=np.uint64)
    real = rng.integers(0, 40, size=n, dtype=np.uint64) << np.uint64(32) | rng.integers(0, 1 << 28, size=n, dtype=np.uint64)
    real[rng.random(n) < 0.03] = LAST
    return [("equal", np.full(n, 0x0123456789abcdef, dtype=np.uint64)), ("ascending", u64(np.arange(n))), ("descending", u64(np.arange(n)[::-1])),
            ("top_byte", r8() << np.uint64(56) | np.uint64(0x1234)), ("byte0", r8() | np.uint64(0xab00)), ("byte3", r8() << np.uint64(24) | np.uint64(0x55)),
            ("five", u64([7, 1 << 40, LAST, 0, 1 << 63])[rng.integers(0, 5, size=n)]), ("random", rng.integers(0, 1 << 64, size=n, dtype=np.uint64)),
            ("real", real)]


SORT_SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 3 * TILE + 17, 70001]


def check_sort(lib, h):
    rng = np.random.default_rng(17)
    for n in SORT_SIZES:
        for name, keys in key_sets(n, rng):
            got = sort_perm(lib, h, keys)
            assert np.array_equal(got, np.argsort(keys, kind="stable").astype(np.uint32)), (n, name)
            if n <= 3 * TILE + 17 or name == "real":
                assert np.array_equal(got, sort_perm(lib, h, keys)), ("two runs differ", n, name)


# ------------------------------------------------------------------------------------------ records, and the rules in Python
def split_records(buf):
    out, off = [], 0
    while off < len(buf):
        size = 4 + struct.unpack_from("<i", buf, off)[0]
        out.append(buf[off:off + size])
        off += size
    assert off == len(buf)
    return out


def rec_key(raw):
    refid, pos = struct.unpack_from("<ii", raw, 4)
    return (refid & 0xffffffff, pos)


def python_sorted(bam):
    return b"".join(sorted(split_records(bam), key=rec_key))


def rec_end(r):
    span = sum(c >> 4 for c in r["cig"] if CIG_OPS[c & 15] in "MDN=X")
    return r["pos"] + max(span, 1)


def with_offsets(bam):
    """parse_records of the stream, each with its start and end in it"""
    recs, off = parse_records(bam), 0
    for r in recs:
        r["off"], off = off, off + 4 + r["block_size"]
        r["stop"] = off
    return recs


def voffsets(member_sizes, coffset0):
    moff = [0]
    for s in member_sizes:
        moff.append(moff[-1] + s)
    return lambda p: (coffset0 + moff[p // BLOCK]) << 16 | p % BLOCK


def build_bai(recs, member_sizes, n_ref, coffset0):
    """the rules of bam_sort.h, plainly"""
    v = voffsets(member_sizes, coffset0)
    bins = [dict() for _ in range(n_ref)]
    lin = [dict() for _ in range(n_ref)]
    prev = None
    for r in recs:
        key = (r["refid"], r["bin"]) if r["refid"] >= 0 else None
        if key is not None:
            chunks = bins[key[0]].setdefault(key[1], [])
            if prev == key:
                chunks[-1][1] = v(r["stop"])
            else:
                chunks.append([v(r["off"]), v(r["stop"])])
            for w in range(r["pos"] >> 14, ((rec_end(r) - 1) >> 14) + 1):
                lin[key[0]].setdefault(w, v(r["off"]))
        prev = key
    o = b"BAI\1" + struct.pack("<i", n_ref)
    for ref in range(n_ref):
        o += struct.pack("<i", len(bins[ref]))
        for b in sorted(bins[ref]):
            o += struct.pack("<Ii", b, len(bins[ref][b])) + b"".join(struct.pack("<QQ", *c) for c in bins[ref][b])
        n_intv = max(lin[ref]) + 1 if lin[ref] else 0
        o += struct.pack("<i", n_intv)
        last = 0
        for w in range(n_intv):
            last = lin[ref].get(w, last)
            o += struct.pack("<Q", last)
    return o + struct.pack("<Q", sum(1 for r in recs if r["refid"] == -1))


def parse_bai(buf):
    assert buf[:4] == b"BAI\1"
    n_ref, = struct.unpack_from("<i", buf, 4)
    off, refs = 8, []
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<i", buf, off); off += 4
        bins = {}
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", buf, off); off += 8
            bins[b] = [struct.unpack_from("<QQ", buf, off + 16 * k) for k in range(n_chunk)]; off += 16 * n_chunk
        n_intv, = struct.unpack_from("<i", buf, off); off += 4
        refs.append((bins, struct.unpack_from("<%dQ" % n_intv, buf, off))); off += 8 * n_intv
    n_no_coor, = struct.unpack_from("<Q", buf, off)
    assert off + 8 == len(buf)
    return refs, n_no_coor


def reg2bins(beg, end):
    """SAM specification 5.3"""
    end -= 1
    out = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += range(first + (beg >> shift), first + (end >> shift) + 1)
    return out


def check_index_works(bai, z, coffset0, recs, ref_lens, seed):
    """test 4: 200 seeded intervals; what the index leads to is what a scan of the sorted records finds"""
    refs, n_no_coor = parse_bai(bai)
    assert n_no_coor == sum(1 for r in recs if r["refid"] == -1)
    ms = members(z, True)
    stream = b"".join(m[2] for m in ms)
    ustart, c = {}, coffset0                                           # compressed offset of a member -> its first byte in the stream
    for k, m in enumerate(ms):
        ustart[c] = k * BLOCK
        c += m[0]
    ustart[c] = len(stream)
    to_p = lambda vo: ustart[vo >> 16] + (vo & 0xffff)
    by_off = {r["off"]: r for r in recs}
    rng = np.random.default_rng(seed)
    queries = [(ref, 0, ln) for ref, ln in enumerate(ref_lens)]
    for ref, ln in enumerate(ref_lens):
        for edge in (1 << 14, 1 << 17, 3 << 14):
            if edge < ln:
                queries += [(ref, edge - 1, edge), (ref, edge, edge + 1), (ref, edge - 100, edge + 100), (ref, edge, min(ln, edge + (1 << 14)))]
    placed = [r for r in recs if r["refid"] >= 0]
    while len(queries) < 200:
        ref = int(rng.integers(0, len(ref_lens)))
        if placed and rng.random() < 0.5:                              # around a record
            r = placed[int(rng.integers(0, len(placed)))]
            ref, beg = r["refid"], max(0, r["pos"] + int(rng.integers(-200, 200)))
        else:
            beg = int(rng.integers(0, ref_lens[ref]))
        queries.append((ref, beg, min(ref_lens[ref], beg + int(rng.choice([1, 50, 1000, 40000])))))
    n_empty = 0
    for ref, beg, end in queries[:200] if len(queries) > 200 else queries:
        if end <= beg:
            continue
        bins, ioff = refs[ref]
        min_off = ioff[beg >> 14] if beg >> 14 < len(ioff) else 0
        found = set()
        for b in reg2bins(beg, end):
            for cb, ce in bins.get(b, ()):
                if ce <= min_off:
                    continue
                p, stop = to_p(cb), to_p(ce)
                while p < stop:
                    r = by_off[p]
                    assert r["refid"] == ref and r["bin"] == b, "a chunk holds a record of another bin"
                    if r["pos"] < end and rec_end(r) > beg:
                        found.add(p)
                    p = r["stop"]
                assert p == stop, "a chunk does not end at a record boundary"
        want = [r["off"] for r in recs if r["refid"] == ref and r["pos"] < end and rec_end(r) > beg]
        assert sorted(found) == want, (ref, beg, end)
        n_empty += not want
    return n_empty


# ------------------------------------------------------------------------------------------ one batch through the new calls
def sorted_batch(lib, h, opts, req, paired, names=None, pes=None, coffsets=(0, 12345)):
    """align -> encode -> download -> sort -> download -> sort again -> compress -> index at every coffset0"""
    d = binds(lib)
    b = d.bwamem_hip_batch_upload(h, req, len(req))
    assert b
    try:
        assert d.bwamem_hip_batch_keep_offsets(b, 1) == 0
        ob = ctypes.create_string_buffer(bytes(opts), B.OPT_SIZE)
        pb = ctypes.create_string_buffer(pes, len(pes)) if pes is not None else None
        assert d.bwamem_hip_batch_align(h, ob, pb, b, 0) == 0
        blob, off = _names_arg(names)
        assert d.bwamem_hip_batch_encode_bam(b, 1 if paired else 0, blob, off) == 0

        def download():
            m = d.bwamem_hip_batch_bam_bytes(b)
            buf = ctypes.create_string_buffer(max(m, 1))
            assert d.bwamem_hip_batch_bam_download(b, buf) == 0
            return buf.raw[:m]
        unsorted = download()
        assert d.bwamem_hip_batch_sort_bam(b) == 0
        srt = download()
        assert d.bwamem_hip_batch_sort_bam(b) == 0 and download() == srt, "sorting a second time must change nothing"
        assert d.bwamem_hip_batch_compress_bam(b, 1) == 0
        nz = d.bwamem_hip_batch_bgzf_bytes(b)
        z = ctypes.create_string_buffer(max(nz, 1))
        assert d.bwamem_hip_batch_bgzf_download(b, z) == 0
        bai = {}
        for c0 in coffsets:
            sz = ctypes.c_size_t()
            p = d.bwamem_hip_batch_index_bam(b, c0, ctypes.byref(sz))
            assert p, "bwamem_hip_batch_index_bam returned NULL"
            bai[c0] = _take(lib, p, sz.value)
        return unsorted, srt, z.raw[:nz], bai
    finally:
        d.bwamem_hip_batch_free(b)


def small_cases(lib, seqs):
    """the requests of sam_writer_requests plus what the issue wants every case to hold: duplicates (ties) and unplaced reads"""
    reads, pairs = sam_writer_requests(seqs)
    reads = reads + [reads[0], reads[5], reads[0], b"ACGTTGCAAC" * 9]
    pairs = pairs[:-1] + [pairs[0], pairs[1], b"AC" * 50, b"GT" * 50, pairs[4]]          # (odd: the trailing read has no record)
    po = B.set_opt(lib.default_options(), flag=B.MEM_F_PE)
    pes = B.pack_pestat(150, 450, 300.0, 30.0)
    out = []
    for rd, paired, pe, opts in ((reads, False, None, lib.default_options()), (pairs, True, pes, po)):
        for names in (None, ["q%d/%s" % (i, "x" * (i % 7)) for i in range(len(rd))]):
            out.append((rd, paired, pe, opts, names))
    return out


def check_sorted_records(unsorted, srt, want_features=True):
    """test 2 for one batch -> the sorted records, parsed, with their places"""
    assert len(unsorted) > 0 and srt == python_sorted(unsorted)
    recs = with_offsets(srt)
    keys = [(r["refid"] & 0xffffffff, r["pos"]) for r in recs]
    assert keys == sorted(keys)
    un = [r["name"] for r in parse_records(unsorted) if r["refid"] == -1]
    assert [r["name"] for r in recs[len(recs) - len(un):]] == un and all(r["refid"] >= 0 for r in recs[:len(recs) - len(un)]), "unplaced reads go last, in input order"
    if want_features:
        assert len(set(keys)) < len(keys), "no tie on (refID, pos)"
        assert un, "no unplaced read"
        assert any(r["flag"] & 0x10 for r in recs) and any(not r["flag"] & 0x10 and not r["flag"] & 4 for r in recs), "one strand only"
    return recs


def check_case(lib, h, seqs, rd, paired, pes, opts, names, want_features=True, seed=1):
    """tests 2, 3 and 4 for one request -> (sorted records, members, index at 0)"""
    unsorted, srt, z, bai = sorted_batch(lib, h, opts, B.pack_request(rd), paired, names, pes)
    recs = check_sorted_records(unsorted, srt, want_features)
    ms = members(z, True)
    assert b"".join(m[2] for m in ms) == srt
    for c0, got in bai.items():
        assert got == build_bai(recs, [m[0] for m in ms], len(seqs), c0), "index bytes, coffset0 = %d" % c0
        n_empty = check_index_works(got, z, c0, recs, [len(s) for _, s in seqs], seed + c0)
    assert n_empty > 0, "no query without a record"
    return srt, z, bai


def check_small_cases(lib, h, seqs):
    placed_unmapped = False
    for k, (rd, paired, pes, opts, names) in enumerate(small_cases(lib, seqs)):
        srt, _, _ = check_case(lib, h, seqs, rd, paired, pes, opts, names, seed=10 * k)
        placed_unmapped |= any(r["flag"] & 4 and r["refid"] >= 0 for r in parse_records(srt))
    assert placed_unmapped, "no placed unmapped mate"


def sorted_file(lib, h, opts, req, n_reads, path, bai_path, names=None, pes=None, write_header=True):
    d = binds(lib)
    ob = ctypes.create_string_buffer(bytes(opts), B.OPT_SIZE)
    pb = ctypes.create_string_buffer(pes, len(pes)) if pes is not None else None
    arr = (ctypes.c_char_p * n_reads)(*[n.encode() for n in names]) if names is not None else None
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    fb = os.open(bai_path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644) if bai_path else -1
    try:
        return d.bwamem_hip_align_to_sorted_bam(h, ob, pb, req, len(req), arr, fd, fb, 1 if write_header else 0)
    finally:
        os.close(fd)
        if fb >= 0:
            os.close(fb)


def headers(lib, h):
    d = binds(lib)
    sz = ctypes.c_size_t()
    plain = _take(lib, d.bwamem_hip_bam_header(h, ctypes.byref(sz)), sz.value)
    p = d.bwamem_hip_bam_header_sorted(h, ctypes.byref(sz))
    assert p
    return plain, _take(lib, p, sz.value)


def check_file(raw, bai, hdr_sorted, srt, n_ref):
    """a file of the sorted call: header + sorted records, the EOF block, and the index of exactly this file"""
    assert raw[-28:] == EOF_BLOCK and gzip.decompress(raw) == hdr_sorted + srt
    ms = members(raw, True)
    n_hdr = (len(hdr_sorted) + BLOCK - 1) // BLOCK
    assert b"".join(m[2] for m in ms[:n_hdr]) == hdr_sorted
    c0 = sum(m[0] for m in ms[:n_hdr])
    assert bai == build_bai(with_offsets(srt), [m[0] for m in ms[n_hdr:]], n_ref, c0)


def check_file_call(lib, h, seqs, tmpdir):
    """test 5, the native half"""
    plain, hdr = headers(lib, h)
    text, refs, used = parse_header(hdr)
    ptext, prefs, pused = parse_header(plain)
    assert used == len(hdr) and refs == prefs and hdr[used:] == plain[pused:]
    assert text.split("\n")[0] == "@HD\tVN:1.6\tSO:coordinate" and text.split("\n")[1:] == ptext.split("\n")[1:]
    path, bpath = os.path.join(tmpdir, "s.bam"), os.path.join(tmpdir, "s.bam.bai")
    for rd, paired, pes, opts, names in small_cases(lib, seqs):
        req = B.pack_request(rd)
        _, bam = batch_bam(lib, h, opts, req, paired, names, pes)
        srt = python_sorted(bam)
        assert sorted_file(lib, h, opts, req, len(rd), path, bpath, names, pes) == 0
        check_file(open(path, "rb").read(), open(bpath, "rb").read(), hdr, srt, len(seqs))
        assert sorted_file(lib, h, opts, req, len(rd), path, None, names, pes, write_header=False) == 0
        assert gzip.decompress(open(path, "rb").read()) == srt
    return hdr


def check_errors_and_state(lib, h, seqs, tmpdir):
    """test 6"""
    d = binds(lib)
    sz = ctypes.c_size_t()
    reads = B.simulate_reads(seqs, 6, length=100, seed=9)
    req = B.pack_request(reads)
    ob = ctypes.create_string_buffer(bytes(lib.default_options()), B.OPT_SIZE)
    b = d.bwamem_hip_batch_upload(h, req, len(req))
    try:
        assert d.bwamem_hip_batch_keep_offsets(b, 1) == 0
        assert d.bwamem_hip_batch_align(h, ob, None, b, 0) == 0
        assert d.bwamem_hip_batch_sort_bam(b) != 0, "sort before encode"
        assert not d.bwamem_hip_batch_index_bam(b, 0, ctypes.byref(sz)) and sz.value == 0
        assert d.bwamem_hip_batch_encode_bam(b, 0, None, None) == 0
        m = d.bwamem_hip_batch_bam_bytes(b)
        first = ctypes.create_string_buffer(m)
        assert d.bwamem_hip_batch_bam_download(b, first) == 0
        assert d.bwamem_hip_batch_compress_bam(b, 1) == 0
        assert not d.bwamem_hip_batch_index_bam(b, 0, ctypes.byref(sz)), "index before sort"
        assert d.bwamem_hip_batch_sort_bam(b) == 0
        assert d.bwamem_hip_batch_bgzf_bytes(b) == 0, "a sort must discard the members"
        assert not d.bwamem_hip_batch_index_bam(b, 0, ctypes.byref(sz)), "index before compress"
        buf = ctypes.create_string_buffer(m)
        assert d.bwamem_hip_batch_bam_bytes(b) == m and d.bwamem_hip_batch_bam_download(b, buf) == 0
        assert buf.raw == python_sorted(first.raw) and buf.raw != first.raw
        assert d.bwamem_hip_batch_encode_bam(b, 0, None, None) == 0
        assert d.bwamem_hip_batch_bam_download(b, buf) == 0 and buf.raw == first.raw, "an encode after a sort gives response order again"
        assert d.bwamem_hip_batch_compress_bam(b, 1) == 0
        assert not d.bwamem_hip_batch_index_bam(b, 0, ctypes.byref(sz)), "the encode must discard the sorted state"
        assert d.bwamem_hip_batch_sort_bam(b) == 0 and d.bwamem_hip_batch_compress_bam(b, 1) == 0
        p = d.bwamem_hip_batch_index_bam(b, 0, ctypes.byref(sz))
        assert p
        lib._free(p)
        assert d.bwamem_hip_batch_align(h, ob, None, b, 0) == 0
        assert d.bwamem_hip_batch_sort_bam(b) != 0, "a new alignment must discard the records"
    finally:
        d.bwamem_hip_batch_free(b)
    assert d.bwamem_hip_batch_sort_bam(None) != 0 and not d.bwamem_hip_batch_index_bam(None, 0, ctypes.byref(sz))
    path, bpath = os.path.join(tmpdir, "e.bam"), os.path.join(tmpdir, "e.bai")
    assert sorted_file(lib, h, lib.default_options(), req, len(reads), path, bpath, write_header=False) != 0
    assert os.path.getsize(path) == 0 and os.path.getsize(bpath) == 0, "a refused call must write nothing"
    # a batch of zero reads
    req0 = B.pack_request([])
    b = d.bwamem_hip_batch_upload(h, req0, len(req0))
    assert b
    try:
        assert d.bwamem_hip_batch_keep_offsets(b, 1) == 0 and d.bwamem_hip_batch_align(h, ob, None, b, 0) == 0
        assert d.bwamem_hip_batch_encode_bam(b, 0, None, None) == 0 and d.bwamem_hip_batch_sort_bam(b) == 0
        p = d.bwamem_hip_batch_index_bam(b, 0, ctypes.byref(sz))
        assert p
        assert _take(lib, p, sz.value) == b"BAI\1" + struct.pack("<i", len(seqs)) + struct.pack("<ii", 0, 0) * len(seqs) + struct.pack("<Q", 0)
    finally:
        d.bwamem_hip_batch_free(b)


# ------------------------------------------------------------------------------------------ CPU suite (emulation build)
def untouched_bytes(lib, h, seqs):
    reads, _ = sam_writer_requests(seqs)
    req = B.pack_request(reads)
    return batch_bam(lib, h, lib.default_options(), req, False), batch_bgzf(lib, h, lib.default_options(), req, False)


@pytest.fixture(scope="module")
def emu_index(small_genome):
    B.build_emu()
    emu = B.product_lib(emu=True)
    seqs, img = small_genome
    h = emu.open_index(img)
    before = untouched_bytes(emu, h, seqs)                             # (test 7: before any sorted batch exists in this module)
    yield emu, h, seqs, before
    emu.destroy_index(h)


def test_sort_pairs_against_stable_argsort(emu_index):
    emu, h, _, _ = emu_index
    check_sort(emu, h)


def test_sorted_records_and_index(emu_index):
    """tests 2, 3 and 4"""
    emu, h, seqs, _ = emu_index
    check_small_cases(emu, h, seqs)


def test_sorted_file_call(emu_index, tmp_path):
    emu, h, seqs, _ = emu_index
    check_file_call(emu, h, seqs, str(tmp_path))


def test_sorted_python_mirror(emu_index, small_genome, tmp_path):
    """BwaMemAligner.alignSeqsToBam(sort=True, index_path=...) over the emulation build"""
    emu, h, seqs, _ = emu_index
    _, img = small_genome
    reads = small_cases(emu, seqs)[0][0]
    r = subprocess.run([sys.executable, "-c", (
        "import sys; sys.path.insert(0, %r); import bwamem\n"
        "ix = bwamem.BwaMemIndex(%r); al = bwamem.BwaMemAligner(ix)\n"
        "reads = %r\n"
        "al.alignSeqsToBam(reads, %r, sort=True, index_path=%r)\n"
        "al.alignSeqsToBam(reads, %r, sort=True)\n"
        "try:\n    al.alignSeqsToBam(reads, %r, index_path=%r)\nexcept ValueError:\n    print('index-needs-sort')\n"
        "al.close(); ix.close()\n") % (B.PKG, img, reads, str(tmp_path / "a.bam"), str(tmp_path / "a.bam.bai"), str(tmp_path / "b.bam"),
                                       str(tmp_path / "c.bam"), str(tmp_path / "c.bai"))],
        env=dict(os.environ, LIBBWA_PATH=B.EMU_LIB), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "index-needs-sort" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
    assert not os.path.exists(str(tmp_path / "c.bam")) and not os.path.exists(str(tmp_path / "c.bai"))
    _, hdr = headers(emu, h)
    _, bam = batch_bam(emu, h, emu.default_options(), B.pack_request(reads), False)
    a = open(str(tmp_path / "a.bam"), "rb").read()
    check_file(a, open(str(tmp_path / "a.bam.bai"), "rb").read(), hdr, python_sorted(bam), len(seqs))
    assert open(str(tmp_path / "b.bam"), "rb").read() == a


def test_sorted_errors_and_state(emu_index, tmp_path):
    emu, h, seqs, _ = emu_index
    check_errors_and_state(emu, h, seqs, str(tmp_path))


def test_unsorted_path_untouched(emu_index):
    """test 7: the bytes of the calls that existed before are what they were before any batch was sorted (the buffer swap)"""
    emu, h, seqs, before = emu_index
    rd, paired, pes, opts, names = small_cases(emu, seqs)[0]
    sorted_batch(emu, h, opts, B.pack_request(rd), paired, names, pes)
    assert untouched_bytes(emu, h, seqs) == before


# ------------------------------------------------------------------------------------------ GPU suite
@pytest.mark.gpu
def test_gpu_sorted_small_cases(hip_lib, small_genome, tmp_path):
    """test 8: tests 1-6 on the device"""
    seqs, img = small_genome
    h = hip_lib.open_index(img)
    try:
        check_sort(hip_lib, h)
        check_small_cases(hip_lib, h, seqs)
        check_file_call(hip_lib, h, seqs, str(tmp_path))
        check_errors_and_state(hip_lib, h, seqs, str(tmp_path))
    finally:
        hip_lib.destroy_index(h)


@pytest.mark.gpu
def test_gpu_sorted_medium_single_and_paired(hip_lib, medium_genome):
    """test 9: the read sets of test_gpu_bam_medium_single_and_paired: several tiles, tens of thousands of records"""
    seqs, img = medium_genome
    h = hip_lib.open_index(img)
    try:
        g = seqs[0][1]
        reads = B.simulate_reads(seqs, 19990, length=150, seed=21, sub=0.02, indel=0.003)
        reads += [g[3000 + 500 * i:3080 + 500 * i] + B.revcomp(g[90000 + 700 * i:90070 + 700 * i]) for i in range(8)] + [b"", b"ACGT" * 30]
        pairs = B.simulate_pairs(seqs, 10000, length=150, seed=22, ins_mean=400, ins_sd=40)
        pairs[10] = b"ACGT" * 37
        po = B.set_opt(hip_lib.default_options(), flag=B.MEM_F_PE)
        for rd, paired, opts in ((reads, False, hip_lib.default_options()), (pairs, True, po)):
            srt, _, _ = check_case(hip_lib, h, seqs, rd, paired, None, opts, None, want_features=False, seed=90)
            assert len(split_records(srt)) > 2 * TILE
    finally:
        hip_lib.destroy_index(h)


@pytest.mark.gpu
def test_gpu_sorted_alt_genome(hip_lib, alt_genome):
    """test 10: many contigs, and references without records"""
    seqs, img, _, _, regions = alt_genome
    h = hip_lib.open_index(img)
    try:
        reads = B.reads_from_regions(seqs, regions, ["chr1_src", "family", "chr1_alt1", "chr1_alt2", "decoy"], 3000, length=150, seed=31, sub=0.01)
        reads += [b"ACGT" * 30, b"N" * 40, b""]
        _, _, bai = check_case(hip_lib, h, seqs, reads, False, None, hip_lib.default_options(), None, want_features=False, seed=91)
        refs, _ = parse_bai(bai[0])
        assert len(refs) == len(seqs) and any(not bins and not ioff for bins, ioff in refs) and sum(1 for bins, _ in refs if bins) > 1
        pairs = B.pairs_from_regions(seqs, regions, ["chr1_src", "chr2_src", "chr1_alt1", "chr2_alt1"], 1500, length=100, seed=32, ins_mean=300, ins_sd=30)
        pairs[5] = b"ACGT" * 25
        po = B.set_opt(hip_lib.default_options(), flag=B.MEM_F_PE)
        check_case(hip_lib, h, seqs, pairs, True, None, po, None, want_features=False, seed=92)
    finally:
        hip_lib.destroy_index(h)


@pytest.mark.gpu
def test_gpu_sorted_long_reads(hip_lib, medium_genome):
    """test 11: the 200 x 10 kb set of test_gpu_bam_long_reads: records of tens of KB cross the gather's chunks and the members"""
    seqs, img = medium_genome
    h = hip_lib.open_index(img)
    try:
        reads = B.simulate_reads(seqs, 196, length=10000, seed=41, sub=0.05, indel=0.01)
        g = seqs[0][1]
        reads += [g[10000:15000] + B.revcomp(g[200000:205000]), g[30000:34000] + g[300000:306000], b"ACGT" * 2500, B.revcomp(g[50000:60000])]
        srt, _, _ = check_case(hip_lib, h, seqs, reads, False, None, hip_lib.default_options(), None, want_features=False, seed=93)
        sizes = [len(r) for r in split_records(srt)]
        assert max(sizes) > 16384 and len(sizes) > len(reads)
    finally:
        hip_lib.destroy_index(h)


@pytest.mark.gpu
def test_gpu_sorted_equals_emulation(hip_lib, small_genome):
    """test 12: the device's sorted bytes, members and index are the emulation build's"""
    B.build_emu()
    emu = B.product_lib(emu=True)
    seqs, img = small_genome
    h, he = hip_lib.open_index(img), emu.open_index(img)
    try:
        for rd, paired, pes, opts, names in small_cases(hip_lib, seqs)[::3]:
            req = B.pack_request(rd)
            assert sorted_batch(hip_lib, h, opts, req, paired, names, pes) == sorted_batch(emu, he, opts, req, paired, names, pes)
    finally:
        hip_lib.destroy_index(h)
        emu.destroy_index(he)
