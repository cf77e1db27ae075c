"""BGZF compression on the device (csrc/bgzf_deflate.h, k_bgzf_deflate / k_bgzf_gather in csrc/k_post.hip, the calls
bwamem_hip_batch_compress_bam / _bgzf_bytes / _bgzf_download, bwamem_hip_bgzf_compress_device, bwamem_hip_align_to_bam_device).
Python's zlib and gzip are the oracle: a wrong Huffman table, bit order, CRC or ISIZE makes them raise.  Conditions on size are
derived from the format (a member is at most n + 31 bytes; a length-258 match costs under 3 bytes) or from what libz makes of the
same bytes with fixed codes, computed here.
CPU suite: the emulation build runs the kernels.  GPU suite (-m gpu): the same on the device, the medium genome, long reads, and
the device's bytes against the emulation build's."""
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
from test_bam_writer import (EOF_BLOCK, _names_arg, _take, _to_sam, batch_bam, bind, check_header, parse_header, parse_records,
                             sam_writer_requests, to_sam)

BLOCK = 0xff00


# ------------------------------------------------------------------------------------------ bindings
def bindz(lib):
    d = bind(lib)
    if getattr(d, "_bgzf_bound", False):
        return d
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    d.bwamem_hip_batch_compress_bam.argtypes = [vp, ctypes.c_int]
    d.bwamem_hip_batch_bgzf_bytes.restype = sz; d.bwamem_hip_batch_bgzf_bytes.argtypes = [vp]
    d.bwamem_hip_batch_bgzf_download.argtypes = [vp, vp]
    d.bwamem_hip_bgzf_compress_device.restype = vp
    d.bwamem_hip_bgzf_compress_device.argtypes = [vp, ctypes.c_char_p, sz, ctypes.c_int, ctypes.POINTER(sz)]
    d.bwamem_hip_align_to_bam_device.argtypes = [vp, vp, vp, ctypes.c_char_p, sz, vp, ctypes.c_int, ctypes.c_int]
    d._bgzf_bound = True
    return d


def zdev(lib, h, data, with_eof):
    d = bindz(lib)
    sz = ctypes.c_size_t()
    p = d.bwamem_hip_bgzf_compress_device(h, data, len(data), 1 if with_eof else 0, ctypes.byref(sz))
    assert p, "bwamem_hip_bgzf_compress_device returned NULL"
    return _take(lib, p, sz.value)


# ------------------------------------------------------------------------------------------ inputs
def big_input():
    """check_bgzf's `big` of tests/test_bam_writer.py: periodic, then random"""
    rng = np.random.default_rng(5)
    return (b"ACGTTGCA" * 40000) + rng.integers(0, 256, size=150000, dtype=np.uint8).tobytes()


def fibonacci_block():
    """byte frequencies 1, 1, 2, 3, 5, ... over 22 symbols (23 would not fit one block): the unlimited Huffman tree is 21 deep, the
    format allows 15"""
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    assert sum(fib) <= BLOCK
    data = np.concatenate([np.full(f, 40 + 3 * i, dtype=np.uint8) for i, f in enumerate(fib)])
    np.random.default_rng(8).shuffle(data)
    return data.tobytes()


def inputs():
    rng = np.random.default_rng(6)
    big = big_input()
    r30, r40 = (rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in (30000, 40000))
    return [("empty", b""), ("x", b"x"), ("big_ff00", big[:BLOCK]), ("big_ff01", big[:BLOCK + 1]), ("big", big),
            ("ff", b"\xff" * 200000), ("twice30k", r30 + r30), ("twice40k", r40 + r40), ("fibonacci", fibonacci_block()),
            ("all256", bytes(range(256)) * 3 + rng.integers(0, 256, size=2000, dtype=np.uint8).tobytes())]


# ------------------------------------------------------------------------------------------ the checks
def members(z, with_eof):
    """walk the members of a BGZF stream -> [(member size, ISIZE, the inflated bytes)], the EOF block left out"""
    out, off = [], 0
    end = len(z) - (len(EOF_BLOCK) if with_eof else 0)
    assert (z[-28:] == EOF_BLOCK) == bool(with_eof)
    while off < end:
        assert z[off:off + 4] == b"\x1f\x8b\x08\x04" and z[off + 4:off + 10] == b"\0\0\0\0\0\xff" and z[off + 10:off + 16] == b"\x06\x00BC\x02\x00"
        bsize, = struct.unpack_from("<H", z, off + 16)
        size = bsize + 1
        assert off + size <= end
        crc, isize = struct.unpack_from("<II", z, off + size - 8)
        o = zlib.decompressobj(-15)
        raw = o.decompress(z[off + 18:off + size - 8])
        assert o.eof and o.unused_data == b"" and o.unconsumed_tail == b""
        assert len(raw) == isize and zlib.crc32(raw) == crc and isize <= BLOCK
        out.append((size, isize, raw))
        off += size
    assert off == end
    return out


def check_round_trip(lib, h, data, name=""):
    """test 1 of the issue for one input -> the members (without EOF)"""
    ms = None
    for eof in (False, True):
        z = zdev(lib, h, data, eof)
        assert gzip.decompress(z) == data, name
        ms = members(z, eof)
        assert sum(m[1] for m in ms) == len(data) and b"".join(m[2] for m in ms) == data
        assert [m[1] for m in ms] == [min(BLOCK, len(data) - at) for at in range(0, len(data), BLOCK)], "not the host framer's cut"
        assert all(size <= isize + 31 for size, isize, _ in ms), name
        assert z == zdev(lib, h, data, eof), "two runs differ: " + name            # test 3: determinism
    return ms


def check_all_inputs(lib, h):
    sizes = {}
    for name, data in inputs():
        sizes[name] = [(size, isize) for size, isize, _ in check_round_trip(lib, h, data, name)]
    # test 2: conditions on size
    big = sizes["big"]
    n_periodic = 320000 // BLOCK                                               # full blocks of the ACGTTGCA run
    for size, isize in big[:n_periodic]:
        assert isize == BLOCK and size * 10 < isize, (size, isize)
    ref = zlib.compressobj(1, zlib.DEFLATED, -15, 8, getattr(zlib, "Z_FIXED", zlib.Z_DEFAULT_STRATEGY))
    assert len(ref.compress(b"ACGTTGCA" * (BLOCK // 8)) + ref.flush()) * 10 < BLOCK     # (what libz makes of such a block: about 1.1 %)
    assert all(size <= isize + 31 for size, isize in big)
    assert any(size == isize + 31 for size, isize in big[n_periodic + 1:]), "random bytes must fall back to stored blocks"
    assert sum(s for s, _ in sizes["ff"]) * 50 < 200000
    # 30 000 random bytes twice: without matches at distance 30 000 the block cannot shrink (60 031 bytes stored); with them the
    # second copy costs matches and the literals between them.  Three quarters of the input separates the two cases whatever the
    # share of positions a matcher still finds 30 000 bytes back.
    assert sizes["twice30k"][0][0] * 4 < 60000 * 3, "the second copy (distance 30 000) must be matched"
    assert sum(s for s, _ in sizes["twice40k"]) >= 80000, "40 000 random bytes twice cannot shrink: distance 40 000 is out of reach"
    fib_size, fib_n = sizes["fibonacci"][0]
    assert fib_size < fib_n * 5 // 8, "22 symbols: a flat 5-bit code gives 5/8 of the input, and a length-limited Huffman code beats a flat one"
    return sizes


def batch_bgzf(lib, h, opts, req, paired, names=None, pes=None, with_eof=True):
    """align -> encode -> compress -> download -> (records, BGZF bytes)"""
    d = bindz(lib)
    b = d.bwamem_hip_batch_upload(h, req, len(req))
    assert b
    try:
        assert d.bwamem_hip_batch_keep_offsets(b, 1) == 0
        ob = ctypes.create_string_buffer(bytes(opts), B.OPT_SIZE)
        pb = ctypes.create_string_buffer(pes, len(pes)) if pes is not None else None
        assert d.bwamem_hip_batch_align(h, ob, pb, b, 0) == 0
        blob, off = _names_arg(names)
        assert d.bwamem_hip_batch_encode_bam(b, 1 if paired else 0, blob, off) == 0
        m = d.bwamem_hip_batch_bam_bytes(b)
        bam = ctypes.create_string_buffer(max(m, 1))
        assert d.bwamem_hip_batch_bam_download(b, bam) == 0
        assert d.bwamem_hip_batch_compress_bam(b, 1 if with_eof else 0) == 0
        nz = d.bwamem_hip_batch_bgzf_bytes(b)
        z = ctypes.create_string_buffer(max(nz, 1))
        assert d.bwamem_hip_batch_bgzf_download(b, z) == 0
        return bam.raw[:m], z.raw[:nz]
    finally:
        d.bwamem_hip_batch_free(b)


def small_batches(lib, seqs):
    reads, pairs = sam_writer_requests(seqs)
    return [(reads, False, None, lib.default_options()),
            (pairs, True, B.pack_pestat(150, 450, 300.0, 30.0), B.set_opt(lib.default_options(), flag=B.MEM_F_PE))]


def check_batch_path(lib, h, seqs):
    """test 4"""
    for rd, paired, pes, opts in small_batches(lib, seqs):
        for eof in (False, True):
            bam, z = batch_bgzf(lib, h, opts, B.pack_request(rd), paired, pes=pes, with_eof=eof)
            assert len(bam) > 0 and gzip.decompress(z) == bam
            members(z, eof)


def align_to_bam_device_file(lib, h, opts, req, n_reads, path, names=None, pes=None, write_header=True):
    d = bindz(lib)
    ob = ctypes.create_string_buffer(bytes(opts), B.OPT_SIZE)
    pb = ctypes.create_string_buffer(pes, len(pes)) if pes is not None else None
    arr = (ctypes.c_char_p * n_reads)(*[n.encode() for n in names]) if names is not None else None
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        return d.bwamem_hip_align_to_bam_device(h, ob, pb, req, len(req), arr, fd, 1 if write_header else 0)
    finally:
        os.close(fd)


def check_align_to_bam_device(lib, h, seqs, tmpdir):
    """test 5"""
    hdr = check_header(lib, h, seqs)
    for rd, paired, pes, opts in small_batches(lib, seqs):
        req = B.pack_request(rd)
        for names in (None, ["q%d" % i for i in range(len(rd))]):
            _, bam = batch_bam(lib, h, opts, req, paired, names, pes)
            path = os.path.join(tmpdir, "dev_%d.bam" % paired)
            assert align_to_bam_device_file(lib, h, opts, req, len(rd), path, names, pes, True) == 0
            raw = open(path, "rb").read()
            assert raw[-28:] == EOF_BLOCK
            assert gzip.decompress(raw) == hdr + bam
            members(raw, True)
            assert align_to_bam_device_file(lib, h, opts, req, len(rd), path, names, pes, False) == 0
            raw = open(path, "rb").read()
            assert raw[-28:] == EOF_BLOCK and gzip.decompress(raw) == bam


def check_errors_device(lib, h, seqs):
    """test 6"""
    d = bindz(lib)
    reads = B.simulate_reads(seqs, 3, length=100, seed=9)
    req = B.pack_request(reads)
    ob = ctypes.create_string_buffer(bytes(lib.default_options()), B.OPT_SIZE)
    b = d.bwamem_hip_batch_upload(h, req, len(req))
    try:
        assert d.bwamem_hip_batch_keep_offsets(b, 1) == 0
        assert d.bwamem_hip_batch_align(h, ob, None, b, 0) == 0
        assert d.bwamem_hip_batch_compress_bam(b, 1) != 0, "compress before encode"
        assert d.bwamem_hip_batch_bgzf_bytes(b) == 0
        blob, off = _names_arg(["a", "b" * 255, "c"])
        assert d.bwamem_hip_batch_encode_bam(b, 0, blob, off) != 0
        assert d.bwamem_hip_batch_compress_bam(b, 1) != 0, "compress after a failed encode"
        assert d.bwamem_hip_batch_bgzf_bytes(b) == 0
        assert d.bwamem_hip_batch_encode_bam(b, 0, None, None) == 0
        assert d.bwamem_hip_batch_compress_bam(b, 1) == 0 and d.bwamem_hip_batch_bgzf_bytes(b) > 28
        assert d.bwamem_hip_batch_encode_bam(b, 0, None, None) == 0
        assert d.bwamem_hip_batch_bgzf_bytes(b) == 0, "a second encode must discard the members"
        assert d.bwamem_hip_batch_compress_bam(b, 0) == 0 and d.bwamem_hip_batch_bgzf_bytes(b) > 0
        assert d.bwamem_hip_batch_align(h, ob, None, b, 0) == 0
        assert d.bwamem_hip_batch_bgzf_bytes(b) == 0, "a new alignment must discard the members"
    finally:
        d.bwamem_hip_batch_free(b)
    assert d.bwamem_hip_batch_compress_bam(None, 1) != 0
    assert d.bwamem_hip_batch_bgzf_bytes(None) == 0


# ------------------------------------------------------------------------------------------ CPU suite (emulation build)
@pytest.fixture(scope="module")
def emu_index(small_genome):
    B.build_emu()
    emu = B.product_lib(emu=True)
    seqs, img = small_genome
    h = emu.open_index(img)
    yield emu, h, seqs
    emu.destroy_index(h)


def test_bgzf_device_round_trip_sizes_determinism(emu_index):
    emu, h, _ = emu_index
    check_all_inputs(emu, h)


def test_bgzf_device_batch_path(emu_index):
    emu, h, seqs = emu_index
    check_batch_path(emu, h, seqs)


def test_bgzf_device_align_to_bam(emu_index, tmp_path):
    emu, h, seqs = emu_index
    check_align_to_bam_device(emu, h, seqs, str(tmp_path))


def test_bgzf_device_errors(emu_index):
    emu, h, seqs = emu_index
    check_errors_device(emu, h, seqs)


def test_bgzf_device_python_mirror(small_genome, tmp_path):
    """BwaMemAligner.alignSeqsToBam(device=True) over the emulation build (the mirror binds whatever LIBBWA_PATH names)"""
    B.build_emu()
    seqs, img = small_genome
    reads, _ = sam_writer_requests(seqs)
    r = subprocess.run([sys.executable, "-c", (
        "import sys; sys.path.insert(0, %r); import bwamem\n"
        "ix = bwamem.BwaMemIndex(%r); al = bwamem.BwaMemAligner(ix)\n"
        "reads = %r\n"
        "al.alignSeqsToBam(reads, %r, device=True)\n"
        "al.alignSeqsToBam(reads, %r, names=['n%%d' %% i for i in range(len(reads))], level=9, device=True)\n"
        "al.close(); ix.close(); print('mirror-ok')\n") % (B.PKG, img, reads, str(tmp_path / "a.bam"), str(tmp_path / "b.bam"))],
        env=dict(os.environ, LIBBWA_PATH=B.EMU_LIB), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "mirror-ok" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
    emu = B.product_lib(emu=True)
    h = emu.open_index(img)
    try:
        contigs = emu.contig_names(h)
        req = B.pack_request(reads)
        for fn, names in (("a.bam", None), ("b.bam", ["n%d" % i for i in range(len(reads))])):
            z = open(str(tmp_path / fn), "rb").read()
            ms = members(z, True)
            assert any(m[0] < m[1] for m in ms), "nothing was compressed"
            raw = gzip.decompress(z)
            _, refs, used = parse_header(raw)
            assert [n for n, _ in refs] == contigs
            resp = emu.align_raw(h, emu.default_options(), req)
            assert to_sam(parse_records(raw[used:]), contigs) == _to_sam(emu, h, req, resp, False, names)
    finally:
        emu.destroy_index(h)


def test_bgzf_device_sanitizers(small_genome):
    """the calls of the tests above under AddressSanitizer + UBSan (tests/emu `make asan`), in a child process that preloads the runtimes"""
    B.make(os.path.join(B.ROOT, "tests", "emu"), "asan")
    libs = [subprocess.run(["gcc", "-print-file-name=" + n], capture_output=True, text=True).stdout.strip() for n in ("libasan.so", "libubsan.so")]
    if not all(os.path.isabs(x) and os.path.exists(x) for x in libs):
        pytest.skip("no sanitizer runtimes next to this gcc")
    seqs, img = small_genome
    env = dict(os.environ, LD_PRELOAD=":".join(libs), ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0")
    r = subprocess.run([sys.executable, os.path.join(B.ROOT, "tests", "bgzf_sanitized_child.py"), img, img[:-4]],
                       env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "sanitized-ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])


# ------------------------------------------------------------------------------------------ GPU suite
def fixed_code_bytes(data):
    """what libz level 1 with fixed codes makes of the same bytes, framed the same way: per 0xff00 block, plus 26 bytes per member"""
    total = 0
    for at in range(0, len(data), BLOCK):
        o = zlib.compressobj(1, zlib.DEFLATED, -15, 8, zlib.Z_FIXED)
        total += len(o.compress(data[at:at + BLOCK]) + o.flush()) + 26
    return total


@pytest.mark.gpu
def test_gpu_bgzf_device_small_cases(hip_lib, small_genome, tmp_path):
    """test 9: the CPU cases on the device"""
    seqs, img = small_genome
    h = hip_lib.open_index(img)
    try:
        check_all_inputs(hip_lib, h)
        check_batch_path(hip_lib, h, seqs)
        check_align_to_bam_device(hip_lib, h, seqs, str(tmp_path))
        check_errors_device(hip_lib, h, seqs)
    finally:
        hip_lib.destroy_index(h)


@pytest.mark.gpu
def test_gpu_bgzf_device_medium_single_and_paired(hip_lib, medium_genome):
    """test 10: the read sets of test_gpu_bam_medium_single_and_paired; the stream round-trips and is smaller than an LZ77 matcher
    without dynamic tables (libz level 1, fixed codes) makes the same records"""
    seqs, img = medium_genome
    h = hip_lib.open_index(img)
    try:
        g = seqs[0][1]
        reads = B.simulate_reads(seqs, 19990, length=150, seed=21, sub=0.02, indel=0.003)
        reads += [g[3000 + 500 * i:3080 + 500 * i] + B.revcomp(g[90000 + 700 * i:90070 + 700 * i]) for i in range(8)] + [b"", b"ACGT" * 30]
        assert len(reads) == 20000
        pairs = B.simulate_pairs(seqs, 10000, length=150, seed=22, ins_mean=400, ins_sd=40)
        pairs[10] = b"ACGT" * 37
        po = B.set_opt(hip_lib.default_options(), flag=B.MEM_F_PE)
        for rd, paired, opts in ((reads, False, hip_lib.default_options()), (pairs, True, po)):
            bam, z = batch_bgzf(hip_lib, h, opts, B.pack_request(rd), paired)
            assert len(bam) > 20000 * 200 and gzip.decompress(z) == bam
            ms = members(z, True)
            assert len(ms) == (len(bam) + BLOCK - 1) // BLOCK
            print("bgzf device: %d records bytes -> %d (%.4f)" % (len(bam), len(z), len(z) / len(bam)))
            if hasattr(zlib, "Z_FIXED"):
                ref = fixed_code_bytes(bam)
                print("libz level 1, fixed codes: %d (%.4f)" % (ref, ref / len(bam)))
                assert len(z) - 28 < ref
    finally:
        hip_lib.destroy_index(h)


@pytest.mark.gpu
def test_gpu_bgzf_device_long_reads(hip_lib, medium_genome):
    """test 11: 200 reads of 10 kb (the set of test_gpu_bam_long_reads): records of tens of KB cross the block boundaries"""
    seqs, img = medium_genome
    h = hip_lib.open_index(img)
    try:
        reads = B.simulate_reads(seqs, 196, length=10000, seed=41, sub=0.05, indel=0.01)
        g = seqs[0][1]
        reads += [g[10000:15000] + B.revcomp(g[200000:205000]), g[30000:34000] + g[300000:306000], b"ACGT" * 2500, B.revcomp(g[50000:60000])]
        bam, z = batch_bgzf(hip_lib, h, hip_lib.default_options(), B.pack_request(reads), False)
        assert len(bam) > 200 * 10000 and gzip.decompress(z) == bam
        assert len(members(z, True)) > 30
    finally:
        hip_lib.destroy_index(h)


@pytest.mark.gpu
def test_gpu_bgzf_device_equals_emulation(hip_lib, small_genome):
    """test 12: the device's bytes are the emulation build's"""
    B.build_emu()
    emu = B.product_lib(emu=True)
    seqs, img = small_genome
    h, he = hip_lib.open_index(img), emu.open_index(img)
    try:
        big = big_input()
        assert zdev(hip_lib, h, big, True) == zdev(emu, he, big, True)
        reads, _ = sam_writer_requests(seqs)
        req = B.pack_request(reads)
        bam_d, z_d = batch_bgzf(hip_lib, h, hip_lib.default_options(), req, False)
        bam_e, z_e = batch_bgzf(emu, he, emu.default_options(), req, False)
        assert bam_d == bam_e and z_d == z_e
    finally:
        hip_lib.destroy_index(h)
        emu.destroy_index(he)
