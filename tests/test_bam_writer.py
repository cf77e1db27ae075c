"""BAM on the native side (csrc/bam_encode.h, the size / emit kernels in csrc/k_post.hip, BGZF and the header in csrc/sam_writer.cpp).
The one rule: a BAM record decodes to exactly the SAM line bwamem_hip_response_to_sam writes for the same response record.  This
file carries its own BAM reader, written from SAM specification 4.2 (gzip for BGZF, struct for the header and the records), turns
every record back into a SAM line and compares the text with the native SAM writer's and with the independent Python formatter of
tests/test_sam_writer.py (_expected).  Nothing is left out of a comparison and nothing has a tolerance.
CPU suite: the emulation build runs the kernels.  GPU suite (-m gpu): the same on the device, plus large, ALT and long-read sets."""
import ctypes
import gzip
import os
import struct
import subprocess
import sys

import pytest

import bwalib as B
from test_sam_writer import _expected, _to_sam

EOF_BLOCK = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
SEQ_CODES = "=ACMGRSVTWYHKDBN"
CIG_OPS = "MIDNSHP=X"
INT_FMT = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I"}


# ------------------------------------------------------------------------------------------ bindings
def bind(lib):
    d = lib.dll
    if getattr(d, "_bam_bound", False):
        return d
    vp, sz, i64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int64
    d.bwamem_hip_batch_upload.restype = vp; d.bwamem_hip_batch_upload.argtypes = [vp, ctypes.c_char_p, sz]
    d.bwamem_hip_batch_align.argtypes = [vp, vp, vp, vp, i64]
    d.bwamem_hip_batch_result_bytes.restype = sz; d.bwamem_hip_batch_result_bytes.argtypes = [vp]
    d.bwamem_hip_batch_download.argtypes = [vp, vp]
    d.bwamem_hip_batch_free.argtypes = [vp]; d.bwamem_hip_batch_free.restype = None
    d.bwamem_hip_batch_keep_offsets.argtypes = [vp, ctypes.c_int]
    d.bwamem_hip_batch_encode_bam.argtypes = [vp, ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(i64)]
    d.bwamem_hip_batch_bam_bytes.restype = sz; d.bwamem_hip_batch_bam_bytes.argtypes = [vp]
    d.bwamem_hip_batch_bam_download.argtypes = [vp, vp]
    d.bwamem_hip_bam_header.restype = vp; d.bwamem_hip_bam_header.argtypes = [vp, ctypes.POINTER(sz)]
    d.bwamem_hip_sam_header.restype = vp; d.bwamem_hip_sam_header.argtypes = [vp, ctypes.POINTER(sz)]
    d.bwamem_hip_bgzf_compress.restype = vp
    d.bwamem_hip_bgzf_compress.argtypes = [ctypes.c_char_p, sz, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(sz)]
    d.bwamem_hip_align_to_bam.argtypes = [vp, vp, vp, ctypes.c_char_p, sz, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    d.bwamem_hip_bam_record_bytes.restype = i64
    d.bwamem_hip_bam_record_bytes.argtypes = [ctypes.c_char_p, sz, ctypes.c_int, ctypes.c_int32, ctypes.c_int32]
    d._bam_bound = True
    return d


def _take(lib, p, n):
    out = ctypes.string_at(p, n)
    lib._free(p)
    return out


def _names_arg(names):
    if names is None:
        return None, None
    enc = [n if isinstance(n, bytes) else n.encode() for n in names]
    off = [0]
    for n in enc:
        off.append(off[-1] + len(n))
    return b"".join(enc), (ctypes.c_int64 * len(off))(*off)


def batch_bam(lib, h, opts, req, paired, names=None, pes=None, read_id0=0):
    """one resident batch: align, download the response, encode BAM records on the device, download them -> (response, records)"""
    d = bind(lib)
    b = d.bwamem_hip_batch_upload(h, req, len(req))
    assert b
    try:
        assert d.bwamem_hip_batch_keep_offsets(b, 1) == 0
        ob = ctypes.create_string_buffer(bytes(opts), B.OPT_SIZE)
        pb = ctypes.create_string_buffer(pes, len(pes)) if pes is not None else None
        assert d.bwamem_hip_batch_align(h, ob, pb, b, read_id0) == 0
        n = d.bwamem_hip_batch_result_bytes(b)
        resp = ctypes.create_string_buffer(max(n, 1))
        assert d.bwamem_hip_batch_download(b, resp) == 0
        blob, off = _names_arg(names)
        assert d.bwamem_hip_batch_encode_bam(b, 1 if paired else 0, blob, off) == 0
        m = d.bwamem_hip_batch_bam_bytes(b)
        bam = ctypes.create_string_buffer(max(m, 1))
        assert d.bwamem_hip_batch_bam_download(b, bam) == 0
        return resp.raw[:n], bam.raw[:m]
    finally:
        d.bwamem_hip_batch_free(b)


def bgzf(lib, data, level, n_threads, with_eof):
    d = bind(lib)
    sz = ctypes.c_size_t()
    p = d.bwamem_hip_bgzf_compress(data, len(data), level, n_threads, 1 if with_eof else 0, ctypes.byref(sz))
    return _take(lib, p, sz.value) if p else None


def have_zlib():
    try:
        ctypes.CDLL("libz.so.1")
        return True
    except OSError:
        return False


# ------------------------------------------------------------------------------------------ the reader (SAM spec 4.2)
def parse_header(buf):
    assert buf[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<i", buf, 4)
    text = buf[8:8 + l_text]
    off = 8 + l_text
    n_ref, = struct.unpack_from("<i", buf, off); off += 4
    refs = []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", buf, off); off += 4
        name = buf[off:off + l_name]; off += l_name
        assert name.endswith(b"\0") and name.count(b"\0") == 1
        l_ref, = struct.unpack_from("<i", buf, off); off += 4
        refs.append((name[:-1].decode(), l_ref))
    return text.decode(), refs, off


def parse_records(buf):
    recs, off = [], 0
    while off < len(buf):
        block_size, = struct.unpack_from("<i", buf, off)
        end = off + 4 + block_size
        assert block_size >= 32 and end <= len(buf)
        refid, pos, l_rn, mapq, bin_, n_cig, flag, l_seq, nrid, npos, tlen = struct.unpack_from("<iiBBHHHiiii", buf, off + 4)
        p = off + 36
        name = buf[p:p + l_rn]; p += l_rn
        cig = struct.unpack_from("<%dI" % n_cig, buf, p); p += 4 * n_cig
        seq = buf[p:p + (l_seq + 1) // 2]; p += (l_seq + 1) // 2
        qual = buf[p:p + l_seq]; p += l_seq
        tags = []
        while p < end:
            tag, ty = buf[p:p + 2].decode(), chr(buf[p + 2]); p += 3
            if ty == "Z":
                z = buf.index(b"\0", p)
                val = buf[p:z].decode(); p = z + 1
            else:
                val, = struct.unpack_from("<" + INT_FMT[ty], buf, p); p += struct.calcsize(INT_FMT[ty])
            tags.append((tag, ty, val))
        assert p == end, "tags overrun the record"
        recs.append(dict(block_size=block_size, refid=refid, pos=pos, l_rn=l_rn, mapq=mapq, bin=bin_, flag=flag, l_seq=l_seq, nrid=nrid,
                         npos=npos, tlen=tlen, name=name, cig=cig, seq=seq, qual=qual, tags=tags))
        off = end
    assert off == len(buf), "block_size values do not sum to the stream length"
    return recs


def sam_line(r, contigs):
    assert r["name"].endswith(b"\0") and r["name"].count(b"\0") == 1 and r["l_rn"] == len(r["name"])
    bases = "".join(SEQ_CODES[b >> 4] + SEQ_CODES[b & 15] for b in r["seq"])[:r["l_seq"]]
    if r["l_seq"] & 1:
        assert r["seq"][-1] & 15 == 0
    f = [r["name"][:-1].decode(), str(r["flag"]), contigs[r["refid"]] if r["refid"] >= 0 else "*", str(r["pos"] + 1), str(r["mapq"]),
         "".join("%d%s" % (c >> 4, CIG_OPS[c & 15]) for c in r["cig"]) or "*",
         "*" if r["nrid"] < 0 else "=" if r["nrid"] == r["refid"] else contigs[r["nrid"]], str(r["npos"] + 1), str(r["tlen"]),
         bases or "*", "*" if all(q == 0xff for q in r["qual"]) else "".join(chr(q + 33) for q in r["qual"])]
    f += ["%s:%s:%s" % (t, "Z" if ty == "Z" else "i", v) for t, ty, v in r["tags"]]
    return "\t".join(f)


def to_sam(recs, contigs):
    return "".join(sam_line(r, contigs) + "\n" for r in recs)


def reg2bin(beg, end):
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def check_fields(recs):
    """what the text cannot show: bin, the NUL of the name, the smallest integer types, QUAL"""
    for r in recs:
        if r["refid"] < 0:
            want = 4680
        elif r["flag"] & 4:
            want = reg2bin(r["pos"], r["pos"] + 1)
        else:
            span = sum(c >> 4 for c in r["cig"] if CIG_OPS[c & 15] in "MDN=X")
            want = reg2bin(r["pos"], r["pos"] + max(span, 1))
        assert r["bin"] == want, (r["bin"], want)
        assert r["l_rn"] == len(r["name"]) and r["name"][-1] == 0 and 2 <= r["l_rn"] <= 255
        assert all(q == 0xff for q in r["qual"]) and len(r["qual"]) == r["l_seq"]
        if r["flag"] & 4:
            assert not r["cig"] and not r["tags"]
        for t, ty, v in r["tags"]:
            if ty == "Z":
                assert v and "\0" not in v
                continue
            small = ("C" if v <= 0xff else "S" if v <= 0xffff else "I") if v >= 0 else ("c" if v >= -128 else "s" if v >= -32768 else "i")
            assert ty == small, (t, ty, v)
        assert [t for t, _, _ in r["tags"]] == [t for t in ("NM", "MD", "AS", "XS", "XA") if t in {x for x, _, _ in r["tags"]}]


def check_batch(lib, h, contigs, reads, opts, paired, names=None, pes=None, read_id0=0, default_names=None, expected=True):
    """align + encode one batch; its BAM records as SAM text must equal the native SAM writer's text (and the Python formatter's)
    -> the parsed records"""
    req = B.pack_request(reads)
    resp, bam = batch_bam(lib, h, opts, req, paired, names, pes, read_id0)
    recs = parse_records(bam)
    sam_names = names if names is not None else default_names
    want = _to_sam(lib, h, req, resp, paired, sam_names)
    assert to_sam(recs, contigs) == want
    if expected:
        n_dec = len(reads) - (1 if paired and len(reads) & 1 else 0)
        dec = B.decode_response(resp, n_dec) + [[]] * (len(reads) - n_dec)
        assert want == _expected(reads, dec, contigs, paired, sam_names)
    assert len(recs) == want.count("\n")
    check_fields(recs)
    return recs


def sam_writer_requests(seqs):
    """the request set of tests/test_sam_writer.py::test_sam_writer_single_and_paired"""
    reads = B.simulate_reads(seqs, 14, length=100, seed=3, sub=0.02, indel=0.004)
    g = seqs[0][1]
    reads += [g[3000:3060] + B.revcomp(g[9000:9070]), g[12000:12050] + g[20000:20080], b"ACGT" * 15, b""]
    pairs = B.simulate_pairs(seqs, 6, length=100, seed=5, ins_mean=300, ins_sd=30)
    pairs[3] = b"ACGT" * 25
    pairs.append(pairs[0])
    return reads, pairs


def run_small_cases(lib, h, seqs):
    """cases 1 and 3 of the issue: single-end and paired-end, default and caller's names"""
    contigs = lib.contig_names(h)
    reads, pairs = sam_writer_requests(seqs)
    opts = lib.default_options()
    recs = check_batch(lib, h, contigs, reads, opts, False)
    assert len({r["name"] for r in recs}) < len(recs), "no read with several records: the clipping rule would go untested"
    assert any(any(CIG_OPS[c & 15] == "H" for c in r["cig"]) for r in recs)
    assert any(r["flag"] & 0x10 for r in recs) and any(r["flag"] & 4 for r in recs) and any(r["l_seq"] == 0 for r in recs)
    names = ["read_%d/x" % i for i in range(len(reads))]
    names[1] = "n"
    names[2] = "N" * 254
    check_batch(lib, h, contigs, reads, opts, False, names)
    po = B.set_opt(lib.default_options(), flag=B.MEM_F_PE)
    pes = B.pack_pestat(150, 450, 300.0, 30.0)
    precs = check_batch(lib, h, contigs, pairs, po, True, pes=pes)
    assert {r["name"] for r in precs} == {b"p%d\0" % i for i in range(6)}, "the odd trailing read must have no record"
    assert any(r["flag"] & 4 and r["refid"] >= 0 for r in precs), "no unmapped read placed at its mate: that rule would go untested"
    check_batch(lib, h, contigs, pairs, po, True, ["pair%d" % (i >> 1) for i in range(len(pairs))], pes=pes)
    check_batch(lib, h, contigs, pairs, po, True)                     # inferred insert-size statistics: the two-phase path
    return reads, pairs


def check_header(lib, h, seqs):
    d = bind(lib)
    sz = ctypes.c_size_t()
    hdr = _take(lib, d.bwamem_hip_bam_header(h, ctypes.byref(sz)), sz.value)
    text, refs, used = parse_header(hdr)
    assert used == len(hdr)
    assert [n for n, _ in refs] == lib.contig_names(h) and refs == [(n, len(s)) for n, s in seqs]
    assert text == _take(lib, d.bwamem_hip_sam_header(h, ctypes.byref(sz)), sz.value).decode()
    return hdr


def check_bgzf(lib):
    import numpy as np
    rng = np.random.default_rng(5)
    big = (b"ACGTTGCA" * 40000) + rng.integers(0, 256, size=150000, dtype=np.uint8).tobytes()       # compressible, then not
    levels = [0] + ([1] if have_zlib() else [])
    for level in levels:
        for data in (b"", b"x", big[:0xff00], big[:0xff01], big):
            for eof in (False, True):
                z1 = bgzf(lib, data, level, 1, eof)
                assert z1 is not None
                assert z1 == bgzf(lib, data, level, 4, eof), "the result depends on the number of threads"
                assert gzip.decompress(z1) == data
                off, n_in = 0, 0
                while off < len(z1):                                         # every member: gzip with the BC field, BSIZE = its size - 1
                    assert z1[off:off + 4] == b"\x1f\x8b\x08\x04" and z1[off + 10:off + 16] == b"\x06\x00BC\x02\x00"
                    bsize, = struct.unpack_from("<H", z1, off + 16)
                    isize, = struct.unpack_from("<I", z1, off + bsize + 1 - 4)
                    assert isize <= 0xff00
                    n_in += isize
                    off += bsize + 1
                assert off == len(z1) and n_in == len(data)
                assert (z1[-28:] == EOF_BLOCK) == eof
    if not have_zlib():
        assert bgzf(lib, b"abc", 1, 1, True) is None
    assert bgzf(lib, b"abc", 10, 1, True) is None


def align_to_bam_file(lib, h, opts, req, n_reads, path, names=None, pes=None, level=0, write_header=True):
    d = bind(lib)
    ob = ctypes.create_string_buffer(bytes(opts), B.OPT_SIZE)
    pb = ctypes.create_string_buffer(pes, len(pes)) if pes is not None else None
    arr = (ctypes.c_char_p * n_reads)(*[n.encode() for n in names]) if names is not None else None
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        return d.bwamem_hip_align_to_bam(h, ob, pb, req, len(req), arr, level, fd, 1 if write_header else 0)
    finally:
        os.close(fd)


def check_align_to_bam(lib, h, seqs, tmpdir):
    reads, pairs = sam_writer_requests(seqs)
    hdr = check_header(lib, h, seqs)
    levels = [0] + ([1] if have_zlib() else [])
    for rd, paired, pes in ((reads, False, None), (pairs, True, B.pack_pestat(150, 450, 300.0, 30.0))):
        opts = B.set_opt(lib.default_options(), flag=B.MEM_F_PE if paired else 0)
        req = B.pack_request(rd)
        for names in (None, ["q%d" % i for i in range(len(rd))]):
            _, bam = batch_bam(lib, h, opts, req, paired, names, pes)
            for level in levels:
                path = os.path.join(tmpdir, "out_%d_%d.bam" % (paired, level))
                assert align_to_bam_file(lib, h, opts, req, len(rd), path, names, pes, level, True) == 0
                raw = open(path, "rb").read()
                assert raw[-28:] == EOF_BLOCK
                assert gzip.decompress(raw) == hdr + bam
                assert align_to_bam_file(lib, h, opts, req, len(rd), path, names, pes, level, False) == 0
                assert gzip.decompress(open(path, "rb").read()) == bam


def check_errors(lib, h, seqs):
    d = bind(lib)
    reads = B.simulate_reads(seqs, 3, length=100, seed=9)
    req = B.pack_request(reads)
    ob = ctypes.create_string_buffer(bytes(lib.default_options()), B.OPT_SIZE)
    b = d.bwamem_hip_batch_upload(h, req, len(req))
    assert d.bwamem_hip_batch_keep_offsets(b, 1) == 0
    assert d.bwamem_hip_batch_encode_bam(b, 0, None, None) != 0, "encode before align"
    assert d.bwamem_hip_batch_bam_bytes(b) == 0
    assert d.bwamem_hip_batch_align(h, ob, None, b, 0) == 0
    for bad in (["a", "b" * 255, "c"], ["a", "", "c"]):
        blob, off = _names_arg(bad)
        assert d.bwamem_hip_batch_encode_bam(b, 0, blob, off) != 0, "a name of %d bytes" % len(bad[1])
        assert d.bwamem_hip_batch_bam_bytes(b) == 0
    blob, off = _names_arg(["a", "b" * 254, "c"])
    assert d.bwamem_hip_batch_encode_bam(b, 0, blob, off) == 0 and d.bwamem_hip_batch_bam_bytes(b) > 0
    assert d.bwamem_hip_batch_encode_bam(b, 0, blob, None) != 0, "names without offsets"
    d.bwamem_hip_batch_free(b)
    b = d.bwamem_hip_batch_upload(h, req, len(req))
    assert d.bwamem_hip_batch_align(h, ob, None, b, 0) == 0
    assert d.bwamem_hip_batch_encode_bam(b, 0, None, None) != 0, "encode without keep_offsets"
    assert d.bwamem_hip_batch_bam_bytes(b) == 0
    d.bwamem_hip_batch_free(b)
    assert d.bwamem_hip_batch_encode_bam(None, 0, None, None) != 0


def check_cigar_limit(lib):
    """n_cigar_op is 16 bits wide: 65 535 operations encode, 65 536 are an error (bam_encode.h's size function, called on the host)"""
    d = bind(lib)

    def rec(n_ops, nm=3, score=100, xs=-1, md=b"50", xa=b""):
        w = struct.pack("<7i", 0 << 16 | 60, 0, 1000, nm, score, xs, n_ops) + struct.pack("<I", 1 << 4 | 0) * n_ops
        for s in (md, xa):
            w += struct.pack("<i", len(s)) + s + b"\0" * (-len(s) % 4)
        return w
    l_read, l_name = 65535, 7
    w = rec(65535)
    fixed = 36 + l_name + 1 + (l_read + 1) // 2 + l_read
    assert d.bwamem_hip_bam_record_bytes(w, len(w) // 4, 0, l_read, l_name) == fixed + 4 * 65535 + (3 + 1) + (3 + 2 + 1) + (3 + 1)
    w = rec(65536)
    assert d.bwamem_hip_bam_record_bytes(w, len(w) // 4, 0, 65536, l_name) == -1
    # integer widths, XS present, XA present
    w = rec(1, nm=300, score=70000, xs=0, md=b"", xa=b"chr1,+5,1M,0;")
    assert d.bwamem_hip_bam_record_bytes(w, len(w) // 4, 0, 1, 1) == 36 + 2 + 4 + 1 + 1 + (3 + 2) + (3 + 4) + (3 + 1) + (3 + 13 + 1)
    assert d.bwamem_hip_bam_record_bytes(w, len(w) // 4 - 1, 0, 1, 1) == -2, "a truncated record"
    assert d.bwamem_hip_bam_record_bytes(w, len(w) // 4, 0, 1, 255) == -2


# ------------------------------------------------------------------------------------------ CPU suite (emulation build)
@pytest.fixture(scope="module")
def emu_index(small_genome):
    B.build_emu()
    emu = B.product_lib(emu=True)
    seqs, img = small_genome
    h = emu.open_index(img)
    yield emu, h, seqs
    emu.destroy_index(h)


def test_bam_records_match_sam_text(emu_index):
    emu, h, seqs = emu_index
    run_small_cases(emu, h, seqs)


def test_bam_header(emu_index):
    emu, h, seqs = emu_index
    check_header(emu, h, seqs)


def test_bgzf_framing(emu_index):
    check_bgzf(emu_index[0])


def test_align_to_bam_file(emu_index, tmp_path):
    emu, h, seqs = emu_index
    check_align_to_bam(emu, h, seqs, str(tmp_path))


def test_bam_errors(emu_index):
    emu, h, seqs = emu_index
    check_errors(emu, h, seqs)


def test_bam_cigar_op_limit(emu_index):
    check_cigar_limit(emu_index[0])


def test_bam_python_mirror(small_genome, tmp_path, monkeypatch):
    """BwaMemAligner.alignSeqsToBam over the emulation build (the mirror binds whatever LIBBWA_PATH names)"""
    B.build_emu()
    seqs, img = small_genome
    reads, _ = sam_writer_requests(seqs)
    r = subprocess.run([sys.executable, "-c", (
        "import sys; sys.path.insert(0, %r); import bwamem\n"
        "ix = bwamem.BwaMemIndex(%r); al = bwamem.BwaMemAligner(ix)\n"
        "reads = %r\n"
        "al.alignSeqsToBam(reads, %r, level=0)\n"
        "al.alignSeqsToBam(reads, %r, names=['n%%d' %% i for i in range(len(reads))], level=0)\n"
        "try:\n    al.alignSeqsToBam(reads, %r, names=['x'], level=0)\nexcept ValueError:\n    print('names-checked')\n"
        "al.close(); ix.close()\n") % (B.PKG, img, reads, str(tmp_path / "a.bam"), str(tmp_path / "b.bam"), str(tmp_path / "c.bam"))],
        env=dict(os.environ, LIBBWA_PATH=B.EMU_LIB), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "names-checked" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
    emu = B.product_lib(emu=True)
    h = emu.open_index(img)
    try:
        contigs = emu.contig_names(h)
        req = B.pack_request(reads)
        for fn, names in (("a.bam", None), ("b.bam", ["n%d" % i for i in range(len(reads))])):
            raw = gzip.decompress(open(str(tmp_path / fn), "rb").read())
            _, refs, used = parse_header(raw)
            assert [n for n, _ in refs] == contigs
            resp = emu.align_raw(h, emu.default_options(), req)
            assert to_sam(parse_records(raw[used:]), contigs) == _to_sam(emu, h, req, resp, False, names)
    finally:
        emu.destroy_index(h)


def test_bam_sanitizers(oracle, small_genome):
    """the BAM calls under AddressSanitizer + UBSan (tests/emu `make asan`), in a child process that preloads the runtimes"""
    B.make(os.path.join(B.ROOT, "tests", "emu"), "asan")
    libs = [subprocess.run(["gcc", "-print-file-name=" + n], capture_output=True, text=True).stdout.strip() for n in ("libasan.so", "libubsan.so")]
    if not all(os.path.isabs(x) and os.path.exists(x) for x in libs):
        pytest.skip("no sanitizer runtimes next to this gcc")
    seqs, img = small_genome
    env = dict(os.environ, LD_PRELOAD=":".join(libs), ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0")
    r = subprocess.run([sys.executable, os.path.join(B.ROOT, "tests", "bam_sanitized_child.py"), img, img[:-4]],
                       env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "sanitized-ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])


# ------------------------------------------------------------------------------------------ GPU suite
def _flags_seen(recs):
    return dict(xa=any(t == "XA" for r in recs for t, _, _ in r["tags"]), hard=any(CIG_OPS[c & 15] == "H" for r in recs for c in r["cig"]),
                rev=any(r["flag"] & 0x10 for r in recs), unmapped=any(r["flag"] & 4 for r in recs))


@pytest.mark.gpu
def test_gpu_bam_small_cases(hip_lib, small_genome, tmp_path):
    seqs, img = small_genome
    h = hip_lib.open_index(img)
    try:
        run_small_cases(hip_lib, h, seqs)
        check_header(hip_lib, h, seqs)
        check_bgzf(hip_lib)
        check_align_to_bam(hip_lib, h, seqs, str(tmp_path))
        check_errors(hip_lib, h, seqs)
        check_cigar_limit(hip_lib)
    finally:
        hip_lib.destroy_index(h)


@pytest.mark.gpu
def test_gpu_bam_medium_single_and_paired(hip_lib, medium_genome):
    seqs, img = medium_genome
    h = hip_lib.open_index(img)
    try:
        contigs = hip_lib.contig_names(h)
        g = seqs[0][1]
        reads = B.simulate_reads(seqs, 19990, length=150, seed=21, sub=0.02, indel=0.003)
        reads += [g[3000 + 500 * i:3080 + 500 * i] + B.revcomp(g[90000 + 700 * i:90070 + 700 * i]) for i in range(8)] + [b"", b"ACGT" * 30]
        assert len(reads) == 20000
        recs = check_batch(hip_lib, h, contigs, reads, hip_lib.default_options(), False, expected=False)
        seen = _flags_seen(recs)
        assert seen["hard"] and seen["rev"] and seen["unmapped"], seen
        check_batch(hip_lib, h, contigs, reads[:3000], hip_lib.default_options(), False, ["name:%d" % (7 * i) for i in range(3000)])
        pairs = B.simulate_pairs(seqs, 10000, length=150, seed=22, ins_mean=400, ins_sd=40)
        pairs[10] = b"ACGT" * 37
        po = B.set_opt(hip_lib.default_options(), flag=B.MEM_F_PE)
        precs = check_batch(hip_lib, h, contigs, pairs, po, True, expected=False)
        assert len({r["name"] for r in precs}) == 10000
        check_batch(hip_lib, h, contigs, pairs[:2001], po, True, pes=B.pack_pestat(200, 600, 400.0, 40.0))
    finally:
        hip_lib.destroy_index(h)


@pytest.mark.gpu
def test_gpu_bam_alt_genome(hip_lib, alt_genome):
    """ALT contigs: XA tags, is_alt records and the flag combinations that come with them"""
    seqs, img, _, _, regions = alt_genome
    h = hip_lib.open_index(img)
    try:
        contigs = hip_lib.contig_names(h)
        reads = B.reads_from_regions(seqs, regions, ["chr1_src", "chr2_src", "family", "chr1_alt1", "chr2_alt1", "chr1_alt2", "decoy"], 3000, length=150, seed=31, sub=0.01)
        g = seqs[0][1]
        reads += [g[42000 + 300 * i:42080 + 300 * i] + B.revcomp(g[20000 + 300 * i:20070 + 300 * i]) for i in range(10)] + [b"ACGT" * 30, b"N" * 40, b""]
        recs = check_batch(hip_lib, h, contigs, reads, hip_lib.default_options(), False)
        seen = _flags_seen(recs)
        assert all(seen.values()), seen
        pairs = B.pairs_from_regions(seqs, regions, ["chr1_src", "chr2_src", "chr1_alt1", "chr2_alt1"], 1500, length=100, seed=32, ins_mean=300, ins_sd=30)
        pairs[5] = b"ACGT" * 25
        po = B.set_opt(hip_lib.default_options(), flag=B.MEM_F_PE)
        precs = check_batch(hip_lib, h, contigs, pairs, po, True)
        pseen = _flags_seen(precs)
        assert pseen["xa"] and pseen["rev"] and pseen["unmapped"], pseen
    finally:
        hip_lib.destroy_index(h)


@pytest.mark.gpu
def test_gpu_bam_long_reads(hip_lib, medium_genome):
    """200 reads of 10 kb: tiles of long reads take the wavefront-per-read form of the emit kernel"""
    seqs, img = medium_genome
    h = hip_lib.open_index(img)
    try:
        contigs = hip_lib.contig_names(h)
        reads = B.simulate_reads(seqs, 196, length=10000, seed=41, sub=0.05, indel=0.01)
        g = seqs[0][1]
        reads += [g[10000:15000] + B.revcomp(g[200000:205000]), g[30000:34000] + g[300000:306000], b"ACGT" * 2500, B.revcomp(g[50000:60000])]
        recs = check_batch(hip_lib, h, contigs, reads, hip_lib.default_options(), False)
        assert any(len(r["cig"]) > 100 for r in recs) and any(CIG_OPS[c & 15] == "H" for r in recs for c in r["cig"])
        check_batch(hip_lib, h, contigs, reads[:50], hip_lib.default_options(), False, ["long/%d" % i for i in range(50)])
    finally:
        hip_lib.destroy_index(h)


@pytest.mark.gpu
def test_gpu_bam_shards_name_globally(hip_lib, medium_genome):
    """two shards of one logical call: the default names count from read_id0, single-end and paired-end"""
    seqs, img = medium_genome
    h = hip_lib.open_index(img)
    try:
        contigs = hip_lib.contig_names(h)
        reads = B.simulate_reads(seqs, 1000, length=150, seed=51)
        opts = hip_lib.default_options()
        a = check_batch(hip_lib, h, contigs, reads[:600], opts, False, read_id0=0, default_names=["r%d" % i for i in range(600)])
        b = check_batch(hip_lib, h, contigs, reads[600:], opts, False, read_id0=600, default_names=["r%d" % i for i in range(600, 1000)])
        assert {r["name"] for r in a + b} == {b"r%d\0" % i for i in range(1000)}
        pairs = B.simulate_pairs(seqs, 500, length=150, seed=52)
        po = B.set_opt(hip_lib.default_options(), flag=B.MEM_F_PE)
        pes = B.pack_pestat(200, 600, 400.0, 50.0)
        a = check_batch(hip_lib, h, contigs, pairs[:400], po, True, pes=pes, read_id0=0, default_names=["p%d" % (i >> 1) for i in range(400)])
        b = check_batch(hip_lib, h, contigs, pairs[400:], po, True, pes=pes, read_id0=400, default_names=["p%d" % (i >> 1) for i in range(400, 1000)])
        assert {r["name"] for r in a + b} == {b"p%d\0" % i for i in range(500)}
    finally:
        hip_lib.destroy_index(h)
