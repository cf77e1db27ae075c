"""FASTQ text taken apart on the device (csrc/fastq_parse.h, the k_fastq_* kernels in csrc/k_post.hip, bwamem_hip_batch_upload_fastq,
bwamem_hip_align_fastq_to_bam, BwaMemAligner.alignFastqToBam).  Nothing has a tolerance: Python writes FASTQ text from (reads, names,
qualities); after upload_fastq + align the response is byte-identical to batch_upload of pack_request(reads) + align, and the BAM
records are byte-identical to _encode_bam with the same names and set_qualities through the host calls.  Malformed text returns
NULL with the smallest offending read.
CPU suite: the emulation build runs the kernels.  GPU suite (-m gpu): the same on the device, the medium genome, long reads, the
file call, and the device's bytes against the emulation build's."""
import ctypes
import gzip
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bwalib as B
from test_bam_quals import RG_ID, RG_LINE, Batch, bindq, quals_blob, rand_quals, with_rg
from test_bam_sorted import check_file, python_sorted, split_records
from test_bam_writer import CIG_OPS, _flags_seen, _take, parse_header, parse_records

CHUNK = int(re.search(r"#define FASTQ_CHUNK (\d+)", open(os.path.join(B.PKG, "csrc", "fastq_parse.h")).read()).group(1))


def fastq_text(reads, names, quals, eol=b"\n", final=True, comments=None, suffix=None, plus=None):
    """comments[i]: what follows the name on line 1 (with its blank); suffix[i]: '/1' or '/2'; plus[i]: what follows the '+'"""
    out = []
    for i, (r, n, q) in enumerate(zip(reads, names, quals)):
        n = n if isinstance(n, bytes) else n.encode()
        out += [b"@" + n + (suffix[i] if suffix else b"") + (comments[i] if comments else b""), r, b"+" + (plus[i] if plus else b""), q]
    text = eol.join(out) + eol if out else b""
    return text if final or not out else text[:len(text) - len(eol)]


def upload(lib, h, t1, t2=None):
    d = bindq(lib)
    bad = ctypes.c_int64(-7)
    b = d.bwamem_hip_batch_upload_fastq(h, t1, len(t1), t2, len(t2) if t2 is not None else 0, ctypes.byref(bad))
    return b, bad.value


_host_cache = {}


def host_path(lib, h, opts, reads, names, quals, paired, pes):
    """the request path: batch_upload of pack_request(reads), set_qualities, _encode_bam with the names -> (response, records)"""
    key = (lib.path, h, tuple(reads), tuple(names), tuple(quals), paired)
    if key not in _host_cache:
        bt = Batch(lib, h, opts, B.pack_request(reads), pes)
        try:
            assert bt.set_quals(list(quals)) == 0
            _host_cache[key] = (bt.resp, bt.encode(paired, list(names)))
        finally:
            bt.free()
    return _host_cache[key]


def fastq_path(lib, h, opts, t1, t2, paired, pes, rg=None):
    b, bad = upload(lib, h, t1, t2)
    assert b, "upload_fastq refused the text (bad_record %d)" % bad
    bt = Batch(lib, h, opts, None, pes, b=b)
    try:
        if rg is not None:
            assert bt.set_rg(rg) == 0
        return bt.resp, bt.encode(paired)
    finally:
        bt.free()


def check_same(lib, h, opts, reads, names, quals, paired, pes, t1, t2=None):
    want = host_path(lib, h, opts, reads, names, quals, paired, pes)
    got = fastq_path(lib, h, opts, t1, t2, paired, pes)
    assert got[0] == want[0], "the response differs from the request path's"
    assert got[1] == want[1], "the records differ from the host-API path's"
    return want


def small_set(seqs, seed=3):
    """reads of every kind the issue names, with names and qualities of every kind it names"""
    g = seqs[0][1]
    reads = B.simulate_reads(seqs, 6, length=70, seed=seed, sub=0.02)
    reads += [g[3000:3060] + B.revcomp(g[9000:9070]), b"", b"T", g[500:560].lower(), g[700:730] + b"NNnn" + g[734:760], b"ACGT" * 12]
    names = ["read%d" % i for i in range(len(reads))]
    names[1], names[2] = "N" * 254, "n"
    quals = rand_quals(reads, seed + 1)
    quals[0] = b"@" + quals[0][1:]
    quals[3] = b"+" + quals[3][1:]
    return reads, names, quals


def pair_set(seqs):
    pairs = B.simulate_pairs(seqs, 5, length=70, seed=5, ins_mean=300, ins_sd=30)
    pairs[3] = b"ACGT" * 20
    names = ["frag%d" % (i >> 1) for i in range(len(pairs))]
    return pairs, names, rand_quals(pairs, 6)


def check_text_forms(lib, h, seqs):
    """the same reads through every spelling of the text"""
    opts = lib.default_options()
    reads, names, quals = small_set(seqs)
    n = len(reads)
    a = (lib, h, opts, reads, names, quals, False, None)
    check_same(*a, fastq_text(reads, names, quals))
    check_same(*a, fastq_text(reads, names, quals, eol=b"\r\n"))
    check_same(*a, fastq_text(reads, names, quals, final=False))
    check_same(*a, fastq_text(reads, names, quals, eol=b"\r\n", final=False))
    comments = [(b" 1:N:0:ACGT", b"\tcomment with blanks", b" ", b"")[i % 4] for i in range(n)]
    suffix = [(b"/1", b"/2", b"")[i % 3] for i in range(n)]
    plus = [(b"", b"read%d" % i, b"@+")[i % 3] for i in range(n)]
    check_same(*a, fastq_text(reads, names, quals, comments=comments, suffix=suffix, plus=plus))
    # a name that keeps what only looks like a read number
    odd = ["a/3", "/1", "b/1/2", "c/"] + names[4:]
    want = ["a/3", "/1", "b/1", "c/"] + names[4:]
    check_same(lib, h, opts, reads, want, quals, False, None, fastq_text(reads, odd, quals))
    # shorter than one chunk, and exactly one chunk
    few = (reads[:3], names[:3], quals[:3])
    t = fastq_text(*few)
    assert len(t) < CHUNK
    check_same(lib, h, opts, *few, False, None, t)
    pad = CHUNK - len(t) - 1
    for extra, final in ((0, True), (0, False), (1, False)):           # exactly one chunk; one byte less; one chunk without its last newline
        t = fastq_text(*few, comments=[b" " + b"c" * (pad + extra), b"", b""], final=final)
        assert len(t) == CHUNK + extra - (0 if final else 1)
        check_same(lib, h, opts, *few, False, None, t)
    b, bad = upload(lib, h, b"")
    assert b, "an empty text holds no record"
    bindq(lib).bwamem_hip_batch_free(b)


def check_chunk_edges(lib, h, seqs):
    """for each of the four line kinds, the line's newline on byte k * CHUNK - 1 and on k * CHUNK; and the text cut after it"""
    opts = lib.default_options()
    reads, names, quals = small_set(seqs)
    few = (reads[:2] + reads[6:9], names[:2] + names[6:9], quals[:2] + quals[6:9])      # (a 254-byte name, an empty and a 1-base read)
    base = fastq_text(*few)
    lines = base.split(b"\n")[:-1]
    for kind in range(4):
        line = 4 * 3 + kind                                            # of the record of the empty read
        nl = sum(len(l) + 1 for l in lines[:line + 1]) - 1             # where its newline is without padding
        for k in (1, 2):
            for target in (k * CHUNK - 1, k * CHUNK):
                pad = target - nl
                assert pad >= 1
                t = fastq_text(*few, comments=[b" " + b"p" * (pad - 1)] + [b""] * 4)
                assert t[target] == 10 and t[:target + 1].count(b"\n") == line + 1
                check_same(lib, h, opts, *few, False, None, t)
                if kind == 3 and k == 1:                               # ... on the last byte of the text, CR LF too
                    check_same(lib, h, opts, few[0][:4], few[1][:4], few[2][:4], False, None, t[:target + 1])
                    tr = fastq_text(*few, eol=b"\r\n", comments=[b" " + b"p" * (pad - 1 - line - 1)] + [b""] * 4)
                    assert tr[target] == 10
                    check_same(lib, h, opts, *few, False, None, tr)
                elif k == 1:                                           # the text ends inside a record: no single record's error
                    b, bad = upload(lib, h, t[:target + 1])
                    assert not b and bad == -1, (kind, bad)


def check_pairs(lib, h, seqs):
    po = B.set_opt(lib.default_options(), flag=B.MEM_F_PE)
    pes = B.pack_pestat(150, 450, 300.0, 30.0)
    pairs, names, quals = pair_set(seqs)
    inter = fastq_text(pairs, names, quals, suffix=[(b"/1", b"/2")[i & 1] for i in range(len(pairs))])
    t1 = fastq_text(pairs[0::2], names[0::2], quals[0::2], suffix=[b"/1"] * 5)
    t2 = fastq_text(pairs[1::2], names[1::2], quals[1::2], suffix=[b"/2"] * 5, eol=b"\r\n", final=False)
    want = check_same(lib, h, po, pairs, names, quals, True, pes, inter)
    check_same(lib, h, po, pairs, names, quals, True, pes, t1, t2)
    assert len({r["name"] for r in parse_records(want[1])}) == 5
    # an odd trailing read of one interleaved text keeps today's behaviour: no record
    odd = (pairs + [pairs[0]], names + ["tail"], quals + [quals[0]])
    check_same(lib, h, po, *odd, True, pes, fastq_text(*odd))
    # interleaved text whose mates' names differ: upload takes it (it may be single-end), a paired encode refuses it
    wrong = list(names)
    wrong[5] = "other"
    b, bad = upload(lib, h, fastq_text(pairs, wrong, quals))
    assert b
    bt = Batch(lib, h, po, None, pes, b=b)
    try:
        d = bindq(lib)
        assert d.bwamem_hip_batch_encode_bam(bt.b, 1, None, None) != 0 and d.bwamem_hip_batch_bam_bytes(bt.b) == 0
        assert d.bwamem_hip_batch_encode_bam(bt.b, 0, None, None) == 0
    finally:
        bt.free()


def check_errors(lib, h, seqs):
    reads, names, quals = small_set(seqs)
    good = fastq_text(reads, names, quals)

    def text(edit, **kw):
        """edit: {(record, line kind): function of the line}"""
        lines = fastq_text(reads, names, quals, **kw).split(b"\n")
        for (rec, kind), f in edit.items():
            lines[4 * rec + kind] = f(lines[4 * rec + kind])
        return b"\n".join(lines)
    cases = {"a missing +": ({(4, 2): lambda l: b"-" + l[1:]}, 4), "an empty + line": ({(2, 2): lambda l: b""}, 2),
             "a missing @": ({(5, 0): lambda l: l[1:]}, 5), "a quality a byte short": ({(3, 3): lambda l: l[:-1]}, 3),
             "a quality a byte long": ({(0, 3): lambda l: l + b"I"}, 0), "a quality on the empty read": ({(7, 3): lambda l: b"I"}, 7),
             "a quality byte 32": ({(9, 3): lambda l: l[:5] + b" " + l[6:]}, 9), "a quality byte 127": ({(9, 3): lambda l: l[:5] + b"\x7f" + l[6:]}, 9),
             "a 255-byte name": ({(1, 0): lambda l: l + b"N"}, 1), "an empty name": ({(2, 0): lambda l: b"@ comment"}, 2),
             "a name that is only a read number's worth": ({(2, 0): lambda l: b"@"}, 2),
             "two errors: the smaller index": ({(8, 2): lambda l: b"x", (3, 0): lambda l: b">" + l[1:]}, 3),
             "two errors, the other way round": ({(3, 2): lambda l: b"x", (8, 0): lambda l: b">" + l[1:]}, 3),
             "the first record": ({(0, 0): lambda l: b""}, 0), "the last record": ({(len(reads) - 1, 3): lambda l: l[:-1]}, len(reads) - 1)}
    for what, (edit, want) in cases.items():
        b, bad = upload(lib, h, text(edit))
        assert not b and bad == want, (what, bad)
    b, bad = upload(lib, h, text({(9, 3): lambda l: l[:5] + b" " + l[6:]}, eol=b"\n").replace(b"\n", b"\r\n"))
    assert not b and bad == 9, "CR LF text"
    for what, t in {"a line short": good[:good.rindex(b"\n", 0, -1) + 1], "a line more": good + b"@x\n", "a blank line at the end": good + b"\n",
                    "one line": b"@x", "a wrapped sequence": fastq_text([b"ACGT\nACGT"], ["w"], [b"IIIIIIII"])}.items():
        b, bad = upload(lib, h, t)
        assert not b and bad == -1, (what, bad)
    b, bad = upload(lib, h, fastq_text([b"ACGT\nACGT"] * 2, ["w", "v"], [b"IIII\nIIII"] * 2))
    assert not b and bad == 0, ("wrapped records whose lines happen to add up to a multiple of four fail the '+' check", bad)
    # two texts
    pairs, pnames, pquals = pair_set(seqs)
    t1 = fastq_text(pairs[0::2], pnames[0::2], pquals[0::2])
    t2 = fastq_text(pairs[1::2], pnames[1::2], pquals[1::2])
    b, bad = upload(lib, h, t1, fastq_text(pairs[1:8:2], pnames[1:8:2], pquals[1:8:2]))
    assert not b and bad == -1, "unequal record counts"
    wrong = list(pnames[1::2])
    wrong[3] = "other"
    wrong[4] = wrong[4] + "x"
    b, bad = upload(lib, h, t1, fastq_text(pairs[1::2], wrong, pquals[1::2]))
    assert not b and bad == 6, ("mate names that differ", bad)
    b, bad = upload(lib, h, t1, t2.replace(b"\n+\n", b"\n-\n", 3).replace(b"\n-\n", b"\n+\n", 2))
    assert not b and bad == 5, ("an error in the second text counts reads of the batch", bad)
    d = bindq(lib)
    assert not d.bwamem_hip_batch_upload_fastq(None, good, len(good), None, 0, None)
    b = d.bwamem_hip_batch_upload_fastq(h, good, len(good), None, 0, None)
    assert b, "bad_record may be NULL"
    d.bwamem_hip_batch_free(b)


def fastq_file(lib, h, opts, t1, t2, rg, sort, path, bai_path, pes=None, write_header=True):
    d = bindq(lib)
    ob = ctypes.create_string_buffer(bytes(opts), B.OPT_SIZE)
    pb = ctypes.create_string_buffer(pes, len(pes)) if pes is not None else None
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    fb = os.open(bai_path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644) if bai_path else -1
    try:
        return d.bwamem_hip_align_fastq_to_bam(h, ob, pb, t1, len(t1), t2, len(t2) if t2 is not None else 0, rg, 1 if sort else 0, fd, fb, 1 if write_header else 0)
    finally:
        os.close(fd)
        if fb >= 0:
            os.close(fb)


def header_rg(lib, h, sorted_, rg):
    d = bindq(lib)
    sz = ctypes.c_size_t()
    p = d.bwamem_hip_bam_header_rg(h, 1 if sorted_ else 0, rg, ctypes.byref(sz))
    assert p
    return _take(lib, p, sz.value)


def check_file_call(lib, h, n_ref, opts, reads, names, quals, paired, pes, t1, t2, tmpdir):
    """bwamem_hip_align_fastq_to_bam, sorted with an index and unsorted without: the records are the batch calls' with RG appended"""
    _, bam = host_path(lib, h, opts, reads, names, quals, paired, pes)
    recs = b"".join(with_rg(r, RG_ID) for r in split_records(bam))
    path, bpath = os.path.join(tmpdir, "f.bam"), os.path.join(tmpdir, "f.bam.bai")
    assert fastq_file(lib, h, opts, t1, t2, RG_LINE, True, path, bpath, pes) == 0
    check_file(open(path, "rb").read(), open(bpath, "rb").read(), header_rg(lib, h, True, RG_LINE), python_sorted(recs), n_ref)
    parsed = parse_records(python_sorted(recs))
    assert all(len(r["qual"]) == r["l_seq"] and all(q <= 93 for q in r["qual"]) and r["tags"][-1] == ("RG", "Z", RG_ID.decode()) for r in parsed)
    assert fastq_file(lib, h, opts, t1, t2, None, False, path, None, pes) == 0
    assert gzip.decompress(open(path, "rb").read()) == header_rg(lib, h, False, None) + bam
    assert fastq_file(lib, h, opts, t1, t2, None, False, path, bpath, pes) != 0 and os.path.getsize(path) == 0, "an index needs a sorted file"
    assert fastq_file(lib, h, opts, t1[:-9], t2, None, True, path, None, pes) != 0 and os.path.getsize(path) == 0, "malformed text writes nothing"
    return parsed


def run_small_cases(lib, h, seqs, tmpdir):
    check_text_forms(lib, h, seqs)
    check_chunk_edges(lib, h, seqs)
    check_pairs(lib, h, seqs)
    check_errors(lib, h, seqs)
    reads, names, quals = small_set(seqs)
    check_file_call(lib, h, len(seqs), lib.default_options(), reads, names, quals, False, None, fastq_text(reads, names, quals), None, tmpdir)


# ------------------------------------------------------------------------------------------ CPU suite (emulation build)
@pytest.fixture(scope="module")
def emu_index(small_genome):
    B.build_emu()
    emu = B.product_lib(emu=True)
    seqs, img = small_genome
    h = emu.open_index(img)
    yield emu, h, seqs
    emu.destroy_index(h)


def test_fastq_text_forms_match_the_request_path(emu_index):
    check_text_forms(*emu_index)


def test_fastq_newlines_on_chunk_edges(emu_index):
    check_chunk_edges(*emu_index)


def test_fastq_pairs_two_texts_and_interleaved(emu_index):
    check_pairs(*emu_index)


def test_fastq_errors_name_the_smallest_record(emu_index):
    check_errors(*emu_index)


def test_fastq_file_call(emu_index, tmp_path):
    emu, h, seqs = emu_index
    reads, names, quals = small_set(seqs)
    check_file_call(emu, h, len(seqs), emu.default_options(), reads, names, quals, False, None, fastq_text(reads, names, quals), None, str(tmp_path))
    pairs, pnames, pquals = pair_set(seqs)
    po = B.set_opt(emu.default_options(), flag=B.MEM_F_PE)
    check_file_call(emu, h, len(seqs), po, pairs, pnames, pquals, True, B.pack_pestat(150, 450, 300.0, 30.0),
                    fastq_text(pairs[0::2], pnames[0::2], pquals[0::2]), fastq_text(pairs[1::2], pnames[1::2], pquals[1::2]), str(tmp_path))


def test_fastq_python_mirror(emu_index, small_genome, tmp_path):
    """BwaMemAligner.alignFastqToBam and alignSeqsToBam(quals=..., read_group=...) over the emulation build, in a child process"""
    emu, h, seqs = emu_index
    _, img = small_genome
    reads, names, quals = small_set(seqs)
    fq = str(tmp_path / "in.fq")
    with open(fq, "wb") as f:
        f.write(fastq_text(reads, names, quals))
    p = {k: str(tmp_path / k) for k in ("a.bam", "a.bam.bai", "b.bam", "c.bam", "d.bam", "d.bai")}
    r = subprocess.run([sys.executable, "-c", (
        "import sys; sys.path.insert(0, %r); import bwamem\n"
        "ix = bwamem.BwaMemIndex(%r); al = bwamem.BwaMemAligner(ix)\n"
        "reads, names, quals, rg, p = %r, %r, %r, %r, %r\n"
        "al.alignFastqToBam(%r, p['a.bam'], read_group=rg, sort=True, index_path=p['a.bam.bai'])\n"
        "al.alignFastqToBam(open(%r, 'rb').read(), p['b.bam'])\n"
        "al.alignSeqsToBam(reads, p['c.bam'], names=names, quals=quals, read_group=rg)\n"
        "al.alignSeqsToBam(reads, p['d.bam'], quals=quals, sort=True, index_path=p['d.bai'])\n"
        "try:\n    al.alignSeqsToBam(reads, p['c.bam'] + 'x', quals=quals[:-1])\nexcept ValueError:\n    print('quals-checked')\n"
        "try:\n    al.alignSeqsToBam(reads, p['c.bam'] + 'x', read_group='RG')\nexcept ValueError:\n    print('rg-checked')\n"
        "try:\n    al.alignFastqToBam(b'@x\\nAC\\n+\\nI\\n', p['c.bam'] + 'y')\nexcept RuntimeError:\n    print('fastq-checked')\n"
        "al.close(); ix.close()\n") % (B.PKG, img, reads, names, quals, RG_LINE.decode(), p, fq, fq)],
        env=dict(os.environ, LIBBWA_PATH=B.EMU_LIB), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and all(w in r.stdout for w in ("quals-checked", "rg-checked", "fastq-checked")), (r.stdout[-500:], r.stderr[-2000:])
    assert not os.path.exists(p["c.bam"] + "x")
    opts = emu.default_options()
    _, bam = host_path(emu, h, opts, reads, names, quals, False, None)
    tagged = b"".join(with_rg(x, RG_ID) for x in split_records(bam))
    check_file(open(p["a.bam"], "rb").read(), open(p["a.bam.bai"], "rb").read(), header_rg(emu, h, True, RG_LINE), python_sorted(tagged), len(seqs))
    assert gzip.decompress(open(p["b.bam"], "rb").read()) == header_rg(emu, h, False, None) + bam
    assert gzip.decompress(open(p["c.bam"], "rb").read()) == header_rg(emu, h, False, RG_LINE) + tagged
    bt = Batch(emu, h, opts, B.pack_request(reads))
    try:
        assert bt.set_quals(list(quals)) == 0
        default_named = bt.encode(False)
    finally:
        bt.free()
    check_file(open(p["d.bam"], "rb").read(), open(p["d.bai"], "rb").read(), header_rg(emu, h, True, None), python_sorted(default_named), len(seqs))


def test_fastq_sanitizers(small_genome, tmp_path):
    """the FASTQ calls under AddressSanitizer + UBSan: a stand-alone driver (tests/fastq_sanitized_driver.cpp), compiled here with
    the sanitizers and linked against the sanitized emulation build (tests/emu `make asan`), run as a program"""
    B.make(os.path.join(B.ROOT, "tests", "emu"), "asan")
    seqs, img = small_genome
    reads, names, quals = small_set(seqs)
    pairs, pnames, pquals = pair_set(seqs)
    files = {"se.fq": fastq_text(reads, names, quals), "crlf.fq": fastq_text(reads, names, quals, eol=b"\r\n", final=False),
             "edge.fq": fastq_text(reads, names, quals, comments=[b" " + b"p" * (CHUNK - 2 - len(names[0]))] + [b""] * (len(reads) - 1)),
             "p1.fq": fastq_text(pairs[0::2], pnames[0::2], pquals[0::2]), "p2.fq": fastq_text(pairs[1::2], pnames[1::2], pquals[1::2]),
             "bad_plus.fq": fastq_text(reads, names, quals).replace(b"\n+\n", b"\n-\n"), "bad_lines.fq": fastq_text(reads, names, quals)[:-80],
             "bad_qual.fq": fastq_text(reads[:3], names[:3], [quals[0], quals[1][:-1], quals[2]]), "empty.fq": b"", "one.fq": b"@",
             "req.bin": B.pack_request(reads), "qual.bin": quals_blob(quals)}
    for k, v in files.items():
        with open(str(tmp_path / k), "wb") as f:
            f.write(v)
    manifest = ["ok se.fq - 0", "ok crlf.fq - 0", "ok edge.fq - 0", "ok p1.fq p2.fq 1", "ok empty.fq - 0", "bad bad_plus.fq - 0", "bad bad_lines.fq - -1",
                "bad bad_qual.fq - 1", "bad one.fq - -1", "bad p1.fq se.fq -1", "req req.bin qual.bin 0"]
    with open(str(tmp_path / "manifest.txt"), "w") as f:
        f.write("\n".join(manifest) + "\n")
    emu_dir = os.path.join(B.ROOT, "tests", "emu", "_build")
    exe = str(tmp_path / "fastq_sanitized_driver")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(B.ROOT, "include"), os.path.join(B.ROOT, "tests", "fastq_sanitized_driver.cpp"), "-o", exe,
                    "-L", emu_dir, "-lbwamem_emu_asan", "-Wl,-rpath," + emu_dir], check=True)
    r = subprocess.run([exe, img, str(tmp_path)], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0"),
                       capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "sanitized-ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


# ------------------------------------------------------------------------------------------ GPU suite
@pytest.mark.gpu
def test_gpu_fastq_small_cases(hip_lib, small_genome, tmp_path):
    seqs, img = small_genome
    h = hip_lib.open_index(img)
    try:
        run_small_cases(hip_lib, h, seqs, str(tmp_path))
    finally:
        hip_lib.destroy_index(h)


@pytest.mark.gpu
def test_gpu_fastq_equals_emulation(hip_lib, small_genome):
    """the records of the FASTQ-built batch: device bytes == emulation bytes"""
    B.build_emu()
    emu = B.product_lib(emu=True)
    seqs, img = small_genome
    h, he = hip_lib.open_index(img), emu.open_index(img)
    try:
        reads, names, quals = small_set(seqs)
        t = fastq_text(reads, names, quals, eol=b"\r\n", comments=[b" c"] * len(reads))
        assert fastq_path(hip_lib, h, hip_lib.default_options(), t, None, False, None, RG_LINE) == fastq_path(emu, he, emu.default_options(), t, None, False, None, RG_LINE)
        pairs, pnames, pquals = pair_set(seqs)
        po = B.set_opt(hip_lib.default_options(), flag=B.MEM_F_PE)
        pes = B.pack_pestat(150, 450, 300.0, 30.0)
        t1, t2 = fastq_text(pairs[0::2], pnames[0::2], pquals[0::2]), fastq_text(pairs[1::2], pnames[1::2], pquals[1::2])
        assert fastq_path(hip_lib, h, po, t1, t2, True, pes) == fastq_path(emu, he, po, t1, t2, True, pes)
    finally:
        hip_lib.destroy_index(h)
        emu.destroy_index(he)


def _medium_names(n, rng):
    return ["M%05d:%d:FC:%d:%d" % (i, i % 8, int(rng.integers(1000, 30000)), i * 7) for i in range(n)]


@pytest.mark.gpu
def test_gpu_fastq_medium_single_end(hip_lib, medium_genome):
    """20 000 x 150 bp from FASTQ text: several chunks per workgroup grid, several tiles"""
    seqs, img = medium_genome
    h = hip_lib.open_index(img)
    try:
        g = seqs[0][1]
        reads = B.simulate_reads(seqs, 19990, length=150, seed=21, sub=0.02, indel=0.003)
        reads += [g[3000 + 500 * i:3080 + 500 * i] + B.revcomp(g[90000 + 700 * i:90070 + 700 * i]) for i in range(8)] + [b"", b"ACGT" * 30]
        names = _medium_names(len(reads), np.random.default_rng(1))
        quals = rand_quals(reads, 2)
        opts = hip_lib.default_options()
        _, bam = check_same(hip_lib, h, opts, reads, names, quals, False, None, fastq_text(reads, names, quals, comments=[b" 1:N:0"] * len(reads)))
        recs = parse_records(bam)
        seen = _flags_seen(recs)
        assert seen["hard"] and seen["rev"] and seen["unmapped"], seen
        assert all(len(r["qual"]) == r["l_seq"] and all(q <= 93 for q in r["qual"]) for r in recs)
    finally:
        hip_lib.destroy_index(h)


@pytest.mark.gpu
def test_gpu_fastq_medium_paired(hip_lib, medium_genome):
    """10 000 pairs from two texts"""
    seqs, img = medium_genome
    h = hip_lib.open_index(img)
    try:
        pairs = B.simulate_pairs(seqs, 10000, length=150, seed=22, ins_mean=400, ins_sd=40)
        pairs[10] = b"ACGT" * 37
        frag = _medium_names(10000, np.random.default_rng(3))
        names = [frag[i >> 1] for i in range(20000)]
        quals = rand_quals(pairs, 4)
        po = B.set_opt(hip_lib.default_options(), flag=B.MEM_F_PE)
        t1 = fastq_text(pairs[0::2], names[0::2], quals[0::2], suffix=[b"/1"] * 10000)
        t2 = fastq_text(pairs[1::2], names[1::2], quals[1::2], suffix=[b"/2"] * 10000, final=False)
        _, bam = check_same(hip_lib, h, po, pairs, names, quals, True, None, t1, t2)
        recs = parse_records(bam)
        assert len({r["name"] for r in recs}) == 10000
        seen = _flags_seen(recs)
        assert seen["rev"] and seen["unmapped"], seen
    finally:
        hip_lib.destroy_index(h)


@pytest.mark.gpu
def test_gpu_fastq_long_reads(hip_lib, medium_genome):
    """200 x 10 kb: the wavefront-per-read forms of the copy and emit kernels, qualities through both"""
    seqs, img = medium_genome
    h = hip_lib.open_index(img)
    try:
        reads = B.simulate_reads(seqs, 194, length=10000, seed=41, sub=0.05, indel=0.01)
        g = seqs[0][1]
        reads += [g[10000:15000] + B.revcomp(g[200000:205000]), g[30000:34000] + g[300000:306000], b"ACGT" * 2500, B.revcomp(g[50000:60000])]
        reads += [g[70000:76000] + B.revcomp(g[400000:404000]), B.revcomp(g[420000:424000]) + g[90000:96000]]      # the shorter, later record on the reverse strand
        assert len(reads) == 200
        names = ["long:%d" % i for i in range(len(reads))]                    # (a trailing /1 or /2 would be removed)
        quals = rand_quals(reads, 8)
        _, bam = check_same(hip_lib, h, hip_lib.default_options(), reads, names, quals, False, None, fastq_text(reads, names, quals, eol=b"\r\n"))
        recs = parse_records(bam)
        assert any(r["flag"] & 0x10 and r["cig"] and "H" in (CIG_OPS[r["cig"][0] & 15], CIG_OPS[r["cig"][-1] & 15]) for r in recs), "no hard-clipped reverse-strand record"
        assert all(len(r["qual"]) == r["l_seq"] and all(q <= 93 for q in r["qual"]) for r in recs)
    finally:
        hip_lib.destroy_index(h)


@pytest.mark.gpu
def test_gpu_fastq_file_call(hip_lib, medium_genome, tmp_path):
    """bwamem_hip_align_fastq_to_bam, sort = 1 with an index, 2 000 reads with a read group"""
    seqs, img = medium_genome
    h = hip_lib.open_index(img)
    try:
        reads = B.simulate_reads(seqs, 1998, length=150, seed=61, sub=0.02, indel=0.003) + [b"", b"ACGT" * 30]
        names = _medium_names(len(reads), np.random.default_rng(5))
        quals = rand_quals(reads, 6)
        parsed = check_file_call(hip_lib, h, len(seqs), hip_lib.default_options(), reads, names, quals, False, None, fastq_text(reads, names, quals), None, str(tmp_path))
        assert len(parsed) >= 2000
    finally:
        hip_lib.destroy_index(h)
