"""SA, MC and MQ tags in BAM and SAM records (the rule at the top of csrc/bam_encode.h; k_bam_tag_size / k_bam_tag_text and the tagged
forms of k_bam_size / k_bam_emit in csrc/k_post.hip; bwamem_hip_batch_set_tags, bwamem_hip_response_to_sam_tags,
bwamem_hip_fastq_to_bam).  Nothing has a tolerance.  The expected tags come from a formatter written here from the rule over
B.decode_response; it shares no code with either writer.  The same aligned batch is encoded without and with the tags: every
record with them is the record without them with the expected tag bytes inserted before RG (or at the end) and block_size
corrected; the decoded text equals bwamem_hip_response_to_sam_tags line for line, which equals the untagged writer's lines with
the formatter's text inserted.  The tests assert on their own inputs that every clause of the rule is met by some record.
CPU suite: the emulation build runs the kernels.  GPU suite (-m gpu): the same cases on the device."""
import ctypes
import gzip
import os
import struct
import subprocess
import sys

import pytest

import bwalib as B
from test_bam_dup import DupCounts
from test_bam_quals import RG_ID, RG_LINE, Batch, rand_quals, to_sam_q
from test_bam_sorted import check_file, rec_key, split_records
from test_bam_writer import CIG_OPS, _take, parse_header, parse_records, sam_writer_requests, to_sam
from test_fastq_device import fastq_text, header_rg
from test_fastq_gz import bgzf_cut, bindgz

SA, MC, MQ = 1, 2, 4
ORDER = ("NM", "MD", "AS", "XS", "XA", "SA", "MC", "MQ", "RG")
PES = B.pack_pestat(150, 450, 300.0, 30.0)


class BamOptions(ctypes.Structure):
    _fields_ = [("size", ctypes.c_size_t), ("rg_line", ctypes.c_char_p), ("sort", ctypes.c_int), ("mark_dup", ctypes.c_int), ("tags", ctypes.c_uint),
                ("write_header", ctypes.c_int)]


def bindt(lib):
    d = bindgz(lib)
    if getattr(d, "_tags_bound", False):
        return d
    vp, sz, cp, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_int
    d.bwamem_hip_batch_set_tags.argtypes = [vp, ctypes.c_uint]
    d.bwamem_hip_response_to_sam_tags.restype = vp
    d.bwamem_hip_response_to_sam_tags.argtypes = [vp, cp, cp, sz, vp, ci, cp, cp, ctypes.c_uint, ctypes.POINTER(sz)]
    d.bwamem_hip_fastq_to_bam.argtypes = [vp, vp, vp, cp, sz, cp, sz, ctypes.POINTER(BamOptions), ci, ci, ctypes.POINTER(DupCounts)]
    d._tags_bound = True
    return d


def to_sam_tags(lib, h, req, resp, paired, quals, rg_id, mask):
    d = bindt(lib)
    sz = ctypes.c_size_t()
    q = b"".join(x + b"\0" for x in quals) if quals is not None else None
    p = d.bwamem_hip_response_to_sam_tags(h, req, resp, len(resp), None, 1 if paired else 0, q, rg_id, mask, ctypes.byref(sz))
    assert p, "bwamem_hip_response_to_sam_tags returned NULL"
    return _take(lib, p, sz.value).decode()


# ------------------------------------------------------------------------------------------ the rule in Python
def expected_tags(dec, contigs, paired, mask):
    """per record, in response order: the (tag, type, value) triples of SA / MC / MQ the rule of bam_encode.h gives it"""
    out = []
    for r, alns in enumerate(dec):
        listed = [k for k, a in enumerate(alns) if not a["flag"] & 4 and not a["flag"] & 0x100]
        entry = {k: "%s,%d,%s,%s,%d,%d;" % (contigs[alns[k]["rid"]], alns[k]["pos"] + 1, "-" if alns[k]["flag"] & 0x10 else "+", alns[k]["cigar"] or "*",
                                            alns[k]["mapq"], alns[k]["nm"]) for k in listed}
        mate = dec[r ^ 1] if paired and (r ^ 1) < len(dec) else []
        m0 = mate[0] if mate and not mate[0]["flag"] & 4 else None
        for k in range(len(alns)):
            t = []
            if mask & SA and k in listed and len(listed) >= 2:
                t.append(("SA", "Z", "".join(entry[j] for j in listed if j != k)))
            if m0 is not None and mask & MC:
                t.append(("MC", "Z", m0["cigar"] or "*"))
            if m0 is not None and mask & MQ:
                t.append(("MQ", "C", m0["mapq"]))
            out.append(t)
    return out


def tag_bytes(tags):
    return b"".join(t.encode() + (b"Z" + v.encode() + b"\0" if ty == "Z" else b"C" + bytes([v])) for t, ty, v in tags)


def tag_text(tags):
    return "".join("\t%s:%s:%s" % (t, "Z" if ty == "Z" else "i", v) for t, ty, v in tags)


def with_tags(raw, tags, rg_id):
    """the untagged record with the tags before RG (which, when there, is the record's end) and block_size corrected"""
    add = tag_bytes(tags)
    tail = b"RGZ" + rg_id + b"\0" if rg_id else b""
    assert raw.endswith(tail)
    body = raw[4:len(raw) - len(tail)] + add + tail
    return struct.pack("<i", len(body)) + body


def line_with_tags(line, tags, rg_id):
    tail = "\tRG:Z:" + rg_id.decode() if rg_id else ""
    assert line.endswith(tail)
    return line[:len(line) - len(tail)] + tag_text(tags) + tail


def without_tags(raw):
    """a record with SA / MC / MQ taken out and block_size corrected (test 8)"""
    r = parse_records(raw)[0]
    p = 36 + r["l_rn"] + 4 * len(r["cig"]) + (r["l_seq"] + 1) // 2 + r["l_seq"]
    out = raw[4:p]
    for t, ty, v in r["tags"]:
        n = 3 + (len(v) + 1 if ty == "Z" else struct.calcsize({"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I"}[ty]))
        if t not in ("SA", "MC", "MQ"):
            out += raw[p:p + n]
        p += n
    assert p == len(raw)
    return struct.pack("<i", len(out)) + out


_repeat = {}


def repeat_read(seqs, k=60):
    """k bases that occur twice in the genome, exactly: a read of them maps with mapping quality 0, and under MEM_F_ALL gets a 0x100 record"""
    key = id(seqs)
    if key not in _repeat:
        seen, found = {}, None
        for ci, (_, s) in enumerate(seqs):
            for i in range(len(s) - k):
                w = s[i:i + k]
                if b"N" in w:
                    continue
                if w in seen or B.revcomp(w) in seen:
                    found = w
                    break
                seen[w] = (ci, i)
            if found:
                break
        assert found, "the genome has no exact repeat of %d bases" % k
        _repeat[key] = found
    return _repeat[key]


def tag_requests(seqs):
    """the reads of sam_writer_requests plus the issue's: a three-piece chimera, one with a reverse-strand piece, one across two contigs, a
    read of an exact repeat; pairs with one mate chimeric, one mate unmapped, both unmapped, a mate of mapping quality 0, and the odd
    trailing read"""
    reads, pairs = sam_writer_requests(seqs)
    g, g2, rep = seqs[0][1], seqs[1][1], repeat_read(seqs)
    reads = reads + [g[3000:3060] + g[9000:9060] + g[15000:15060], g[4000:4060] + B.revcomp(g[9500:9570]), g[12000:12060] + g2[5000:5070], rep]
    pairs = pairs[:-1] + [g[20000:20060] + g[30000:30060], B.revcomp(g[20200:20300]), b"ACGT" * 25, B.revcomp(g[40300:40400]), b"ACGT" * 25, b"TTGCA" * 20,
                          rep, g2[5000:5100]] + pairs[-1:]
    assert len(pairs) & 1
    return reads, pairs


def features(recs, contigs):
    """which clauses of the rule the records exercise"""
    f = set()
    for r in recs:
        tags = {t: v for t, _, v in r["tags"]}
        own_h = any(CIG_OPS[c & 15] == "H" for c in r["cig"])
        if "SA" in tags:
            ents = [e.split(",") for e in tags["SA"].split(";")[:-1]]
            assert all(len(e) == 6 for e in ents) and tags["SA"].endswith(";")
            assert not any("H" in e[3] for e in ents), "clips in SA are S"
            f |= {"sa2"} if len(ents) >= 2 else set()
            f |= {"minus"} if any(e[2] == "-" for e in ents) else set()
            f |= {"other_contig"} if any(e[0] != contigs[r["refid"]] for e in ents) else set()
            f |= {"H_lists_S"} if own_h and any("S" in e[3] for e in ents) else set()
        if r["flag"] & 4 and "MC" in tags and "MQ" in tags:
            f.add("unmapped_with_mate_tags")
        if r["flag"] & 8 and "MC" not in tags and "MQ" not in tags:
            f.add("flag8_without")
        if r["flag"] & 0x100:
            assert "SA" not in tags
            f.add("secondary")
        if tags.get("MQ") == 0:
            f.add("mq0")
    return f


# ------------------------------------------------------------------------------------------ the checks
def set_tags(bt, mask):
    return bindt(bt.lib).bwamem_hip_batch_set_tags(bt.b, mask)


def check_tags(lib, h, reads, opts, paired, pes=None, mask=SA | MC | MQ, quals=None, rg=None, masks=False):
    """one batch without and with the tags -> (the tagged stream, its parsed records)"""
    contigs = lib.contig_names(h)
    req = B.pack_request(reads)
    rg_id = RG_ID if rg else None
    bt = Batch(lib, h, opts, req, pes)
    try:
        if quals is not None:
            assert bt.set_quals(quals) == 0
        if rg:
            assert bt.set_rg(rg) == 0
        plain = bt.encode(paired)
        n_dec = len(reads) - (1 if paired and len(reads) & 1 else 0)
        dec = B.decode_response(bt.resp, n_dec)
        raws = split_records(plain)
        assert len(raws) == sum(len(a) for a in dec)
        by_mask = {}
        for m in (range(8) if masks else (mask,)):
            assert set_tags(bt, m) == 0
            by_mask[m] = bt.encode(paired)
            exp = expected_tags(dec, contigs, paired, m)
            assert split_records(by_mask[m]) == [with_tags(raw, t, rg_id) for raw, t in zip(raws, exp)], "mask %d: each bit adds its tag and nothing else" % m
        if masks:
            assert by_mask[0] == plain, "mask 0 is an encode without _set_tags"
            assert set_tags(bt, mask) == 0
            for bad in (8, 0x80000000 | SA, 0xffffffff):
                assert set_tags(bt, bad) != 0, "unknown bits"
                assert bt.encode(paired) == by_mask[mask], "a refused mask leaves the previous one working"
            if not paired:
                assert by_mask[SA | MC | MQ] == by_mask[SA] and by_mask[MC | MQ] == plain, "an unpaired encode ignores MC and MQ"
            ob = ctypes.create_string_buffer(bytes(opts), B.OPT_SIZE)
            pb = ctypes.create_string_buffer(pes, len(pes)) if pes is not None else None
            assert bt.d.bwamem_hip_batch_align(h, ob, pb, bt.b, 0) == 0
            assert bt.encode(paired) == by_mask[mask], "a new alignment keeps the mask"
        tagged = by_mask[mask]
    finally:
        bt.free()
    recs = parse_records(tagged)
    exp = expected_tags(dec, contigs, paired, mask)
    sam = to_sam_tags(lib, h, req, bt.resp, paired, quals, rg_id, mask)
    assert to_sam(recs, contigs) == sam, "a BAM record decodes to the line of bwamem_hip_response_to_sam_tags"
    base = to_sam_q(lib, h, req, bt.resp, paired, None, quals, rg_id).split("\n")[:-1]
    assert sam == "".join(line_with_tags(l, t, rg_id) + "\n" for l, t in zip(base, exp)), "the native writer against the Python formatter"
    for r, want in zip(recs, exp):
        names = [t for t, _, _ in r["tags"]]
        assert names == [t for t in ORDER if t in names], names
        assert [x for x in r["tags"] if x[0] in ("SA", "MC", "MQ")] == want, "values, and MQ in the smallest type"
        if rg:
            assert names[-1] == "RG"
        if paired and mask & MC and mask & MQ:
            assert ("MC" in names) == ("MQ" in names) == bool(r["flag"] & 1 and not r["flag"] & 8), hex(r["flag"])
    return tagged, recs


def check_single_end(lib, h, seqs):
    reads, _ = tag_requests(seqs)
    _, recs = check_tags(lib, h, reads, lib.default_options(), False, masks=True)
    f = features(recs, lib.contig_names(h))
    assert {"sa2", "minus", "other_contig", "H_lists_S"} <= f, f
    assert not any(t in ("MC", "MQ") for r in recs for t, _, _ in r["tags"])


def check_paired(lib, h, seqs):
    _, pairs = tag_requests(seqs)
    po = B.set_opt(lib.default_options(), flag=B.MEM_F_PE)
    for pes in (PES, None):                                          # supplied statistics; inferred ones: the two-phase path
        _, recs = check_tags(lib, h, pairs, po, True, pes=pes, masks=pes is not None)
        f = features(recs, lib.contig_names(h))
        assert {"unmapped_with_mate_tags", "flag8_without", "mq0"} <= f, f
        assert any(r["flag"] & 0x800 for r in recs) and any("SA" in {t for t, _, _ in r["tags"]} for r in recs), "no chimeric mate"
        assert sum(1 for r in recs if r["flag"] & 4 and r["flag"] & 8) >= 2, "no pair with both mates unmapped"
        assert {r["name"] for r in recs} == {b"p%d\0" % i for i in range(len(pairs) >> 1)}, "the odd trailing read has no record"


def check_mem_f_all(lib, h, seqs):
    g, rep = seqs[0][1], repeat_read(seqs)
    reads = [rep, g[3000:3060] + g[9000:9060] + g[15000:15060], rep + g[15000:15060]] + B.simulate_reads(seqs, 6, length=100, seed=13)
    _, recs = check_tags(lib, h, reads, B.set_opt(lib.default_options(), flag=B.MEM_F_ALL), False)
    f = features(recs, lib.contig_names(h))
    assert {"secondary", "sa2"} <= f, f


def long_reads(seqs):
    """reads of 2.1 kb, each three distant segments with indels: SA entries with many CIGAR operations, and a tile of the wavefront form
    (three of them and a plain one: the emulation build takes most of a minute for these)"""
    seg = B.simulate_reads(seqs, 9, length=700, seed=17, sub=0.01, indel=0.01, n_rate=0.0, random_frac=0.0)
    return [seg[3 * i] + seg[3 * i + 1] + seg[3 * i + 2] for i in range(3)] + [seg[0]]


def check_long_reads(lib, h, seqs):
    reads = long_reads(seqs)
    assert max(len(r) for r in reads) > 1000
    _, recs = check_tags(lib, h, reads, lib.default_options(), False)
    sa = [v for r in recs for t, _, v in r["tags"] if t == "SA"]
    assert any(v.count(";") >= 2 for v in sa) and max(sum(e.split(",")[3].count(c) for c in "MIDS") for v in sa for e in v.split(";")[:-1]) >= 8, "no long CIGAR in SA"


def check_tiles(lib, h, seqs, setenv):
    """a batch cut into several tiles: the pairs fall on both sides of every boundary, and the bytes are those of one tile"""
    reads, pairs = tag_requests(seqs)
    po = B.set_opt(lib.default_options(), flag=B.MEM_F_PE)
    one_p, _ = check_tags(lib, h, pairs, po, True, pes=PES)
    one_s, _ = check_tags(lib, h, reads, lib.default_options(), False)
    setenv("BWAMEM_HIP_TILE", "6")
    try:
        cut_p, _ = check_tags(lib, h, pairs, po, True, pes=PES)
        setenv("BWAMEM_HIP_TILE", "5")
        cut_s, _ = check_tags(lib, h, reads, lib.default_options(), False)
    finally:
        setenv("BWAMEM_HIP_TILE", None)
    assert len(pairs) > 3 * 6 and cut_p == one_p and cut_s == one_s


def check_quals_and_rg(lib, h, seqs):
    reads, pairs = tag_requests(seqs)
    check_tags(lib, h, reads, lib.default_options(), False, quals=rand_quals(reads, 5), rg=RG_LINE)
    check_tags(lib, h, pairs, B.set_opt(lib.default_options(), flag=B.MEM_F_PE), True, pes=PES, quals=rand_quals(pairs, 6), rg=RG_LINE)


def one_call(lib, h, opts, pes, t1, t2, tmpdir, tag, **kw):
    d = bindt(lib)
    ob = ctypes.create_string_buffer(bytes(opts), B.OPT_SIZE)
    pb = ctypes.create_string_buffer(pes, len(pes)) if pes is not None else None
    o = BamOptions(size=ctypes.sizeof(BamOptions), **kw)
    path, bpath = os.path.join(tmpdir, tag + ".bam"), os.path.join(tmpdir, tag + ".bai")
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    fb = os.open(bpath, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644) if kw.get("sort") else -1
    counts = DupCounts(*([77] * 6))
    try:
        rc = d.bwamem_hip_fastq_to_bam(h, ob, pb, t1, len(t1), t2, len(t2) if t2 is not None else 0, ctypes.byref(o), fd, fb, ctypes.byref(counts))
    finally:
        os.close(fd)
        if fb >= 0:
            os.close(fb)
    return rc, open(path, "rb").read(), open(bpath, "rb").read() if fb >= 0 else None, counts.as_dict()


def check_chain(lib, h, seqs, tmpdir):
    """tagged records through mark, sort, compress, index and the one-call entry point, against the untagged run of the same call"""
    reads, pairs = tag_requests(seqs)
    reads, pairs = reads + reads[:6], pairs[:-1] + pairs[:4]            # some duplicates to mark
    n_ref = len(seqs)
    po = B.set_opt(lib.default_options(), flag=B.MEM_F_PE)
    for paired, rd, opts, pes in ((False, reads, lib.default_options(), None), (True, pairs, po, PES)):
        rd = [r for r in rd if r]                                    # (FASTQ text of this shape has no empty read)
        names = ["q%d" % (i >> 1 if paired else i) for i in range(len(rd))]
        text = fastq_text(rd, names, rand_quals(rd, 8))
        kw = dict(rg_line=RG_LINE, sort=1, mark_dup=1, write_header=1)
        rc0, raw0, bai0, cnt0 = one_call(lib, h, opts, pes, text, None, tmpdir, "plain", tags=0, **kw)
        rc1, raw1, bai1, cnt1 = one_call(lib, h, opts, pes, text, None, tmpdir, "tagged", tags=SA | MC | MQ, **kw)
        assert rc0 == 0 and rc1 == 0
        assert one_call(lib, h, opts, pes, bgzf_cut(text, 4096), None, tmpdir, "gz", tags=SA | MC | MQ, **kw) == (rc1, raw1, bai1, cnt1), "compressed FASTQ, by 1f 8b"
        d = bindt(lib)
        old = os.path.join(tmpdir, "old.bam"), os.path.join(tmpdir, "old.bai")
        fds = [os.open(p, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644) for p in old]
        c_old = DupCounts()
        try:
            ob = ctypes.create_string_buffer(bytes(opts), B.OPT_SIZE)
            pb = ctypes.create_string_buffer(pes, len(pes)) if pes is not None else None
            assert d.bwamem_hip_align_fastq_to_marked_bam(h, ob, pb, text, len(text), None, 0, RG_LINE, 1, fds[0], fds[1], 1, ctypes.byref(c_old)) == 0
        finally:
            for f in fds:
                os.close(f)
        assert (raw0, bai0, cnt0) == (open(old[0], "rb").read(), open(old[1], "rb").read(), c_old.as_dict()), "tags = 0 is the existing one-call entry"
        hdr = header_rg(lib, h, True, RG_LINE)
        body0, body1 = gzip.decompress(raw0), gzip.decompress(raw1)
        assert body0[:len(hdr)] == hdr and body1[:len(hdr)] == hdr and parse_header(body1)[2] == len(hdr)
        srt0, srt1 = body0[len(hdr):], body1[len(hdr):]
        r0, r1 = split_records(srt0), split_records(srt1)
        keys = [rec_key(r) for r in r1]
        assert keys == sorted(keys), "coordinate-sorted"
        assert [without_tags(r) for r in r1] == r0, "without SA / MC / MQ: the untagged run's records in the same order"
        assert cnt1 == cnt0 and sum(cnt0.values()) > 0
        p0, p1 = parse_records(srt0), parse_records(srt1)
        assert [r["flag"] for r in p1] == [r["flag"] for r in p0] and any(r["flag"] & 0x400 for r in p1), "duplicate flags"
        assert any(t == "SA" for r in p1 for t, _, _ in r["tags"]) and (not paired or any(t == "MC" for r in p1 for t, _, _ in r["tags"]))
        assert all(r["tags"][-1][0] == "RG" for r in p1)
        check_file(raw1, bai1, hdr, srt1, n_ref)
    bad = BamOptions(size=ctypes.sizeof(BamOptions) + 8, tags=SA)
    path = os.path.join(tmpdir, "bad.bam")
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        ob = ctypes.create_string_buffer(bytes(lib.default_options()), B.OPT_SIZE)
        assert bindt(lib).bwamem_hip_fastq_to_bam(h, ob, None, text, len(text), None, 0, ctypes.byref(bad), fd, -1, None) != 0, "an options size the library does not know"
        bad = BamOptions(size=ctypes.sizeof(BamOptions), tags=8)
        assert bindt(lib).bwamem_hip_fastq_to_bam(h, ob, None, text, len(text), None, 0, ctypes.byref(bad), fd, -1, None) != 0, "an unknown tag bit"
    finally:
        os.close(fd)
    assert os.path.getsize(path) == 0
    assert bindt(lib).bwamem_hip_batch_set_tags(None, SA) != 0


def env_setter(monkeypatch):
    return lambda k, v: monkeypatch.delenv(k, raising=False) if v is None else monkeypatch.setenv(k, v)


def run_small_cases(lib, h, seqs, tmpdir, setenv):
    check_single_end(lib, h, seqs)
    check_paired(lib, h, seqs)
    check_mem_f_all(lib, h, seqs)
    check_long_reads(lib, h, seqs)
    check_tiles(lib, h, seqs, setenv)
    check_quals_and_rg(lib, h, seqs)
    check_chain(lib, h, seqs, tmpdir)


# ------------------------------------------------------------------------------------------ CPU suite (emulation build)
@pytest.fixture(scope="module")
def emu_index(small_genome):
    B.build_emu()
    emu = B.product_lib(emu=True)
    seqs, img = small_genome
    h = emu.open_index(img)
    yield emu, h, seqs
    emu.destroy_index(h)


def test_tags_single_end_and_every_mask(emu_index):
    emu, h, seqs = emu_index
    check_single_end(emu, h, seqs)


def test_tags_paired_supplied_and_inferred_statistics(emu_index):
    emu, h, seqs = emu_index
    check_paired(emu, h, seqs)


def test_tags_secondary_records_under_mem_f_all(emu_index):
    emu, h, seqs = emu_index
    check_mem_f_all(emu, h, seqs)


def test_tags_long_read_tile(emu_index):
    emu, h, seqs = emu_index
    check_long_reads(emu, h, seqs)


def test_tags_across_tiles(emu_index, monkeypatch):
    emu, h, seqs = emu_index
    check_tiles(emu, h, seqs, env_setter(monkeypatch))


def test_tags_with_qualities_and_read_group(emu_index):
    emu, h, seqs = emu_index
    check_quals_and_rg(emu, h, seqs)


def test_tags_through_mark_sort_compress_index(emu_index, tmp_path):
    emu, h, seqs = emu_index
    check_chain(emu, h, seqs, str(tmp_path))


def test_tags_python_mirror(emu_index, small_genome, tmp_path):
    """alignSeqsToBam / alignFastqToBam with tags= over the emulation build (the mirror binds whatever LIBBWA_PATH names)"""
    emu, h, seqs = emu_index
    img = small_genome[1]
    reads = [r for r in tag_requests(seqs)[0] if r]
    text = fastq_text(reads, ["r%d" % i for i in range(len(reads))], rand_quals(reads, 4))
    r = subprocess.run([sys.executable, "-c", (
        "import sys; sys.path.insert(0, %r); import bwamem\n"
        "ix = bwamem.BwaMemIndex(%r); al = bwamem.BwaMemAligner(ix)\n"
        "al.alignSeqsToBam(%r, %r, tags=('SA', 'MC', 'MQ'))\n"
        "al.alignFastqToBam(%r, %r, tags=['SA'])\n"
        "try:\n    al.alignSeqsToBam([b'ACGT'], %r, tags=('XX',))\nexcept ValueError:\n    print('tags-checked')\n"
        "al.close(); ix.close()\n") % (B.PKG, img, reads, str(tmp_path / "a.bam"), text, str(tmp_path / "b.bam"), str(tmp_path / "c.bam"))],
        env=dict(os.environ, LIBBWA_PATH=B.EMU_LIB), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "tags-checked" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
    tagged, recs = check_tags(emu, h, reads, emu.default_options(), False, mask=SA)
    raw = gzip.decompress(open(str(tmp_path / "a.bam"), "rb").read())
    assert raw[parse_header(raw)[2]:] == tagged
    raw = gzip.decompress(open(str(tmp_path / "b.bam"), "rb").read())
    got = parse_records(raw[parse_header(raw)[2]:])
    sa = lambda rs: [[x for x in r["tags"] if x[0] == "SA"] for r in rs]
    assert sa(got) == sa(recs) and any(sa(got))


# ------------------------------------------------------------------------------------------ GPU suite
@pytest.mark.gpu
def test_gpu_tags_small_cases(hip_lib, small_genome, tmp_path, monkeypatch):
    seqs, img = small_genome
    h = hip_lib.open_index(img)
    try:
        run_small_cases(hip_lib, h, seqs, str(tmp_path), env_setter(monkeypatch))
    finally:
        hip_lib.destroy_index(h)
