"""Base qualities and read groups in BAM and SAM records (csrc/bam_encode.h: QUAL and the RG section; k_qual_check and the
qualities form of k_bam_emit in csrc/k_post.hip; bwamem_hip_batch_set_qualities / _set_read_group, bwamem_hip_response_to_sam_q,
bwamem_hip_bam_header_rg / bwamem_hip_sam_header_rg).  Nothing has a tolerance.  The same aligned batch is encoded without and with
qualities and a read group: every record with them is the record without them with its QUAL section replaced -- computed here from
the record's own flag and CIGAR -- and RG:Z:<ID> appended; every other byte is identical.  The decoded text equals
bwamem_hip_response_to_sam_q line for line.
CPU suite: the emulation build runs the kernels.  GPU suite (-m gpu): the same on the device."""
import ctypes
import struct

import numpy as np
import pytest

import bwalib as B
from test_bam_sorted import binds, split_records
from test_bam_writer import CIG_OPS, _names_arg, _take, parse_header, parse_records, sam_writer_requests, to_sam

RG_LINE = b"@RG\tID:grp.1\tSM:sample\tPL:ILLUMINA"
RG_ID = b"grp.1"


def bindq(lib):
    d = binds(lib)
    if getattr(d, "_quals_bound", False):
        return d
    vp, sz, i64, cp = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int64, ctypes.c_char_p
    d.bwamem_hip_batch_set_qualities.argtypes = [vp, cp, sz]
    d.bwamem_hip_batch_set_read_group.argtypes = [vp, cp]
    d.bwamem_hip_bam_header_rg.restype = vp; d.bwamem_hip_bam_header_rg.argtypes = [vp, ctypes.c_int, cp, ctypes.POINTER(sz)]
    d.bwamem_hip_sam_header_rg.restype = vp; d.bwamem_hip_sam_header_rg.argtypes = [vp, cp, ctypes.POINTER(sz)]
    d.bwamem_hip_response_to_sam_q.restype = vp
    d.bwamem_hip_response_to_sam_q.argtypes = [vp, cp, cp, sz, vp, ctypes.c_int, cp, cp, ctypes.POINTER(sz)]
    d.bwamem_hip_batch_upload_fastq.restype = vp; d.bwamem_hip_batch_upload_fastq.argtypes = [vp, cp, sz, cp, sz, ctypes.POINTER(i64)]
    d.bwamem_hip_align_fastq_to_bam.argtypes = [vp, vp, vp, cp, sz, cp, sz, cp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    d._quals_bound = True
    return d


def rand_quals(reads, seed):
    """seeded qualities over the whole range 33..126; the first and last byte of the first long read are the two ends of it"""
    rng = np.random.default_rng(seed)
    out = [rng.integers(33, 127, size=len(r), dtype=np.uint8).tobytes() for r in reads]
    k = next(i for i, r in enumerate(reads) if len(r) > 2)
    out[k] = b"!" + out[k][1:-1] + b"~"
    return out


def quals_blob(quals):
    return b"".join(q + b"\0" for q in quals)


def to_sam_q(lib, h, req, resp, paired, names, quals, rg_id):
    d = bindq(lib)
    sz = ctypes.c_size_t()
    arr = (ctypes.c_char_p * len(names))(*[n if isinstance(n, bytes) else n.encode() for n in names]) if names is not None else None
    p = d.bwamem_hip_response_to_sam_q(h, req, resp, len(resp), arr, 1 if paired else 0, quals_blob(quals) if quals is not None else None, rg_id, ctypes.byref(sz))
    assert p, "bwamem_hip_response_to_sam_q returned NULL"
    return _take(lib, p, sz.value).decode()


class Batch:
    """one resident batch, aligned once; encode() gives the records under the qualities / read group set at that moment"""

    def __init__(self, lib, h, opts, req, pes=None, b=None):
        self.lib, self.d, self.h = lib, bindq(lib), h
        d = self.d
        self.b = b if b is not None else d.bwamem_hip_batch_upload(h, req, len(req))
        assert self.b
        assert d.bwamem_hip_batch_keep_offsets(self.b, 1) == 0
        ob = ctypes.create_string_buffer(bytes(opts), B.OPT_SIZE)
        pb = ctypes.create_string_buffer(pes, len(pes)) if pes is not None else None
        assert d.bwamem_hip_batch_align(h, ob, pb, self.b, 0) == 0
        n = d.bwamem_hip_batch_result_bytes(self.b)
        buf = ctypes.create_string_buffer(max(n, 1))
        assert d.bwamem_hip_batch_download(self.b, buf) == 0
        self.resp = buf.raw[:n]

    def set_quals(self, quals):
        blob = quals_blob(quals) if isinstance(quals, list) else quals
        return self.d.bwamem_hip_batch_set_qualities(self.b, blob, len(blob) if blob is not None else 0)

    def set_rg(self, line):
        return self.d.bwamem_hip_batch_set_read_group(self.b, line)

    def download(self):
        m = self.d.bwamem_hip_batch_bam_bytes(self.b)
        buf = ctypes.create_string_buffer(max(m, 1))
        assert self.d.bwamem_hip_batch_bam_download(self.b, buf) == 0
        return buf.raw[:m]

    def encode(self, paired, names=None):
        blob, off = _names_arg(names)
        assert self.d.bwamem_hip_batch_encode_bam(self.b, 1 if paired else 0, blob, off) == 0
        return self.download()

    def free(self):
        self.d.bwamem_hip_batch_free(self.b)


def read_of(rec, paired):
    """the read a record with a default name belongs to"""
    i = int(rec["name"][1:-1])
    return 2 * i + (1 if rec["flag"] & 0x80 else 0) if paired else i


def expected_qual(rec, q):
    """the issue's rule from the record's own flag and CIGAR: reversed if 0x10, cut by the H lengths"""
    if rec["flag"] & 0x10:
        q = q[::-1]
    cig = rec["cig"]
    lead = cig[0] >> 4 if cig and CIG_OPS[cig[0] & 15] == "H" else 0
    trail = cig[-1] >> 4 if len(cig) > 1 and CIG_OPS[cig[-1] & 15] == "H" else 0
    q = q[lead:len(q) - trail]
    assert len(q) == rec["l_seq"]
    return bytes(c - 33 for c in q)


def with_quals(raw, rec, qual_bytes):
    o = 36 + rec["l_rn"] + 4 * len(rec["cig"]) + (rec["l_seq"] + 1) // 2
    assert raw[o:o + rec["l_seq"]] == b"\xff" * rec["l_seq"]
    return raw[:o] + qual_bytes + raw[o + rec["l_seq"]:]


def with_rg(raw, rg_id):
    tag = b"RGZ" + rg_id + b"\0"
    return struct.pack("<i", struct.unpack_from("<i", raw, 0)[0] + len(tag)) + raw[4:] + tag


def quals_requests(seqs):
    """sam_writer_requests plus a read of one base, single-end and paired (the pairs keep their odd trailing read)"""
    reads, pairs = sam_writer_requests(seqs)
    return reads + [b"A"], pairs[:-1] + [b"G", b""] + pairs[-1:]


def check_quals_and_rg(lib, h, reads, opts, paired, pes=None, want_features=True):
    """the issue's 'Qualities' and 'Read group' cases for one request -> the parsed records with qualities"""
    contigs = lib.contig_names(h)
    req = B.pack_request(reads)
    quals = rand_quals(reads, 77)
    bt = Batch(lib, h, opts, req, pes)
    try:
        plain = bt.encode(paired)
        assert bt.set_quals(quals) == 0
        withq = bt.encode(paired)
        assert bt.set_rg(RG_LINE) == 0
        both = bt.encode(paired)
        names = ["nm%d" % (i >> 1 if paired else i) for i in range(len(reads))]
        both_named = bt.encode(paired, names)
        assert bt.set_quals(None) == 0
        only_rg = bt.encode(paired)
        assert bt.set_rg(None) == 0
        assert bt.encode(paired) == plain, "removing qualities and read group must restore the records byte for byte"
    finally:
        bt.free()
    raws, recs = split_records(plain), parse_records(plain)
    assert all(all(x == 0xff for x in r["qual"]) for r in recs)
    want_q = [with_quals(raw, r, expected_qual(r, quals[read_of(r, paired)])) for raw, r in zip(raws, recs)]
    assert split_records(withq) == want_q
    assert split_records(only_rg) == [with_rg(raw, RG_ID) for raw in raws], "RG:Z:<ID> \\0 at the end of every record, nothing else moves"
    assert split_records(both) == [with_rg(raw, RG_ID) for raw in want_q]
    qrecs = parse_records(both)
    for r in qrecs:
        assert r["tags"][-1] == ("RG", "Z", RG_ID.decode())
        assert [t for t, _, _ in r["tags"][:-1]] == [t for t in ("NM", "MD", "AS", "XS", "XA") if t in {x for x, _, _ in r["tags"]}]
    assert to_sam(parse_records(withq), contigs) == to_sam_q(lib, h, req, bt.resp, paired, None, quals, None)
    assert to_sam(qrecs, contigs) == to_sam_q(lib, h, req, bt.resp, paired, None, quals, RG_ID)
    assert to_sam(parse_records(only_rg), contigs) == to_sam_q(lib, h, req, bt.resp, paired, None, None, RG_ID)
    assert to_sam(parse_records(both_named), contigs) == to_sam_q(lib, h, req, bt.resp, paired, names, quals, RG_ID)
    if want_features:
        assert any(r["flag"] & 0x10 and r["l_seq"] > 1 for r in recs) and any(r["flag"] & 4 for r in recs)
        assert paired or any(CIG_OPS[c & 15] == "H" for r in recs for c in r["cig"]), "no hard-clipped record"
        assert {0, 1} <= {r["l_seq"] for r in recs}, "reads of length 0 and 1"
    return qrecs


def check_quality_errors(lib, h, seqs):
    reads = B.simulate_reads(seqs, 5, length=60, seed=9) + [b"", b"AC"]
    req = B.pack_request(reads)
    good = rand_quals(reads, 5)
    bt = Batch(lib, h, lib.default_options(), req)
    try:
        assert bt.set_quals(good) == 0
        ref = bt.encode(False)

        def edited(i, f):
            q = list(good)
            q[i] = f(q[i])
            return q
        two = edited(1, lambda q: q[:-1])
        two[3] += b"5"
        no_nul = bytearray(quals_blob(good))
        no_nul[sum(len(q) + 1 for q in good[:5])] = ord("I")          # where the NUL of the empty read belongs
        bad = {"a byte short": edited(2, lambda q: q[:-1]), "a byte long": edited(2, lambda q: q + b"I"),
               "a byte 32": edited(4, lambda q: q[:7] + b" " + q[8:]), "a byte 127": edited(0, lambda q: q[:-1] + b"\x7f"),
               "one short, one long": two, "a quality where the empty read's NUL belongs": bytes(no_nul)}
        for what, q in bad.items():
            assert bt.set_quals(q) != 0, what
            assert bt.encode(False) == ref, "a refused call must leave the previous qualities: " + what
        assert bt.set_quals(None) == 0
        plain = bt.encode(False)
        assert plain != ref and all(all(x == 0xff for x in r["qual"]) for r in parse_records(plain))
        assert bt.set_quals(bad["a byte 32"]) != 0 and bt.encode(False) == plain
    finally:
        bt.free()
    d = bindq(lib)
    assert d.bwamem_hip_batch_set_qualities(None, b"", 0) != 0 and d.bwamem_hip_batch_set_read_group(None, RG_LINE) != 0


REFUSED_RG = {"no @RG prefix": b"ID:x\tSM:s", "no tab after @RG": b"@RG ID:x", "no ID": b"@RG\tSM:s\tPL:x", "an empty ID": b"@RG\tID:\tSM:s",
              "a 255-byte ID": b"@RG\tID:" + b"i" * 255, "an embedded newline": b"@RG\tID:x\nSM:s", "a carriage return": b"@RG\tID:x\r"}


def header_texts(lib, h, line):
    d = bindq(lib)
    sz = ctypes.c_size_t()
    out = []
    for sorted_ in (0, 1):
        p = d.bwamem_hip_bam_header_rg(h, sorted_, line, ctypes.byref(sz))
        if not p:
            return None
        hdr = _take(lib, p, sz.value)
        text, refs, used = parse_header(hdr)
        assert used == len(hdr)
        out.append((text, refs))
    p = d.bwamem_hip_sam_header_rg(h, line, ctypes.byref(sz))
    if not p:
        return None
    return out + [(_take(lib, p, sz.value).decode(), None)]


def check_read_group_headers(lib, h):
    d = bindq(lib)
    sz = ctypes.c_size_t()
    old = header_texts(lib, h, None)
    assert old[0][0] == _take(lib, d.bwamem_hip_sam_header(h, ctypes.byref(sz)), sz.value).decode() == old[2][0]
    assert old[1][0].split("\n")[0] == "@HD\tVN:1.6\tSO:coordinate"
    for line in (RG_LINE, b"@RG\tID:" + b"i" * 254, b"@RG\tSM:s\tID:z"):
        new = header_texts(lib, h, line)
        for (text, refs), (otext, orefs) in zip(new, old):
            lines, olines = text.split("\n"), otext.split("\n")
            at = max(i for i, l in enumerate(olines) if l.startswith("@SQ")) + 1
            assert lines == olines[:at] + [line.decode()] + olines[at:], "the @RG line once, right after the last @SQ"
            assert refs == orefs
    for what, line in REFUSED_RG.items():
        assert header_texts(lib, h, line) is None, what
    reads = [b"ACGT" * 10]
    bt = Batch(lib, h, lib.default_options(), B.pack_request(reads))
    try:
        assert bt.set_rg(b"@RG\tID:" + b"i" * 254) == 0
        ref = bt.encode(False)
        assert ref.endswith(b"RGZ" + b"i" * 254 + b"\0")
        for what, line in REFUSED_RG.items():
            assert bt.set_rg(line) != 0, what
            assert bt.encode(False) == ref, "a refused line must leave the previous read group"
    finally:
        bt.free()


def run_small_cases(lib, h, seqs):
    reads, pairs = quals_requests(seqs)
    check_quals_and_rg(lib, h, reads, lib.default_options(), False)
    po = B.set_opt(lib.default_options(), flag=B.MEM_F_PE)
    precs = check_quals_and_rg(lib, h, pairs, po, True, pes=B.pack_pestat(150, 450, 300.0, 30.0))
    assert any(r["flag"] & 4 and r["refid"] >= 0 for r in precs), "no unmapped read placed at its mate"
    check_quality_errors(lib, h, seqs)
    check_read_group_headers(lib, h)


# ------------------------------------------------------------------------------------------ CPU suite (emulation build)
@pytest.fixture(scope="module")
def emu_index(small_genome):
    B.build_emu()
    emu = B.product_lib(emu=True)
    seqs, img = small_genome
    h = emu.open_index(img)
    yield emu, h, seqs
    emu.destroy_index(h)


def test_qualities_and_read_group_single_end(emu_index):
    emu, h, seqs = emu_index
    check_quals_and_rg(emu, h, quals_requests(seqs)[0], emu.default_options(), False)


def test_qualities_and_read_group_paired(emu_index):
    emu, h, seqs = emu_index
    po = B.set_opt(emu.default_options(), flag=B.MEM_F_PE)
    recs = check_quals_and_rg(emu, h, quals_requests(seqs)[1], po, True, pes=B.pack_pestat(150, 450, 300.0, 30.0))
    assert any(r["flag"] & 4 and r["refid"] >= 0 for r in recs), "no unmapped read placed at its mate"


def test_quality_errors_leave_the_previous_state(emu_index):
    emu, h, seqs = emu_index
    check_quality_errors(emu, h, seqs)


def test_read_group_headers_and_refused_lines(emu_index):
    emu, h, _ = emu_index
    check_read_group_headers(emu, h)


# ------------------------------------------------------------------------------------------ GPU suite
@pytest.mark.gpu
def test_gpu_quals_small_cases(hip_lib, small_genome):
    seqs, img = small_genome
    h = hip_lib.open_index(img)
    try:
        run_small_cases(hip_lib, h, seqs)
    finally:
        hip_lib.destroy_index(h)
