"""Duplicates marked on the device between the encoder and the coordinate sort (csrc/bam_dup.h, the k_dup_* kernels in
csrc/k_post.hip, the calls bwamem_hip_batch_mark_duplicates, bwamem_hip_mark_duplicates_device, bwamem_hip_align_to_marked_bam,
bwamem_hip_align_fastq_to_marked_bam).  The reference is mark_duplicates_py below: the rule at the top of bam_dup.h restated with
dicts and sorted(), from the record bytes and the read offsets alone.  Every comparison is exact equality of bytes and counts.
Parity with Picard's own output is not checked: there is no JVM and no Picard where this suite runs.
CPU suite: the emulation build runs the kernels.  GPU suite (-m gpu): the same on the device, the medium genome, long reads, and the
device's bytes against the emulation build's."""
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
from test_bam_quals import RG_ID, RG_LINE, Batch, bindq, quals_blob, with_rg
from test_bam_sorted import TILE, build_bai, check_file, headers, python_sorted, sorted_file, split_records, with_offsets
from test_bam_writer import CIG_OPS, _take, batch_bam, parse_records, reg2bin, sam_writer_requests
from test_bgzf_device import batch_bgzf, members
from test_fastq_device import fastq_file, fastq_text, header_rg, upload

COUNT_NAMES = ["unpaired_reads_examined", "read_pairs_examined", "secondary_or_supplementary", "unmapped_reads", "unpaired_read_duplicates",
               "read_pair_duplicates"]
SCORE_CAP = 16383
PES = B.pack_pestat(150, 450, 300.0, 30.0)


class DupCounts(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in COUNT_NAMES]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n in COUNT_NAMES}


# ------------------------------------------------------------------------------------------ bindings
def bindd(lib):
    d = bindq(lib)
    if getattr(d, "_dup_bound", False):
        return d
    vp, sz, cp, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_int
    pc = ctypes.POINTER(DupCounts)
    d.bwamem_hip_batch_mark_duplicates.argtypes = [vp, ci, pc]
    d.bwamem_hip_mark_duplicates_device.argtypes = [vp, vp, sz, ctypes.POINTER(ctypes.c_int64), sz, ci, pc]
    d.bwamem_hip_align_to_marked_bam.argtypes = [vp, vp, vp, cp, sz, vp, ci, ci, ci, ci, pc]
    d.bwamem_hip_align_fastq_to_marked_bam.argtypes = [vp, vp, vp, cp, sz, cp, sz, cp, ci, ci, ci, ci, pc]
    d._dup_bound = True
    return d


def mark_device(lib, h, bam, read_off, paired):
    """bwamem_hip_mark_duplicates_device -> (return code, the bytes handed back, counts)"""
    d = bindd(lib)
    buf = ctypes.create_string_buffer(bytes(bam), max(len(bam), 1))
    off = (ctypes.c_int64 * len(read_off))(*read_off)
    c = DupCounts(*([77] * 6))
    rc = d.bwamem_hip_mark_duplicates_device(h, buf, len(bam), off, len(read_off) - 1, 1 if paired else 0, ctypes.byref(c))
    return rc, buf.raw[:len(bam)], c.as_dict()


# ------------------------------------------------------------------------------------------ the rule in Python (bam_dup.h)
def end_of(r):
    """(refID, u, strand) of a mapped primary record: the unclipped 5' coordinate"""
    ops = [(CIG_OPS[c & 15], c >> 4) for c in r["cig"]]
    lead = 0
    while lead < len(ops) and ops[lead][0] in "SH":
        lead += 1
    trail = len(ops)
    while trail > lead and ops[trail - 1][0] in "SH":
        trail -= 1
    if r["flag"] & 0x10:
        u = r["pos"] + sum(n for o, n in ops if o in "MDN=X") - 1 + sum(n for _, n in ops[trail:])
    else:
        u = r["pos"] - sum(n for _, n in ops[:lead])
    return (r["refid"], u, 1 if r["flag"] & 0x10 else 0)


def mark_duplicates_py(bam, read_off, paired):
    """-> (the marked bytes, the counts, {template: the rules that made it a duplicate}, {template: its number of records})"""
    n_reads = len(read_off) - 1
    step = 2 if paired else 1
    counts = dict.fromkeys(COUNT_NAMES, 0)
    frags, pairs, places = [], [], {}
    for t, r0 in enumerate(range(0, n_reads, step)):
        ends = []
        for r in range(r0, min(r0 + step, n_reads)):
            off = read_off[r]
            for raw in split_records(bam[read_off[r]:read_off[r + 1]]):
                places.setdefault(t, []).append(off)
                off += len(raw)
                rec = parse_records(raw)[0]
                if rec["flag"] & 0x900:
                    counts["secondary_or_supplementary"] += 1
                elif rec["flag"] & 4:
                    counts["unmapped_reads"] += 1
                else:
                    score = min(sum(q for q in rec["qual"] if q >= 15 and q != 0xff), SCORE_CAP)
                    ends.append((end_of(rec), score))
                    frags.append(dict(end=end_of(rec), paired=bool(rec["flag"] & 1) and not rec["flag"] & 8, score=score, t=t))
        if paired and len(ends) == 2:
            pairs.append(dict(key=tuple(sorted(e for e, _ in ends)), score=ends[0][1] + ends[1][1], t=t))
    why = {}
    groups = {}
    for p in pairs:
        groups.setdefault(p["key"], []).append(p)
    for g in groups.values():
        for p in sorted(g, key=lambda p: (-p["score"], p["t"]))[1:]:
            why.setdefault(p["t"], set()).add("pair")
            counts["read_pair_duplicates"] += 1
    groups = {}
    for f in frags:
        groups.setdefault(f["end"], []).append(f)
    for g in groups.values():
        alone = [f for f in g if not f["paired"]]
        if len(alone) < len(g):
            losers, rule = alone, "fragment next to a pair"
        else:
            losers, rule = sorted(alone, key=lambda f: (-f["score"], f["t"]))[1:], "fragment"
        for f in losers:
            why.setdefault(f["t"], set()).add(rule)
            counts["unpaired_read_duplicates"] += 1
    counts["unpaired_reads_examined"] = sum(1 for f in frags if not f["paired"])
    counts["read_pairs_examined"] = len(pairs)
    out = bytearray(bam)
    for t, offs in places.items():
        for o in offs:
            out[o + 19] = (out[o + 19] & ~4) | (4 if t in why else 0)
    return bytes(out), counts, why, {t: len(o) for t, o in places.items()}


def read_offsets(bam, paired):
    """the read offsets of a batch's records, for which no call hands them out: the records of a read are the consecutive ones with
    its name (and, of a pair, its first / second flag); the names of the batches here are unique"""
    off, at, prev = [0], 0, None
    for raw in split_records(bam):
        r = parse_records(raw)[0]
        key = (r["name"], r["flag"] & 0xc0 if paired else 0)
        if prev is not None and key != prev:
            off.append(at)
        prev, at = key, at + len(raw)
    return off + [at] if at else [0, 0]


# ------------------------------------------------------------------------------------------ test 1: hand-made records
def rec(name, flag, refid=-1, pos=-1, cigar="", qual=30, l_seq=None, nrid=-1, npos=-1):
    """one BAM record; qual: a Phred value for every base, or the bytes"""
    cig = [(int(n), CIG_OPS.index(o)) for n, o in re.findall(r"(\d+)([MIDNSHP=X])", cigar)]
    if l_seq is None:
        l_seq = sum(n for n, o in cig if CIG_OPS[o] in "MIS=X")
    q = bytes([qual]) * l_seq if isinstance(qual, int) else qual
    assert len(q) == l_seq
    span = sum(n for n, o in cig if CIG_OPS[o] in "MDN=X")
    nm = name + b"\0"
    body = struct.pack("<iiBBHHHiiii", refid, pos, len(nm), 60 if cig else 0, reg2bin(pos, pos + max(span, 1)) & 0xffff if pos >= 0 else 4680, len(cig), flag, l_seq, nrid, npos, 0)
    body += nm + b"".join(struct.pack("<I", n << 4 | o) for n, o in cig) + b"\x11" * ((l_seq + 1) // 2) + q
    return struct.pack("<i", len(body)) + body


def frag(name, pos, cigar="100M", rev=False, qual=30, refid=0, flag=0):
    return [rec(name, flag | (0x10 if rev else 0), refid, pos, cigar, qual)]


def mates(name, a, b, swap=False):
    """the two reads of a pair, a and b = (refid, pos, cigar, rev, qual) or None for an unmapped read; swap: b is the first of the pair"""
    out = []
    for me, other, bit in ((a, b, 0x80 if swap else 0x40), (b, a, 0x40 if swap else 0x80)):
        flag = 1 | bit | (0x8 if other is None else 0x20 if other[3] else 0)
        if me is None:
            place = other if other is not None else (-1, -1)
            out.append([rec(name, flag | 4, place[0], place[1], "", 30, l_seq=100)])
        else:
            out.append([rec(name, flag | (0x10 if me[3] else 0), me[0], me[1], me[2], me[4])])
    return out[::-1] if swap else out


FWD100, REV399, REV100, FWD399 = (0, 100, "100M", False, 30), (0, 300, "100M", True, 30), (0, 1, "100M", True, 30), (0, 399, "100M", False, 30)


def hand_cases():
    """(name, paired, the reads -- each a list of records --, the expected mark of every read)"""
    q = lambda e, v: e[:4] + (v,)
    c = []
    c.append(("forward, different scores", False, [frag(b"a", 100, qual=30), frag(b"b", 100, qual=35), frag(b"c", 100, qual=20)], [1, 0, 1]))
    c.append(("forward, equal scores", False, [frag(b"a", 100), frag(b"b", 100), frag(b"c", 100)], [0, 1, 1]))
    c.append(("leading S", False, [frag(b"a", 105, "5S95M"), frag(b"b", 100, "100M")], [0, 1]))
    c.append(("leading H, the longer QUAL wins", False, [frag(b"a", 105, "5H95M"), frag(b"b", 100, "100M")], [1, 0]))
    c.append(("leading H and S", False, [frag(b"a", 100, "100M"), frag(b"b", 107, "3H4S93M"), frag(b"c", 106, "3H4S93M")], [0, 1, 0]))
    c.append(("reverse, trailing S", False, [frag(b"a", 100, "100M", True), frag(b"b", 100, "95M5S", True)], [0, 1]))
    c.append(("reverse, trailing H", False, [frag(b"a", 100, "100M", True), frag(b"b", 100, "95M5H", True), frag(b"c", 105, "5S90M3S2H", True)], [0, 1, 1]))
    c.append(("reverse, leading clips do not count", False, [frag(b"a", 100, "100M", True), frag(b"b", 105, "5S95M", True), frag(b"c", 100, "5S95M", True)], [0, 1, 0]))
    c.append(("deletions and introns span, insertions do not", False, [frag(b"a", 100, "50M10D40M10N10M", True), frag(b"b", 100, "60M5I60M", True), frag(b"c", 110, "110M", True)],
              [1, 0, 1]))
    c.append(("same u on opposite strands", False, [frag(b"a", 100, "100M"), frag(b"b", 1, "100M", True)], [0, 0]))
    c.append(("negative u", False, [frag(b"a", 2, "5S95M"), frag(b"b", 0, "3S97M"), frag(b"c", 0, "2S98M")], [0, 1, 0]))
    c.append(("another contig", False, [frag(b"a", 100), frag(b"b", 100, refid=1), frag(b"c", 100, refid=1)], [0, 0, 1]))
    c.append(("FR pairs, the second swapped", True, mates(b"p", FWD100, REV399) + mates(b"q", FWD100, REV399, swap=True), [0, 0, 1, 1]))
    c.append(("FR pairs, the better second pair wins", True, mates(b"p", FWD100, REV399) + mates(b"q", q(FWD100, 31), REV399), [1, 1, 0, 0]))
    c.append(("FR against RF", True, mates(b"p", FWD100, REV399) + mates(b"q", REV100, FWD399), [0, 0, 0, 0]))
    c.append(("both ends at one coordinate", True, mates(b"p", FWD100, REV100) + mates(b"q", REV100, FWD100) + mates(b"r", FWD100, REV100, swap=True), [0, 0, 1, 1, 1, 1]))
    c.append(("mates on different contigs", True, mates(b"p", FWD100, (1, 200, "100M", True, 30)) + mates(b"q", (1, 200, "100M", True, 30), FWD100)
              + mates(b"r", FWD100, (1, 201, "100M", True, 30)), [0, 0, 1, 1, 0, 0]))
    c.append(("a fragment at an end of a pair", True, mates(b"p", q(FWD100, 20), q(REV399, 20)) + mates(b"q", q(FWD100, 40), None) + mates(b"r", None, q(REV399, 40)),
              [0, 0, 1, 1, 1, 1]))
    c.append(("the same fragments without the pair", True, mates(b"q", q(FWD100, 20), None) + mates(b"r", q(FWD100, 40), None) + mates(b"s", None, q(FWD100, 40)),
              [1, 1, 0, 0, 1, 1]))
    sup = rec(b"q", 1 | 8 | 0x40 | 0x800, 0, 5000, "60H40M", 30)
    sec = rec(b"q", 1 | 8 | 0x40 | 0x100, 1, 7000, "100M", 30)
    multi = mates(b"q", q(FWD100, 20), None)
    multi[0] = [sup, multi[0][0], sec]                                  # (the primary is not the first record of its read)
    c.append(("supplementary, secondary and the unmapped mate carry the bit", True, mates(b"p", q(FWD100, 40), None) + multi, [0, 0, 1, 1]))
    c.append(("a supplementary record creates nothing", False, [frag(b"a", 100), frag(b"b", 500) + [rec(b"b", 0x800, 0, 100, "100M", 30)],
                                                               [rec(b"c", 0x100, 0, 100, "100M", 30)] + frag(b"c", 900)], [0, 0, 0]))
    c.append(("unmapped templates", False, [[rec(b"a", 4, l_seq=50)], [rec(b"b", 4, l_seq=50)], [], frag(b"d", 100)], [0, 0, 0, 0]))
    c.append(("unmapped pairs", True, mates(b"p", None, None) + mates(b"q", None, None) + mates(b"r", FWD100, REV399), [0, 0, 0, 0, 0, 0]))
    c.append(("QUAL all 0xff", False, [frag(b"a", 100, qual=0xff), frag(b"b", 100, qual=0xff), frag(b"c", 100, qual=0xff)], [0, 1, 1]))
    c.append(("bytes under 15 count nothing", False, [frag(b"a", 100, qual=14), frag(b"b", 100, qual=b"\x0f" + b"\x0e" * 99), frag(b"c", 100, qual=0)], [1, 0, 1]))
    c.append(("2 000 bases, both capped", False, [frag(b"a", 100, "2000M", qual=40), frag(b"b", 100, "2000M", qual=41)], [0, 1]))
    c.append(("the cap is 16 383", False, [frag(b"a", 100, "400M", qual=40), frag(b"b", 100, "410M", qual=40), frag(b"c", 100, "409M", qual=40), frag(b"d", 100, "420M", qual=40)],
              [1, 0, 1, 1]))
    c.append(("an odd trailing read", True, mates(b"p", FWD100, REV399) + mates(b"q", FWD100, REV399) + [[]], [0, 0, 1, 1, 0]))
    return c


def marks_of(bam, read_off):
    """per read: 1 when every record carries 0x400, 0 when none does (or there is none)"""
    out = []
    for r in range(len(read_off) - 1):
        bits = {bool(x[19] & 4) for x in split_records(bam[read_off[r]:read_off[r + 1]])}
        assert len(bits) <= 1, "the records of one read differ in 0x400"
        out.append(1 if True in bits else 0)
    return out


def layout(reads):
    off = [0]
    for r in reads:
        off.append(off[-1] + sum(len(x) for x in r))
    return b"".join(b"".join(r) for r in reads), off


def only_bit_differs(a, b):
    if len(a) != len(b):
        return False
    x, y, at = bytearray(a), bytearray(b), 0
    for raw in split_records(a):
        x[at + 19] &= ~4 & 0xff
        y[at + 19] &= ~4 & 0xff
        at += len(raw)
    return x == y


def check_hand_cases(lib, h):
    for name, paired, reads, want in hand_cases():
        bam, off = layout(reads)
        py, py_counts, why, _ = mark_duplicates_py(bam, off, paired)
        assert marks_of(py, off) == want, ("the checker", name)
        rc, got, counts = mark_device(lib, h, bam, off, paired)
        assert rc == 0, name
        assert marks_of(got, off) == want, name
        assert got == py and counts == py_counts and only_bit_differs(bam, got), name
        # idempotence: 0x400 pre-set exactly on the keepers comes back cleared, and a second call returns the same bytes
        pre = bytearray(bam)
        at = 0
        for r, reads_r in enumerate(reads):
            for x in reads_r:
                if not want[r]:
                    pre[at + 19] |= 4
                at += len(x)
        rc, got2, counts2 = mark_device(lib, h, bytes(pre), off, paired)
        assert rc == 0 and got2 == got and counts2 == counts, ("pre-set bits", name)
        rc, got3, _ = mark_device(lib, h, got, off, paired)
        assert rc == 0 and got3 == got, ("second call", name)
    # counts written out for one case: a pair, a fragment at its end with its unmapped mate, a fragment elsewhere with a supplementary
    reads = mates(b"p", FWD100, REV399) + mates(b"q", FWD100, None) + mates(b"r", (0, 700, "100M", False, 30), None)
    reads[4].append(rec(b"r", 1 | 8 | 0x40 | 0x800, 0, 5000, "60H40M", 30))
    bam, off = layout(reads)
    rc, got, counts = mark_device(lib, h, bam, off, True)
    assert rc == 0 and marks_of(got, off) == [0, 0, 1, 1, 0, 0]
    assert counts == dict(unpaired_reads_examined=2, read_pairs_examined=1, secondary_or_supplementary=1, unmapped_reads=2, unpaired_read_duplicates=1, read_pair_duplicates=0)
    # refused: records that do not chain, two primaries, a coordinate that does not fit; the bytes come back untouched
    bam, off = layout([frag(b"a", 100), frag(b"b", 100)])
    assert mark_device(lib, h, bam, [0, len(bam) - 8, len(bam)], False)[:2] == (-1, bam)
    assert mark_device(lib, h, bam, [0, len(bam)], False)[:2] == (-1, bam), "two primary records of one read"
    far, off2 = layout([frag(b"a", 0x7fffffff - 5, "100M5S", True), frag(b"b", 100)])
    assert mark_device(lib, h, far, off2, False)[:2] == (-1, far)
    assert mark_device(lib, h, bam, [0, len(bam) + 1], False)[0] != 0 and mark_device(lib, h, b"", [0], False)[0] == 0


# ------------------------------------------------------------------------------------------ test 2: random records
def random_set(n, paired, seed, crowd=0, alone=False):
    """n templates at 2 contigs x P positions x 2 strands with clips of 0..3 at either end; P = n // 6 (40 at 240 templates) grows
    with the set, so that a group holds one to three entries whatever the size (at a fixed P the large sets would be all duplicates).
    crowd: that many templates more at one place; alone: every template at a place of its own."""
    rng = np.random.default_rng(seed)
    n_pos = max(1, n // 6)
    reads = []

    def one(u, rev, refid, qual, flag, name):
        a, z = int(rng.integers(0, 4)), int(rng.integers(0, 4))
        clip = lambda k, o: "%d%s" % (k, o) if k else ""
        so, eo = ("S", "H")[int(rng.integers(0, 2))], ("S", "H")[int(rng.integers(0, 2))]
        m = 30 - a - z
        cigar = clip(a, so) + "%dM" % m + clip(z, eo)
        pos = u - (m - 1 + z) if rev else u + a
        return rec(name, flag | (0x10 if rev else 0), refid, pos, cigar, qual)

    for t in range(n + crowd):
        name = b"t%d" % t
        site = 0 if t >= n else t if alone else int(rng.integers(0, n_pos))
        refid, rev = (site & 1, bool(site >> 1 & 1)) if alone or t >= n else (int(rng.integers(0, 2)), bool(rng.integers(0, 2)))
        u = 200 + (7 * site if alone else site)
        qual = int(rng.choice([10, 20, 30, 0xff]))
        if not paired:
            if rng.random() < 0.1 and t < n:
                reads.append([rec(name, 4, l_seq=30)])
                continue
            recs = [one(u, rev, refid, qual, 0, name)]
            if rng.random() < 0.1:
                recs.insert(int(rng.integers(0, 2)), rec(name, 0x800 | (0x10 if rev else 0), refid, u + 1000, "10H20M", qual))
            reads.append(recs)
            continue
        first_un, second_un = (rng.random() < 0.15, rng.random() < 0.15) if t < n else (False, False)
        swap = 0x80 if rng.random() < 0.5 else 0x40
        mate_u, mate_rev = u + 150 + u % 3, not rev
        f1 = 1 | swap | (8 if second_un else 0x20 if mate_rev else 0)
        f2 = 1 | (swap ^ 0xc0) | (8 if first_un else 0x20 if rev else 0)
        q2 = int(rng.choice([10, 20, 30, 0xff]))
        reads.append([rec(name, f1 | 4, refid if not second_un else -1, u if not second_un else -1, "", qual, l_seq=30)] if first_un else [one(u, rev, refid, qual, f1, name)])
        reads.append([rec(name, f2 | 4, refid if not first_un else -1, u if not first_un else -1, "", q2, l_seq=30)] if second_un else [one(mate_u, mate_rev, refid, q2, f2, name)])
    return reads


RANDOM_SIZES = [0, 1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 17]


def check_random_sets(lib, h, sizes=RANDOM_SIZES):
    sets = [("n=%d" % n, paired, random_set(n, paired, 100 + n + paired), n >= 63) for n in sizes for paired in (False, True)]
    sets += [("crowd", paired, random_set(300, paired, 7, crowd=TILE + 100), False) for paired in (False, True)]
    sets += [("alone", paired, random_set(200, paired, 8, alone=True), False) for paired in (False, True)]
    for name, paired, reads, dense in sets:
        bam, off = layout(reads)
        py, counts, why, _ = mark_duplicates_py(bam, off, paired)
        n_t = len(reads) // 2 if paired else len(reads)
        if dense:
            assert n_t / 4 < len(why) < 3 * n_t / 4, ("the set is not dense", name, paired, len(why), n_t)
        if name == "crowd":
            assert len(why) > TILE, "no group larger than a tile"
        if name == "alone":
            assert not why and counts["unpaired_reads_examined"] + counts["read_pairs_examined"] > 150
        rc, got, got_counts = mark_device(lib, h, bam, off, paired)
        assert rc == 0 and got_counts == counts, (name, paired, got_counts, counts)
        assert got == py, (name, paired)
    return sets


# ------------------------------------------------------------------------------------------ test 3: end to end on the small genome
def seeded_quals(reads, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(33 + 2, 33 + 42, size=len(r), dtype=np.uint8).tobytes() for r in reads]


def planted_single(seqs):
    """single reads from unique places, some repeated 2-4 times under other names; one of them is chimeric (several records)"""
    g = seqs[0][1]
    base = B.simulate_reads(seqs, 10, length=80, seed=31, sub=0.0, indel=0.0, n_rate=0.0, random_frac=0.0)
    base.append(g[3000:3060] + B.revcomp(g[9000:9070]))
    reads = list(base)
    for k, copies in ((0, 1), (3, 3), (5, 2), (10, 2)):
        reads += [base[k]] * copies
    reads += [b"ACGT" * 20, B.revcomp(base[3])]
    names = ["s%d" % i for i in range(len(reads))]
    return reads, names, seeded_quals(reads, 32)


def planted_pairs(seqs):
    """pairs from unique places, some repeated 2-4 times; in some copies one mate is replaced by ACGT repeats"""
    base = B.simulate_pairs(seqs, 8, length=80, seed=33, ins_mean=300, ins_sd=30, sub=0.0, indel=0.0, n_rate=0.0, random_frac=0.0)
    junk = b"ACGT" * 20
    pairs = list(base)
    for k, copies in ((0, 2), (2, 3), (5, 1)):
        pairs += base[2 * k:2 * k + 2] * copies
    pairs += [base[0], junk, junk, base[5], base[4], junk, base[4], junk, base[13], base[12]]
    names = ["f%d" % (i >> 1) for i in range(len(pairs))]
    return pairs, names, seeded_quals(pairs, 34)


def marked_batch(lib, h, opts, paired, pes, req=None, quals=None, t1=None, t2=None):
    """one batch -> (the unmarked records, the marked records, the counts); from a request (with qualities or without) or FASTQ text"""
    d = bindd(lib)
    if req is None:
        b, bad = upload(lib, h, t1, t2)
        assert b, "upload_fastq refused the text (bad_record %d)" % bad
        bt = Batch(lib, h, opts, None, pes, b=b)
    else:
        bt = Batch(lib, h, opts, req, pes)
    try:
        if quals is not None:
            assert bt.set_quals(list(quals)) == 0
        plain = bt.encode(paired)
        c = DupCounts()
        assert d.bwamem_hip_batch_mark_duplicates(bt.b, 1 if paired else 0, ctypes.byref(c)) == 0
        return plain, bt.download(), c.as_dict()
    finally:
        bt.free()


def end_to_end_sets(lib, seqs):
    reads, names, quals = planted_single(seqs)
    pairs, pnames, pquals = planted_pairs(seqs)
    po = B.set_opt(lib.default_options(), flag=B.MEM_F_PE)
    so = lib.default_options()
    return [("single-end", so, False, None, dict(t1=fastq_text(reads, names, quals))),
            ("interleaved", po, True, PES, dict(t1=fastq_text(pairs, pnames, pquals))),
            ("two texts", po, True, PES, dict(t1=fastq_text(pairs[0::2], pnames[0::2], pquals[0::2]), t2=fastq_text(pairs[1::2], pnames[1::2], pquals[1::2]))),
            ("request with qualities", po, True, PES, dict(req=B.pack_request(pairs), quals=pquals)),
            ("request without qualities", so, False, None, dict(req=B.pack_request(reads))),
            ("paired request without qualities", po, True, PES, dict(req=B.pack_request(pairs)))]


def check_end_to_end(lib, h, seqs):
    rules, multi, out = set(), False, []
    for name, opts, paired, pes, src in end_to_end_sets(lib, seqs):
        plain, marked, counts = marked_batch(lib, h, opts, paired, pes, **src)
        off = read_offsets(plain, paired)
        py, py_counts, why, n_recs = mark_duplicates_py(plain, off, paired)
        assert marked == py and counts == py_counts, name
        for t, r in why.items():
            rules |= r
            multi |= n_recs[t] > (2 if paired else 1)
        out.append((plain, marked, counts))
    assert rules == {"pair", "fragment", "fragment next to a pair"} and multi, (rules, multi)
    return out


# ------------------------------------------------------------------------------------------ test 4: the file calls
def marked_file(lib, h, opts, path, bai_path, sort, pes=None, req=None, n_reads=0, t1=None, t2=None, rg=None, write_header=True):
    d = bindd(lib)
    ob = ctypes.create_string_buffer(bytes(opts), B.OPT_SIZE)
    pb = ctypes.create_string_buffer(pes, len(pes)) if pes is not None else None
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    fb = os.open(bai_path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644) if bai_path else -1
    c = DupCounts()
    try:
        if req is not None:
            rc = d.bwamem_hip_align_to_marked_bam(h, ob, pb, req, len(req), None, 1 if sort else 0, fd, fb, 1 if write_header else 0, ctypes.byref(c))
        else:
            rc = d.bwamem_hip_align_fastq_to_marked_bam(h, ob, pb, t1, len(t1), t2, len(t2) if t2 is not None else 0, rg, 1 if sort else 0, fd, fb, 1 if write_header else 0,
                                                        ctypes.byref(c))
        return rc, c.as_dict()
    finally:
        os.close(fd)
        if fb >= 0:
            os.close(fb)


def check_file_calls(lib, h, seqs, tmpdir):
    path, bpath = os.path.join(tmpdir, "m.bam"), os.path.join(tmpdir, "m.bam.bai")
    sets = end_to_end_sets(lib, seqs)
    _, hdr_sorted = headers(lib, h)
    for name, opts, paired, pes, src in (sets[1], sets[0]):             # the FASTQ call: interleaved pairs, single reads
        _, marked, counts = marked_batch(lib, h, opts, paired, pes, **src)
        rc, got = marked_file(lib, h, opts, path, bpath, True, pes, **src)
        assert rc == 0 and got == counts, name
        check_file(open(path, "rb").read(), open(bpath, "rb").read(), hdr_sorted, python_sorted(marked), len(seqs))
        rc, got = marked_file(lib, h, opts, path, None, False, pes, **src)
        assert rc == 0 and got == counts and gzip.decompress(open(path, "rb").read()) == header_rg(lib, h, False, None) + marked, name
        tagged = b"".join(with_rg(r, RG_ID) for r in split_records(marked))
        rc, got = marked_file(lib, h, opts, path, bpath, True, pes, rg=RG_LINE, **src)
        assert rc == 0 and got == counts
        check_file(open(path, "rb").read(), open(bpath, "rb").read(), header_rg(lib, h, True, RG_LINE), python_sorted(tagged), len(seqs))
        assert marked_file(lib, h, opts, path, bpath, False, pes, **src)[0] != 0 and os.path.getsize(path) == 0, "an index needs a sorted file"
    name, opts, paired, pes, src = sets[5]                              # the request call
    _, marked, counts = marked_batch(lib, h, opts, paired, pes, **src)
    assert sum(1 for r in split_records(marked) if r[19] & 4) > 0
    rc, got = marked_file(lib, h, opts, path, bpath, True, pes, req=src["req"])
    assert rc == 0 and got == counts
    check_file(open(path, "rb").read(), open(bpath, "rb").read(), hdr_sorted, python_sorted(marked), len(seqs))
    rc, got = marked_file(lib, h, opts, path, None, False, pes, req=src["req"])
    assert rc == 0 and got == counts and gzip.decompress(open(path, "rb").read()) == header_rg(lib, h, False, None) + marked
    rc, _ = marked_file(lib, h, opts, path, None, True, pes, req=src["req"], write_header=False)
    assert rc == 0 and gzip.decompress(open(path, "rb").read()) == python_sorted(marked)
    assert marked_file(lib, h, opts, path, bpath, False, pes, req=src["req"])[0] != 0 and os.path.getsize(path) == 0 and os.path.getsize(bpath) == 0
    assert marked_file(lib, h, opts, path, bpath, True, pes, req=src["req"], write_header=False)[0] != 0 and os.path.getsize(path) == 0


# ------------------------------------------------------------------------------------------ test 5: errors and state
def check_errors_and_state(lib, h, seqs):
    d = bindd(lib)
    reads, names, quals = planted_single(seqs)
    req = B.pack_request(reads)
    bt = Batch(lib, h, lib.default_options(), req)
    try:
        c = DupCounts(*([5] * 6))
        assert d.bwamem_hip_batch_mark_duplicates(bt.b, 0, ctypes.byref(c)) != 0 and c.as_dict() == dict.fromkeys(COUNT_NAMES, 0), "mark before encode"
        assert bt.set_quals(list(quals)) == 0
        plain = bt.encode(False)
        py, counts, why, _ = mark_duplicates_py(plain, read_offsets(plain, False), False)
        assert why and py != plain
        assert d.bwamem_hip_batch_compress_bam(bt.b, 1) == 0 and d.bwamem_hip_batch_bgzf_bytes(bt.b) > 0
        assert d.bwamem_hip_batch_mark_duplicates(bt.b, 0, None) == 0, "counts may be NULL"
        assert d.bwamem_hip_batch_bgzf_bytes(bt.b) == 0, "marking must discard the members"
        assert bt.download() == py
        assert d.bwamem_hip_batch_mark_duplicates(bt.b, 0, ctypes.byref(c)) == 0 and bt.download() == py and c.as_dict() == counts, "a second call changes nothing"
        assert d.bwamem_hip_batch_compress_bam(bt.b, 1) == 0
        z = ctypes.create_string_buffer(d.bwamem_hip_batch_bgzf_bytes(bt.b))
        assert d.bwamem_hip_batch_bgzf_download(bt.b, z) == 0 and gzip.decompress(z.raw) == py, "the members hold the marked records"
        assert d.bwamem_hip_batch_sort_bam(bt.b) == 0
        srt = bt.download()
        assert srt == python_sorted(py)
        assert d.bwamem_hip_batch_mark_duplicates(bt.b, 0, ctypes.byref(c)) != 0 and bt.download() == srt, "mark after sort: refused, the records as they were"
        assert c.as_dict() == dict.fromkeys(COUNT_NAMES, 0)
        assert bt.encode(False) == plain, "an encode gives unmarked records again"
        assert d.bwamem_hip_batch_mark_duplicates(bt.b, 0, ctypes.byref(c)) == 0 and bt.download() == py
        ob = ctypes.create_string_buffer(bytes(lib.default_options()), B.OPT_SIZE)
        assert d.bwamem_hip_batch_align(h, ob, None, bt.b, 0) == 0
        assert d.bwamem_hip_batch_mark_duplicates(bt.b, 0, None) != 0, "a new alignment must discard the records"
    finally:
        bt.free()
    assert d.bwamem_hip_batch_mark_duplicates(None, 0, None) != 0
    bt = Batch(lib, h, lib.default_options(), B.pack_request([]))
    try:
        assert bt.encode(False) == b""
        c = DupCounts(*([5] * 6))
        assert d.bwamem_hip_batch_mark_duplicates(bt.b, 0, ctypes.byref(c)) == 0 and c.as_dict() == dict.fromkeys(COUNT_NAMES, 0)
        assert d.bwamem_hip_batch_sort_bam(bt.b) == 0
    finally:
        bt.free()


# ------------------------------------------------------------------------------------------ test 6: the calls that existed before
def untouched_bytes(lib, h, seqs, tmpdir):
    reads, _ = sam_writer_requests(seqs)
    req = B.pack_request(reads)
    opts = lib.default_options()
    path, bpath = os.path.join(tmpdir, "u.bam"), os.path.join(tmpdir, "u.bai")
    d = bindq(lib)
    b = d.bwamem_hip_batch_upload(h, req, len(req))
    assert b
    bt = Batch(lib, h, opts, None, b=b)
    try:
        plain = bt.encode(False)
        assert d.bwamem_hip_batch_sort_bam(bt.b) == 0
        srt = bt.download()
    finally:
        bt.free()
    out = [plain, srt, batch_bgzf(lib, h, opts, req, False)]
    assert sorted_file(lib, h, opts, req, len(reads), path, bpath) == 0
    out += [open(path, "rb").read(), open(bpath, "rb").read()]
    r2, n2, q2 = planted_single(seqs)
    assert fastq_file(lib, h, opts, fastq_text(r2, n2, q2), None, RG_LINE, True, path, bpath) == 0
    out += [open(path, "rb").read(), open(bpath, "rb").read()]
    assert fastq_file(lib, h, opts, fastq_text(r2, n2, q2), None, None, False, path, None) == 0
    return out + [open(path, "rb").read()]


# ------------------------------------------------------------------------------------------ CPU suite (emulation build)
@pytest.fixture(scope="module")
def emu_index(small_genome, tmp_path_factory):
    B.build_emu()
    emu = B.product_lib(emu=True)
    seqs, img = small_genome
    h = emu.open_index(img)
    before = untouched_bytes(emu, h, seqs, str(tmp_path_factory.mktemp("before")))     # (test 6: before any marked batch exists in this module)
    yield emu, h, seqs, before
    emu.destroy_index(h)


def test_dup_hand_made_records(emu_index):
    emu, h, _, _ = emu_index
    check_hand_cases(emu, h)


def test_dup_random_records_against_the_checker(emu_index):
    emu, h, _, _ = emu_index
    check_random_sets(emu, h)


def test_dup_end_to_end_planted_duplicates(emu_index):
    emu, h, seqs, _ = emu_index
    check_end_to_end(emu, h, seqs)


def test_dup_file_calls(emu_index, tmp_path):
    emu, h, seqs, _ = emu_index
    check_file_calls(emu, h, seqs, str(tmp_path))


def test_dup_python_mirror(emu_index, small_genome, tmp_path):
    """BwaMemAligner.alignFastqToBam / alignSeqsToBam with mark_duplicates=True over the emulation build, in a child process"""
    emu, h, seqs, _ = emu_index
    _, img = small_genome
    reads, names, quals = planted_single(seqs)
    fq = str(tmp_path / "in.fq")
    with open(fq, "wb") as f:
        f.write(fastq_text(reads, names, quals))
    p = {k: str(tmp_path / k) for k in ("a.bam", "a.bam.bai", "b.bam", "c.bam", "d.bam", "e.bam")}
    r = subprocess.run([sys.executable, "-c", (
        "import sys; sys.path.insert(0, %r); import bwamem\n"
        "ix = bwamem.BwaMemIndex(%r); al = bwamem.BwaMemAligner(ix)\n"
        "reads, quals, p = %r, %r, %r\n"
        "print('A', sorted(al.alignFastqToBam(%r, p['a.bam'], sort=True, index_path=p['a.bam.bai'], mark_duplicates=True).items()))\n"
        "print('B', sorted(al.alignFastqToBam(%r, p['b.bam'], mark_duplicates=True).items()))\n"
        "print('C', sorted(al.alignSeqsToBam(reads, p['c.bam'], sort=True, mark_duplicates=True).items()))\n"
        "print('D', sorted(al.alignSeqsToBam(reads, p['d.bam'], device=True, mark_duplicates=True).items()))\n"
        "print('E', sorted(al.alignSeqsToBam(reads, p['e.bam'], quals=quals, mark_duplicates=True).items()))\n"
        "print('N', al.alignFastqToBam(%r, p['b.bam'] + 'n'), al.alignSeqsToBam(reads, p['b.bam'] + 'n', device=True))\n"
        "try:\n    al.alignSeqsToBam(reads, p['c.bam'] + 'x', mark_duplicates=True)\nexcept ValueError:\n    print('host-framing-refused')\n"
        "al.close(); ix.close()\n") % (B.PKG, img, reads, quals, p, fq, fq, fq)],
        env=dict(os.environ, LIBBWA_PATH=B.EMU_LIB), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "host-framing-refused" in r.stdout and "N None None" in r.stdout, (r.stdout[-1500:], r.stderr[-2000:])
    assert not os.path.exists(p["c.bam"] + "x")
    opts = emu.default_options()
    _, with_q, cq = marked_batch(emu, h, opts, False, None, t1=fastq_text(reads, names, quals))
    _, without_q, cn = marked_batch(emu, h, opts, False, None, req=B.pack_request(reads))
    _, named_q, ce = marked_batch(emu, h, opts, False, None, req=B.pack_request(reads), quals=quals)
    assert cq["unpaired_read_duplicates"] > 0
    lines = dict(ln.split(" ", 1) for ln in r.stdout.splitlines() if ln[:2] in ("A ", "B ", "C ", "D ", "E "))
    assert lines["A"] == lines["B"] == str(sorted(cq.items())) and lines["C"] == lines["D"] == str(sorted(cn.items())) and lines["E"] == str(sorted(ce.items()))
    _, hdr_sorted = headers(emu, h)
    check_file(open(p["a.bam"], "rb").read(), open(p["a.bam.bai"], "rb").read(), hdr_sorted, python_sorted(with_q), len(seqs))
    assert gzip.decompress(open(p["b.bam"], "rb").read()) == header_rg(emu, h, False, None) + with_q
    assert gzip.decompress(open(p["c.bam"], "rb").read()) == hdr_sorted + python_sorted(without_q)
    assert gzip.decompress(open(p["d.bam"], "rb").read()) == header_rg(emu, h, False, None) + without_q
    assert gzip.decompress(open(p["e.bam"], "rb").read()) == header_rg(emu, h, False, None) + named_q


def test_dup_errors_and_state(emu_index):
    emu, h, seqs, _ = emu_index
    check_errors_and_state(emu, h, seqs)


def test_dup_earlier_calls_untouched(emu_index, tmp_path):
    """test 6: after marked batches have existed in the process (where the library has the call at all), the bytes of the calls
    that existed before are what they were"""
    emu, h, seqs, before = emu_index
    if hasattr(emu.dll, "bwamem_hip_batch_mark_duplicates"):
        for name, opts, paired, pes, src in end_to_end_sets(emu, seqs)[:2]:
            marked_batch(emu, h, opts, paired, pes, **src)
    assert untouched_bytes(emu, h, seqs, str(tmp_path)) == before


def test_dup_sanitizers(emu_index, small_genome, tmp_path):
    """the marking calls under AddressSanitizer + UBSan: a stand-alone driver (tests/bam_dup_sanitized_driver.cpp), compiled here
    with the sanitizers and linked against the sanitized emulation build (tests/emu `make asan`), run as a program.  It compares
    what the tooling call hands back with the checker's bytes, written here."""
    B.make(os.path.join(B.ROOT, "tests", "emu"), "asan")
    seqs, img = small_genome
    manifest = []

    def add(tag, bam, off, paired):
        py, counts, _, _ = mark_duplicates_py(bam, off, paired)
        for ext, data in ((".bam", bam), (".off", struct.pack("<%dq" % len(off), *off)), (".want", py)):
            with open(str(tmp_path / (tag + ext)), "wb") as f:
                f.write(data)
        manifest.append("rec %s %d %s" % (tag, 1 if paired else 0, " ".join(str(counts[n]) for n in COUNT_NAMES)))
    for k, (_, paired, reads, _) in enumerate(hand_cases()):
        add("hand%d" % k, *layout(reads), paired)
    for k, (n, paired) in enumerate(((65, False), (65, True), (TILE + 1, True))):
        add("rand%d" % k, *layout(random_set(n, paired, 50 + k)), paired)
    pairs, pnames, pquals = planted_pairs(seqs)
    with open(str(tmp_path / "pairs.fq"), "wb") as f:
        f.write(fastq_text(pairs, pnames, pquals))
    manifest.append("fastq pairs.fq 1 0 0 0 0 0 0")
    with open(str(tmp_path / "manifest.txt"), "w") as f:
        f.write("\n".join(manifest) + "\n")
    emu_dir = os.path.join(B.ROOT, "tests", "emu", "_build")
    exe = str(tmp_path / "bam_dup_sanitized_driver")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(B.ROOT, "include"), os.path.join(B.ROOT, "tests", "bam_dup_sanitized_driver.cpp"), "-o", exe,
                    "-L", emu_dir, "-lbwamem_emu_asan", "-Wl,-rpath," + emu_dir], check=True)
    r = subprocess.run([exe, img, str(tmp_path)], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0"),
                       capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "sanitized-ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


# ------------------------------------------------------------------------------------------ GPU suite
@pytest.mark.gpu
def test_gpu_dup_small_cases(hip_lib, small_genome, tmp_path):
    """test 8: tests 1-5 on the device"""
    seqs, img = small_genome
    h = hip_lib.open_index(img)
    try:
        check_hand_cases(hip_lib, h)
        check_random_sets(hip_lib, h)
        check_end_to_end(hip_lib, h, seqs)
        check_file_calls(hip_lib, h, seqs, str(tmp_path))
        check_errors_and_state(hip_lib, h, seqs)
    finally:
        hip_lib.destroy_index(h)


def repeat_every_tenth(items, step):
    """every tenth read (step 1) or pair (step 2) once more, at the end"""
    return items + [x for k in range(0, len(items) - step + 1, 10 * step) for x in items[k:k + step]]


def check_marked_sorted_indexed(lib, h, seqs, opts, paired, reads, quals):
    """one batch: marked against the checker, then sorted, compressed and indexed -> (the checker's verdicts, the marked records)"""
    d = bindd(lib)
    bt = Batch(lib, h, opts, B.pack_request(reads))
    try:
        if quals is not None:
            assert bt.set_quals(quals) == 0
        plain = bt.encode(paired)
        c = DupCounts()
        assert d.bwamem_hip_batch_mark_duplicates(bt.b, 1 if paired else 0, ctypes.byref(c)) == 0
        marked = bt.download()
        py, counts, why, n_recs = mark_duplicates_py(plain, read_offsets(plain, paired), paired)
        assert c.as_dict() == counts and marked == py
        assert d.bwamem_hip_batch_sort_bam(bt.b) == 0
        srt = bt.download()
        assert srt == python_sorted(marked)
        assert d.bwamem_hip_batch_compress_bam(bt.b, 1) == 0
        z = ctypes.create_string_buffer(d.bwamem_hip_batch_bgzf_bytes(bt.b))
        assert d.bwamem_hip_batch_bgzf_download(bt.b, z) == 0
        sz = ctypes.c_size_t()
        p = d.bwamem_hip_batch_index_bam(bt.b, 0, ctypes.byref(sz))
        assert p
        bai = _take(lib, p, sz.value)
    finally:
        bt.free()
    ms = members(z.raw, True)
    assert b"".join(m[2] for m in ms) == srt
    assert bai == build_bai(with_offsets(srt), [m[0] for m in ms], len(seqs), 0)
    return why, n_recs, counts, marked


@pytest.mark.gpu
def test_gpu_dup_medium_single_and_paired(hip_lib, medium_genome):
    """test 9: the read sets of test_gpu_sorted_medium_single_and_paired with every tenth read or pair repeated once"""
    seqs, img = medium_genome
    h = hip_lib.open_index(img)
    try:
        g = seqs[0][1]
        reads = B.simulate_reads(seqs, 19990, length=150, seed=21, sub=0.02, indel=0.003)
        reads += [g[3000 + 500 * i:3080 + 500 * i] + B.revcomp(g[90000 + 700 * i:90070 + 700 * i]) for i in range(8)] + [b"", b"ACGT" * 30]
        pairs = B.simulate_pairs(seqs, 10000, length=150, seed=22, ins_mean=400, ins_sd=40)
        pairs[10] = b"ACGT" * 37
        po = B.set_opt(hip_lib.default_options(), flag=B.MEM_F_PE)
        for rd, paired, opts, step in ((reads, False, hip_lib.default_options(), 1), (pairs, True, po, 2)):
            rd = repeat_every_tenth(rd, step)
            why, _, counts, marked = check_marked_sorted_indexed(hip_lib, h, seqs, opts, paired, rd, quals_blob(seeded_quals(rd, 23)))
            assert len(split_records(marked)) > 2 * TILE
            assert len(why) >= len(rd) // step // 11 * 0.9, "the repeated reads are not found"
            assert counts["read_pair_duplicates" if paired else "unpaired_read_duplicates"] >= len(rd) // step // 11 * 0.9
    finally:
        hip_lib.destroy_index(h)


@pytest.mark.gpu
def test_gpu_dup_long_reads(hip_lib, medium_genome):
    """test 10: the 200 x 10 kb set of test_gpu_sorted_long_reads with 8 reads repeated: a wavefront per read adds up QUAL, records
    larger than a sort chunk, supplementary records that carry the bit"""
    seqs, img = medium_genome
    h = hip_lib.open_index(img)
    try:
        reads = B.simulate_reads(seqs, 196, length=10000, seed=41, sub=0.05, indel=0.01)
        g = seqs[0][1]
        reads += [g[10000:15000] + B.revcomp(g[200000:205000]), g[30000:34000] + g[300000:306000], b"ACGT" * 2500, B.revcomp(g[50000:60000])]
        repeated = list(range(6)) + [196, 197]
        reads += [reads[k] for k in repeated]
        why, n_recs, counts, marked = check_marked_sorted_indexed(hip_lib, h, seqs, hip_lib.default_options(), False, reads, quals_blob(seeded_quals(reads, 42)))
        # where a repeated read and its copy have the same primary alignment, one of the two is a duplicate (between alignments of
        # equal score the aligner chooses the primary by the read's index, so the two halves of read 196 may swap)
        prim = {int(r["name"][1:-1]): (r["refid"], r["pos"], r["flag"] & 0x10, r["cig"]) for r in parse_records(marked) if not r["flag"] & 0x904}
        same = [(k, 200 + j) for j, k in enumerate(repeated) if k in prim and prim[k] == prim.get(200 + j)]
        assert len(same) >= 6 and counts["unpaired_read_duplicates"] >= len(same) and all(k in why or c in why for k, c in same)
        assert any(n_recs[t] > 1 for t in why), "no duplicate with a supplementary record"
        assert max(len(r) for r in split_records(marked)) > 16384
        assert any(r[19] & 4 and struct.unpack_from("<H", r, 18)[0] & 0x800 for r in split_records(marked))
    finally:
        hip_lib.destroy_index(h)


@pytest.mark.gpu
def test_gpu_dup_equals_emulation(hip_lib, small_genome):
    """test 11: the device's marked bytes and counts are the emulation build's, on the sets of test 3"""
    B.build_emu()
    emu = B.product_lib(emu=True)
    seqs, img = small_genome
    h, he = hip_lib.open_index(img), emu.open_index(img)
    try:
        for name, opts, paired, pes, src in end_to_end_sets(hip_lib, seqs):
            assert marked_batch(hip_lib, h, opts, paired, pes, **src) == marked_batch(emu, he, opts, paired, pes, **src), name
    finally:
        hip_lib.destroy_index(h)
        emu.destroy_index(he)
