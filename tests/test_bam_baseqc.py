"""Base-level QC on the device (csrc/bam_baseqc.h): quality, base, mismatch and indel tables per sequencing cycle and end, the reads'
GC histograms, GC bias over 100-base reference windows, and windows[] of the index.  The checker baseqc_py restates the rule of the
header with loops and dicts over the fixtures' <fasta>.pac and .amb; the CPU suite runs the kernels through the emulation build, the
GPU suite on the device, where the serialized accumulator must equal the emulation build's."""
import collections
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
from test_bam_dup import PES, DupCounts, end_to_end_sets, planted_single, seeded_quals, untouched_bytes
from test_bam_qc import Qc, bindqc, contigs_of, qc_py
from test_bam_quals import Batch, quals_blob
from test_bam_tags import BamOptions
from test_bam_writer import CIG_OPS, _take, reg2bin
from test_fastq_device import fastq_text, upload

CYCLES, LDS_CYCLES, W, GC_BINS = 1024, 256, 100, 101          # BASEQC_CYCLES, BASEQC_LDS_CYCLES (the implementation's LDS window), the window
TABLES = ["base", "qual_sum", "qual_n", "aligned", "mism", "ins", "del_ev", "soft", "read_gc", "gcb_reads", "gcb_qual_sum", "gcb_qual_n"]   # BWAMEM_HIP_BASEQC_*
TABLE_LEN = dict(base=3 * CYCLES * 5, read_gc=3 * GC_BINS, gcb_reads=GC_BINS, gcb_qual_sum=GC_BINS, gcb_qual_n=GC_BINS)
ERR_WALK, ERR_CONTIG, ERR_CIGAR, ERR_RANGE = 1, 2, 4, 8
REPORT_CYCLES, REPORT_GC = 0, 1


class BaseQcCounts(ctypes.Structure):
    _fields_ = [("records", ctypes.c_uint64 * 3), ("qcfail_skipped", ctypes.c_uint64), ("gcb_skipped", ctypes.c_uint64)]


# ------------------------------------------------------------------------------------------ bindings
def bindbq(lib):
    d = bindqc(lib)
    if getattr(d, "_baseqc_bound", False):
        return d
    vp, sz, cp, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_int
    d.bwamem_hip_baseqc_create.restype = vp
    d.bwamem_hip_baseqc_create.argtypes = [vp]
    d.bwamem_hip_baseqc_free.restype = None
    d.bwamem_hip_baseqc_free.argtypes = [vp]
    d.bwamem_hip_baseqc_add_batch.argtypes = [vp, vp]
    d.bwamem_hip_baseqc_add_records_device.argtypes = [vp, cp, sz]
    d.bwamem_hip_baseqc_counts.argtypes = [vp, ctypes.POINTER(BaseQcCounts)]
    d.bwamem_hip_baseqc_array.restype = ctypes.c_int64
    d.bwamem_hip_baseqc_array.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_uint64), sz]
    d.bwamem_hip_baseqc_serialize.restype = vp
    d.bwamem_hip_baseqc_serialize.argtypes = [vp, ctypes.POINTER(sz)]
    d.bwamem_hip_baseqc_add_serialized.argtypes = [vp, cp, sz]
    d.bwamem_hip_baseqc_report.restype = vp
    d.bwamem_hip_baseqc_report.argtypes = [vp, ci, ctypes.POINTER(sz)]
    d.bwamem_hip_index_gc_windows.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    d.bwamem_hip_fastq_to_bam_metrics.argtypes = [vp, vp, vp, cp, sz, cp, sz, ctypes.POINTER(BamOptions), ci, ci, ctypes.POINTER(DupCounts), vp, vp]
    d._baseqc_bound = True
    return d


class BaseQc:
    """one accumulator of `lib` over the index h"""

    def __init__(self, lib, h):
        self.lib, self.d = lib, bindbq(lib)
        self.q = self.d.bwamem_hip_baseqc_create(h)
        assert self.q

    def add_records(self, bam):
        return self.d.bwamem_hip_baseqc_add_records_device(self.q, bytes(bam), len(bam))

    def add_batch(self, b):
        return self.d.bwamem_hip_baseqc_add_batch(self.q, b)

    def state(self):
        c = BaseQcCounts()
        assert self.d.bwamem_hip_baseqc_counts(self.q, ctypes.byref(c)) == 0
        counts = dict(records=tuple(int(x) for x in c.records), qcfail_skipped=int(c.qcfail_skipped), gcb_skipped=int(c.gcb_skipped))
        arrays = {}
        for k, name in enumerate(TABLES):
            n = self.d.bwamem_hip_baseqc_array(self.q, k, None, 0)
            assert n == TABLE_LEN.get(name, 3 * CYCLES), name
            buf = (ctypes.c_uint64 * n)()
            assert self.d.bwamem_hip_baseqc_array(self.q, k, buf, n) == n
            arrays[name] = [int(x) for x in buf]
        assert self.d.bwamem_hip_baseqc_array(self.q, len(TABLES), None, 0) < 0 and self.d.bwamem_hip_baseqc_array(self.q, -1, None, 0) < 0
        return dict(counts=counts, arrays=arrays)

    def serialize(self):
        sz = ctypes.c_size_t()
        p = self.d.bwamem_hip_baseqc_serialize(self.q, ctypes.byref(sz))
        assert p
        return _take(self.lib, p, sz.value)

    def add_serialized(self, blob):
        return self.d.bwamem_hip_baseqc_add_serialized(self.q, blob, len(blob))

    def report(self, kind):
        sz = ctypes.c_size_t()
        p = self.d.bwamem_hip_baseqc_report(self.q, kind, ctypes.byref(sz))
        assert p
        return _take(self.lib, p, sz.value).decode()

    def free(self):
        self.d.bwamem_hip_baseqc_free(self.q)


def gc_windows(lib, h):
    out = (ctypes.c_uint64 * GC_BINS)()
    assert bindbq(lib).bwamem_hip_index_gc_windows(h, out) == 0
    return [int(x) for x in out]


# ------------------------------------------------------------------------------------------ the reference as the index files hold it
Ref = collections.namedtuple("Ref", "contigs offsets codes holes")        # contigs: (name, length); codes: the 2-bit codes of the .pac; holes: (offset, length)


def load_ref(img, seqs):
    """<fasta>.pac and <fasta>.amb of a fixture's index (img = <fasta>.img)"""
    fa = img[:-len(".img")]
    contigs = contigs_of(seqs)
    l_pac = sum(n for _, n in contigs)
    pac = np.fromfile(fa + ".pac", dtype=np.uint8)
    idx = np.arange(l_pac)
    codes = (pac[idx >> 2] >> ((~idx & 3) << 1)) & 3
    with open(fa + ".amb") as f:
        head = f.readline().split()
        assert int(head[0]) == l_pac and int(head[1]) == len(contigs)
        holes = [(int(a), int(b)) for a, b, _ in (ln.split() for ln in f if ln.strip())]
    assert len(holes) == int(head[2]) and holes == sorted(holes)
    offsets, o = [], 0
    for _, n in contigs:
        offsets.append(o)
        o += n
    return Ref(contigs, offsets, codes, holes)


def ref_text(ref, c, p, n):
    """the letters the .pac holds at contig c, [p, p + n)"""
    return bytes(b"ACGT"[int(x)] for x in ref.codes[ref.offsets[c] + p:ref.offsets[c] + p + n])


# ------------------------------------------------------------------------------------------ the rule in Python (the issue's text)
def walk_records(bam):
    """the records of a stream -> (offset, size) each; None where block_size does not chain"""
    out, o = [], 0
    while o < len(bam):
        if len(bam) - o < 36:
            return None
        size = 4 + struct.unpack_from("<i", bam, o)[0]
        if size < 36 or size > len(bam) - o:
            return None
        out.append((o, size))
        o += size
    return out


def baseqc_py(bam, contigs, pac, holes):
    """-> dict(counts=..., arrays=...) of the record stream shaped like BaseQc.state(), or the BASEQC_ERR_* bits of a refused one.
    contigs: (name, length) in index order; pac: the 2-bit code of every base of the packed reference; holes: (offset, length)"""
    offsets, o = [], 0
    for _, n in contigs:
        offsets.append(o)
        o += n
    places = walk_records(bam)
    if places is None:
        return ERR_WALK
    err = 0
    records, qcfail, gcb_skipped = [0, 0, 0], 0, 0
    t = {name: collections.defaultdict(int) for name in TABLES}
    for o, size in places:
        refid, pos, l_name, _, _, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHi", bam, o + 4)
        if l_seq < 0:
            err |= ERR_WALK
            continue
        cig_off = o + 36 + l_name
        seq_off = cig_off + 4 * n_cig
        qual_off = seq_off + (l_seq + 1) // 2
        if qual_off + l_seq > o + size:
            err |= ERR_WALK
            continue
        if refid >= len(contigs):
            err |= ERR_CONTIG
            continue
        if flag & 0x900:
            continue
        cig = [(x & 15, x >> 4) for x in struct.unpack_from("<%dI" % n_cig, bam, cig_off)]
        mapped = not flag & 4
        if mapped:                                                     # every mapped primary is checked, QC-fail or not
            if n_cig == 0 or sum(n for op, n in cig if op in (0, 1, 4, 7, 8)) != l_seq or any(op == 5 and k not in (0, n_cig - 1) for k, (op, n) in enumerate(cig)):
                err |= ERR_CIGAR
                continue
            span = sum(n for op, n in cig if op in (0, 2, 3, 7, 8))
            if refid < 0 or pos < 0 or pos + span > contigs[refid][1]:
                err |= ERR_RANGE
                continue
        if flag & 0x200:
            qcfail += 1
            continue
        e = (1 if flag & 0x40 else 2 if flag & 0x80 else 0) if flag & 1 else 0
        records[e] += 1
        hl = cig[0][1] if cig and cig[0][0] == 5 else 0
        hr = cig[-1][1] if len(cig) > 1 and cig[-1][0] == 5 else 0
        rev = bool(flag & 0x10)

        def bin_of(i):
            c = hr + (l_seq - 1 - i) if rev else hl + i
            return min(max(c, 0), CYCLES - 1)

        def code_of(i):
            nib = bam[seq_off + (i >> 1)] >> (0 if i & 1 else 4) & 15
            return {1: 0, 2: 1, 4: 2, 8: 3}.get(nib, 4)
        has_qual = l_seq > 0 and bam[qual_off] != 0xff
        gc = acgt = 0
        for i in range(l_seq):
            k, c = code_of(i), bin_of(i)
            if k < 4:
                acgt += 1
                gc += k in (1, 2)
            t["base"][(e, c, 3 - k if rev and k < 4 else k)] += 1
            if has_qual:
                t["qual_sum"][(e, c)] += bam[qual_off + i]
                t["qual_n"][(e, c)] += 1
        if acgt:
            t["read_gc"][(e, (200 * gc + acgt) // (2 * acgt))] += 1
        if not mapped:
            continue
        i, p = 0, offsets[refid] + pos
        for op, n in cig:
            if op in (0, 7, 8):
                for j in range(n):
                    t["aligned"][(e, bin_of(i + j))] += 1
                    if code_of(i + j) != int(pac[p + j]):
                        t["mism"][(e, bin_of(i + j))] += 1
                i += n
                p += n
            elif op == 1 or op == 4:
                for j in range(n):
                    t["ins" if op == 1 else "soft"][(e, bin_of(i + j))] += 1
                i += n
            elif op == 2:
                t["del_ev"][(e, bin_of(i - 1))] += 1
                p += n
            elif op == 3:
                p += n
        s = pos + span - W if rev else pos
        g0 = offsets[refid] + s
        if s >= 0 and s + W <= contigs[refid][1] and not any(ho < g0 + W and ho + hn > g0 for ho, hn in holes):
            g = sum(1 for x in pac[g0:g0 + W] if int(x) in (1, 2))
            t["gcb_reads"][g] += 1
            if has_qual:
                t["gcb_qual_sum"][g] += sum(bam[qual_off:qual_off + l_seq])
                t["gcb_qual_n"][g] += l_seq
        else:
            gcb_skipped += 1
    if err:
        return err
    arrays = {}
    for name in TABLES:
        a = [0] * TABLE_LEN.get(name, 3 * CYCLES)
        for key, x in t[name].items():
            if name == "base":
                a[(key[0] * CYCLES + key[1]) * 5 + key[2]] = x
            elif name == "read_gc":
                a[key[0] * GC_BINS + key[1]] = x
            elif name.startswith("gcb"):
                a[key] = x
            else:
                a[key[0] * CYCLES + key[1]] = x
        arrays[name] = a
    return dict(counts=dict(records=tuple(records), qcfail_skipped=qcfail, gcb_skipped=gcb_skipped), arrays=arrays)


def add_states(a, b):
    counts = dict(records=tuple(x + y for x, y in zip(a["counts"]["records"], b["counts"]["records"])),
                  qcfail_skipped=a["counts"]["qcfail_skipped"] + b["counts"]["qcfail_skipped"], gcb_skipped=a["counts"]["gcb_skipped"] + b["counts"]["gcb_skipped"])
    return dict(counts=counts, arrays={n: [x + y for x, y in zip(a["arrays"][n], b["arrays"][n])] for n in TABLES})


def diff_states(got, want):
    if not isinstance(want, dict):
        return "the checker refuses the stream: %r" % (want,)
    out = [(k, got["counts"][k], want["counts"][k]) for k in want["counts"] if got["counts"][k] != want["counts"][k]]
    for n in TABLES:
        out += [(n, i, x, y) for i, (x, y) in enumerate(zip(got["arrays"][n], want["arrays"][n])) if x != y][:6]
    return out[:30]


def nonzero(st, name, e=0):
    """{cycle: count} of one end of an [e][c] table (for base: {(cycle, column): count})"""
    a = st["arrays"][name]
    if name == "base":
        return {(c, k): a[(e * CYCLES + c) * 5 + k] for c in range(CYCLES) for k in range(5) if a[(e * CYCLES + c) * 5 + k]}
    return {c: a[e * CYCLES + c] for c in range(CYCLES) if a[e * CYCLES + c]}


# ------------------------------------------------------------------------------------------ records
def brec(name, flag, refid=-1, pos=-1, cigar="", seq=b"", qual=30, mapq=60, nrid=-1, npos=-1, tlen=0, aux=b""):
    """one BAM record with the SEQ given as letters"""
    cig = [(int(n), CIG_OPS.index(o)) for n, o in re.findall(r"(\d+)([MIDNSHP=X])", cigar)]
    l_seq = len(seq)
    q = bytes([qual]) * l_seq if isinstance(qual, int) else qual
    assert len(q) == l_seq
    span = sum(n for n, o in cig if CIG_OPS[o] in "MDN=X")
    nib = [{65: 1, 67: 2, 71: 4, 84: 8}.get(x, 15) for x in seq] + [0]
    packed = bytes(nib[2 * k] << 4 | nib[2 * k + 1] for k in range((l_seq + 1) // 2))
    nm = name + b"\0"
    body = struct.pack("<iiBBHHHiiii", refid, pos, len(nm), mapq, reg2bin(pos, pos + max(span, 1)) & 0xffff if pos >= 0 else 4680, len(cig), flag, l_seq, nrid, npos, tlen)
    body += nm + b"".join(struct.pack("<I", n << 4 | o) for n, o in cig) + packed + q + aux
    return struct.pack("<i", len(body)) + body


def state_of(lib, h, bam):
    q = BaseQc(lib, h)
    try:
        assert q.add_records(bam) == 0
        return q.state()
    finally:
        q.free()


def clear_stretch(ref, c, n):
    """a position p of contig c with [p - W, p + n + W) inside the contig and free of holes"""
    off, length = ref.offsets[c], ref.contigs[c][1]
    p = W + 50
    while p + n + W <= length:
        hit = [ho + hn for ho, hn in ref.holes if ho < off + p + n + W and ho + hn > off + p - W]
        if not hit:
            return p
        p = max(hit) - off + W + 1
    raise AssertionError("no clear stretch of %d bases on contig %d" % (n, c))


def lone_hole(ref):
    """a hole with W + 20 clear bases of its own contig on either side -> (contig, start, end) in contig coordinates"""
    for ho, hn in ref.holes:
        c = max(k for k, o in enumerate(ref.offsets) if o <= ho)
        s, e = ho - ref.offsets[c], ho + hn - ref.offsets[c]
        others = [(a, b) for a, b in ref.holes if (a, b) != (ho, hn) and a < ho + hn + W + 20 and a + b > ho - W - 20]
        if s >= W + 20 and e + W + 20 <= ref.contigs[c][1] and not others:
            return c, s, e
    raise AssertionError("the genome has no hole with clear flanks")


# ------------------------------------------------------------------------------------------ test 1: hand-made records
def check_hand_records(lib, h, ref):
    """one assertion per line of the rule; every case is also held against the checker"""
    comp = {65: 84, 67: 71, 71: 67, 84: 65}
    col = {65: 0, 67: 1, 71: 2, 84: 3, 78: 4}
    p = clear_stretch(ref, 0, 1100)

    def run(*recs):
        bam = b"".join(recs)
        st = state_of(lib, h, bam)
        want = baseqc_py(bam, ref.contigs, ref.codes, ref.holes)
        assert st == want, diff_states(st, want)
        return st
    r5 = ref_text(ref, 0, p, 5)
    # leading and trailing H, forward: c = Hl + i
    st = run(brec(b"hf", 0, 0, p, "3H5M2H", r5))
    assert nonzero(st, "aligned") == {c: 1 for c in range(3, 8)} and nonzero(st, "mism") == {} and st["counts"]["records"] == (1, 0, 0)
    assert nonzero(st, "base") == {(3 + i, col[x]): 1 for i, x in enumerate(r5)} and nonzero(st, "qual_sum") == {c: 30 for c in range(3, 8)}
    # ... reverse: c = Hr + (l_seq - 1 - i), bases complemented
    st = run(brec(b"hr", 0x10, 0, p, "3H5M2H", r5))
    assert nonzero(st, "aligned") == {c: 1 for c in range(2, 7)} and nonzero(st, "base") == {(2 + 4 - i, col[comp[x]]): 1 for i, x in enumerate(r5)}
    # an unmapped record with 0x10: the flag decides, N stays N, nothing is aligned
    st = run(brec(b"ur", 4 | 0x10, -1, -1, "", b"ACGTN", qual=bytes([10, 11, 12, 13, 14])))
    assert nonzero(st, "base") == {(4, 3): 1, (3, 2): 1, (2, 1): 1, (1, 0): 1, (0, 4): 1} and nonzero(st, "qual_sum") == {4: 10, 3: 11, 2: 12, 1: 13, 0: 14}
    assert nonzero(st, "aligned") == {} and sum(st["arrays"]["gcb_reads"]) == 0 and st["counts"]["gcb_skipped"] == 0
    assert st["arrays"]["read_gc"][50] == 1 and sum(st["arrays"]["read_gc"]) == 1, "2 of 4 called bases are C/G"
    # l_seq 0, 1, 2
    st = run(brec(b"l0", 4), brec(b"l1", 4, seq=b"C"), brec(b"l2", 4, seq=b"AT"))
    assert st["counts"]["records"] == (3, 0, 0) and nonzero(st, "base") == {(0, 1): 1, (0, 0): 1, (1, 3): 1} and nonzero(st, "qual_n") == {0: 2, 1: 1}
    assert st["arrays"]["read_gc"][100] == 1 and st["arrays"]["read_gc"][0] == 1 and sum(st["arrays"]["read_gc"]) == 2
    st = run(brec(b"nn", 4, seq=b"NNN"))
    assert sum(st["arrays"]["read_gc"]) == 0 and nonzero(st, "base") == {(0, 4): 1, (1, 4): 1, (2, 4): 1}, "no called base: no read_gc"
    # QUAL 0xff
    st = run(brec(b"nq", 0, 0, p, "5M", r5, qual=0xff))
    assert nonzero(st, "qual_n") == {} and nonzero(st, "qual_sum") == {} and len(nonzero(st, "base")) == 5 and sum(st["arrays"]["gcb_reads"]) == 1
    assert sum(st["arrays"]["gcb_qual_n"]) == 0
    # a read N on a match column is a mismatch; any other difference too
    other = bytes([comp[r5[4]]])
    st = run(brec(b"rn", 0, 0, p, "5M", r5[:2] + b"N" + r5[3:4] + other))
    assert nonzero(st, "mism") == {2: 1, 4: 1} and nonzero(st, "aligned") == {c: 1 for c in range(5)}
    # I at the first aligned base, D after it: the deletion counts once, at the cycle of the base before it
    r9 = ref_text(ref, 0, p, 3) + ref_text(ref, 0, p + 5, 4)
    st = run(brec(b"id", 0, 0, p, "2I3M2D4M", b"GG" + r9))
    assert nonzero(st, "ins") == {0: 1, 1: 1} and nonzero(st, "del_ev") == {4: 1} and nonzero(st, "aligned") == {c: 1 for c in range(2, 9)} and nonzero(st, "mism") == {}
    st = run(brec(b"idr", 0x10, 0, p, "2I3M2D4M", b"GG" + r9))
    assert nonzero(st, "ins") == {8: 1, 7: 1} and nonzero(st, "del_ev") == {4: 1} and nonzero(st, "mism") == {}
    st = run(brec(b"d0", 0, 0, p, "2D5M", ref_text(ref, 0, p + 2, 5)), brec(b"sc", 0, 0, p, "2S3M1S", b"TT" + ref_text(ref, 0, p, 3) + b"A"))
    assert nonzero(st, "del_ev") == {0: 1} and nonzero(st, "soft") == {0: 1, 1: 1, 5: 1} and nonzero(st, "mism") == {}, "a D before the first read base: cycle 0"
    # 0x200
    st = run(brec(b"qf", 0x200, 0, p, "5M", r5))
    assert st["counts"] == dict(records=(0, 0, 0), qcfail_skipped=1, gcb_skipped=0) and all(sum(st["arrays"][n]) == 0 for n in TABLES)
    # secondary and supplementary records contribute nothing at all
    st = run(brec(b"se", 0x100, 0, p, "5M", r5), brec(b"su", 0x800, 0, p, "5M", r5))
    assert st["counts"] == dict(records=(0, 0, 0), qcfail_skipped=0, gcb_skipped=0) and all(sum(st["arrays"][n]) == 0 for n in TABLES)
    # each of the three ends
    st = run(brec(b"e1", 1 | 0x40, 0, p, "5M", r5), brec(b"e1b", 1 | 0x40 | 0x80, 0, p, "5M", r5), brec(b"e2", 1 | 0x80, 0, p, "5M", r5),
             brec(b"e0a", 1, 0, p, "5M", r5), brec(b"e0b", 0x40, 0, p, "5M", r5), brec(b"e0c", 0x80, 0, p, "5M", r5))
    assert st["counts"]["records"] == (3, 2, 1) and nonzero(st, "aligned", 1) == {c: 2 for c in range(5)} and nonzero(st, "aligned", 2) == {c: 1 for c in range(5)}
    # the window at s = 0 and at s + W = length, valid; one base outside, skipped
    cl, length = next((c, n) for c, (_, n) in enumerate(ref.contigs) if n >= 3 * W and not any(ho < ref.offsets[c] + W or ho + hn > ref.offsets[c] + n - W
                      for ho, hn in ref.holes if ref.offsets[c] <= ho < ref.offsets[c] + n))
    gc_of = lambda c, s: sum(1 for x in ref.codes[ref.offsets[c] + s:ref.offsets[c] + s + W] if int(x) in (1, 2))
    st = run(brec(b"w0", 0, cl, 0, "20M", ref_text(ref, cl, 0, 20), qual=7))
    assert st["counts"]["gcb_skipped"] == 0 and st["arrays"]["gcb_reads"][gc_of(cl, 0)] == 1 and st["arrays"]["gcb_qual_sum"][gc_of(cl, 0)] == 140
    assert st["arrays"]["gcb_qual_n"][gc_of(cl, 0)] == 20
    st = run(brec(b"wl", 0x10, cl, length - 20, "20M", ref_text(ref, cl, length - 20, 20)))
    assert st["counts"]["gcb_skipped"] == 0 and st["arrays"]["gcb_reads"][gc_of(cl, length - W)] == 1
    st = run(brec(b"wr0", 0x10, cl, W - 20, "20M", ref_text(ref, cl, W - 20, 20)))
    assert st["counts"]["gcb_skipped"] == 0 and st["arrays"]["gcb_reads"][gc_of(cl, 0)] == 1, "a reverse record whose window starts at 0"
    st = run(brec(b"o1", 0x10, cl, W - 21, "20M", ref_text(ref, cl, W - 21, 20)), brec(b"o2", 0, cl, length - W + 1, "20M", ref_text(ref, cl, length - W + 1, 20)))
    assert st["counts"]["gcb_skipped"] == 2 and sum(st["arrays"]["gcb_reads"]) == 0
    # windows against a hole: overlapping it by exactly one base on either side, and ending / starting right at it
    ch, hs, he = lone_hole(ref)
    touching = [brec(b"t1", 0, ch, hs - W + 1, "20M", ref_text(ref, ch, hs - W + 1, 20)), brec(b"t2", 0, ch, he - 1, "20M", ref_text(ref, ch, he - 1, 20))]
    st = run(*touching)
    assert st["counts"]["gcb_skipped"] == 2 and sum(st["arrays"]["gcb_reads"]) == 0
    st = run(brec(b"b1", 0, ch, hs - W, "20M", ref_text(ref, ch, hs - W, 20)), brec(b"b2", 0, ch, he, "20M", ref_text(ref, ch, he, 20)))
    assert st["counts"]["gcb_skipped"] == 0 and sum(st["arrays"]["gcb_reads"]) == 2
    # 1 030 bases: the last bin stands for every cycle from 1 023 on
    for flag in (0, 0x10):
        st = run(brec(b"long", flag, 0, p, "1030M", ref_text(ref, 0, p, 1030), qual=2))
        want = {c: 1 for c in range(CYCLES - 1)}
        want[CYCLES - 1] = 7
        assert nonzero(st, "aligned") == want and nonzero(st, "qual_n") == want and nonzero(st, "qual_sum")[CYCLES - 1] == 14 and nonzero(st, "mism") == {}


# ------------------------------------------------------------------------------------------ test 2: random records
RANDOM_SIZES = [1, 31, 32, 33, 257, 3000]
READ_LENGTHS = list(range(1, 10)) + [63, 64, 65, 255, 256, 257, 1000, 1001, 1023, 1024]      # 255 .. 257: around the LDS window of 256 cycles
FLAGS = [0, 0x10, 1 | 0x40, 1 | 0x40 | 0x10, 1 | 0x80, 1 | 0x80 | 0x10, 1 | 0x40 | 0x20, 0x400, 1 | 2 | 0x80 | 0x20]


def random_records(n, seed, ref, lengths=READ_LENGTHS, short=True):
    """n records with CIGARs that cover l_seq, placed inside their contigs; short: beyond one record of every length, mostly short ones"""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    out = []
    for k in range(n):
        if k < len(lengths) and n >= len(lengths):
            l_seq = lengths[k]
        elif short and rng.random() < 0.9:
            l_seq = int(rng.choice([x for x in lengths if x <= 65]))
        else:
            l_seq = int(rng.choice(lengths))
        flag = FLAGS[int(rng.integers(0, len(FLAGS)))]
        u = rng.random()
        flag |= 0x100 if u < 0.04 else 0x800 if u < 0.08 else 0x200 if u < 0.1 else 0
        qual = 0xff if rng.random() < 0.1 else rng.integers(0, 94 if rng.random() < 0.9 else 256, size=l_seq, dtype=np.uint8).tobytes()
        if isinstance(qual, bytes) and qual[:1] == b"\xff":
            qual = b"\x28" + qual[1:]
        if rng.random() < 0.12:                                        # unmapped, placed or not
            seq = bytes(rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), size=l_seq))
            refid = int(rng.integers(-1, len(ref.contigs)))
            out.append(brec(b"u%d" % k, flag | 4, refid, int(rng.integers(0, 50)) if refid >= 0 else -1, "", seq, qual))
            continue
        # a CIGAR that covers l_seq: clips, then blocks of M / = / X with I, D and N between them
        ops, left = [], l_seq
        hl, hr = (int(rng.integers(1, 40)) if rng.random() < 0.15 else 0 for _ in range(2))
        sl = int(rng.integers(0, min(left, 6))) if rng.random() < 0.3 else 0
        left -= sl
        sr = int(rng.integers(0, min(left, 6))) if left > 1 and rng.random() < 0.3 else 0
        left -= sr
        while left > 0:
            m = left if left < 3 or rng.random() < 0.4 else int(rng.integers(1, left))
            ops.append((m, "M=X"[int(rng.choice(3, p=[0.8, 0.1, 0.1]))]))
            left -= m
            if left > 0:
                v = rng.random()
                if v < 0.4:
                    i = int(rng.integers(1, min(left, 4) + 1))
                    ops.append((i, "I"))
                    left -= i
                elif v < 0.8:
                    ops.append((int(rng.integers(1, 6)), "D"))
                else:
                    ops.append((int(rng.integers(1, 40)), "N"))
        if ops and ops[-1][1] in "DN" and rng.random() < 0.7:
            ops.pop()
        if not ops or rng.random() < 0.05:
            ops.insert(0, (int(rng.integers(1, 4)), "D"))              # a deletion in front of the first read base
        span = sum(x for x, o in ops if o in "MDN=X")
        refid = int(rng.integers(0, len(ref.contigs)))
        length = ref.contigs[refid][1]
        if span > length:
            refid = max(range(len(ref.contigs)), key=lambda c: ref.contigs[c][1])
            length = ref.contigs[refid][1]
        v = rng.random()
        pos = 0 if v < 0.05 else length - span if v < 0.1 else int(rng.integers(0, length - span + 1))
        seq, pp = bytearray(rng.choice(letters, size=sl).tobytes()), pos
        for x, o in ops:
            if o in "M=X":
                seq += ref_text(ref, refid, pp, x)
            elif o == "I":
                seq += rng.choice(letters, size=x).tobytes()
            if o in "MDN=X":
                pp += x
        seq += rng.choice(letters, size=sr).tobytes()
        for i in np.flatnonzero(rng.random(len(seq)) < 0.03):
            seq[int(i)] = b"ACGTN"[int(rng.integers(0, 5))]
        cigar = ("%dH" % hl if hl else "") + ("%dS" % sl if sl else "") + "".join("%d%s" % op for op in ops) + ("%dS" % sr if sr else "") + ("%dH" % hr if hr else "")
        out.append(brec(b"r%d" % k, flag, refid, pos, cigar, bytes(seq), qual))
    return out


def check_random_sets(lib, h, ref, sizes=RANDOM_SIZES, seed0=500):
    sets = []
    for n in sizes:
        recs = random_records(n, seed0 + n, ref)
        bam = b"".join(recs)
        want = baseqc_py(bam, ref.contigs, ref.codes, ref.holes)
        assert isinstance(want, dict), (n, want)
        whole, halves, shuffled = BaseQc(lib, h), BaseQc(lib, h), BaseQc(lib, h)
        try:
            assert whole.add_records(bam) == 0
            got = whole.state()
            assert got == want, (n, diff_states(got, want))
            assert halves.add_records(b"".join(recs[:n // 2])) == 0 and halves.add_records(b"".join(recs[n // 2:])) == 0
            assert halves.state() == want and halves.serialize() == whole.serialize(), (n, "two halves")
            order = np.random.default_rng(n).permutation(n)
            assert shuffled.add_records(b"".join(recs[i] for i in order)) == 0 and shuffled.serialize() == whole.serialize(), (n, "shuffled")
        finally:
            whole.free(), halves.free(), shuffled.free()
        sets.append((bam, want))
    if max(sizes) >= 3000:
        big = sets[-1][1]
        assert all(sum(big["arrays"][t]) > 0 for t in TABLES) and all(big["counts"][k] > 0 for k in ("qcfail_skipped", "gcb_skipped")) and min(big["counts"]["records"]) > 0
        for t, width in (("base", 1), ("aligned", 1), ("qual_sum", 1), ("mism", 16)):
            a = big["arrays"][t]
            per = 5 if t == "base" else 1
            at = lambda lo, hi: sum(a[(e * CYCLES + lo) * per:(e * CYCLES + hi) * per] != [0] * ((hi - lo) * per) for e in range(3))
            assert at(LDS_CYCLES - width, LDS_CYCLES) and at(LDS_CYCLES, LDS_CYCLES + width) and at(CYCLES - 1 - width, CYCLES - 1) and at(CYCLES - 1, CYCLES), \
                (t, "both sides of the LDS window, and the last two bins")
    return sets


# ------------------------------------------------------------------------------------------ test 3: windows[]
def windows_np(ref):
    l_pac = len(ref.codes)
    out = np.zeros(GC_BINS, dtype=np.int64)
    if l_pac < W:
        return [0] * GC_BINS
    is_gc = np.concatenate(([0], np.cumsum((ref.codes == 1) | (ref.codes == 2))))
    hole = np.zeros(l_pac + 1, dtype=np.int64)
    for ho, hn in ref.holes:
        hole[ho:ho + hn] = 1
    in_hole = np.concatenate(([0], np.cumsum(hole[:l_pac])))
    for off, (_, n) in zip(ref.offsets, ref.contigs):
        if n < W:
            continue
        s = off + np.arange(n - W + 1)
        ok = in_hole[s + W] - in_hole[s] == 0
        out += np.bincount((is_gc[s + W] - is_gc[s])[ok], minlength=GC_BINS)
    return [int(x) for x in out]


def check_windows(lib, h, ref):
    got, want = gc_windows(lib, h), windows_np(ref)
    assert got == want, [(g, a, b) for g, (a, b) in enumerate(zip(got, want)) if a != b][:10]
    assert gc_windows(lib, h) == want, "asked for again"
    return want


def tiny_genome(lib, workdir):
    """contigs of 5 000 (with N runs at both ends and inside), 60, 100, 101 and 99 bases: shorter than, exactly and just above one window"""
    rng = np.random.default_rng(77)
    big = bytearray(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=5000).tobytes())
    for a, b in ((0, 3), (700, 701), (1500, 1620), (4990, 5000)):
        big[a:b] = b"N" * (b - a)
    seqs = [("t_big", bytes(big))] + [("t_%d" % n, rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n).tobytes()) for n in (60, 100, 101, 99)]
    fa = os.path.join(workdir, "tiny.fa")
    B.write_fasta(fa, seqs)
    build = lib.dll.jnibwa_createReferenceIndex
    build.argtypes = [ctypes.c_char_p] * 3
    assert build(fa.encode(), fa.encode(), b"auto") == 0
    assert lib.create_index_file(fa, fa + ".img") == 0
    return seqs, fa + ".img"


# ------------------------------------------------------------------------------------------ test 4: end to end
def bam_file_records(data):
    """the record stream of a BAM file"""
    raw = gzip.decompress(data)
    assert raw[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<i", raw, 4)
    p = 8 + l_text
    n_ref, = struct.unpack_from("<i", raw, p)
    p += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", raw, p)
        p += 4 + l_name + 4
    return raw[p:]


def one_call_metrics(lib, h, opts, pes, t1, t2, tmpdir, tag, qc, bq, closed_fd=False, **kw):
    """bwamem_hip_fastq_to_bam_metrics (qc: a Qc or None; bq: a BaseQc or None) -> (return code, the BAM bytes)"""
    d = bindbq(lib)
    ob = ctypes.create_string_buffer(bytes(opts), B.OPT_SIZE)
    pb = ctypes.create_string_buffer(pes, len(pes)) if pes is not None else None
    o = BamOptions(size=ctypes.sizeof(BamOptions), **kw)
    path = os.path.join(tmpdir, tag + ".bam")
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    if closed_fd:
        os.close(fd)
    try:
        rc = d.bwamem_hip_fastq_to_bam_metrics(h, ob, pb, t1, len(t1), t2, len(t2) if t2 is not None else 0, ctypes.byref(o), fd, -1, None,
                                               qc.q if qc is not None else None, bq.q if bq is not None else None)
    finally:
        if not closed_fd:
            os.close(fd)
    return rc, open(path, "rb").read()


def check_end_to_end(lib, h, seqs, ref, tmpdir):
    d = bindbq(lib)
    for name, opts, paired, pes, src in end_to_end_sets(lib, seqs)[:2]:        # single-end, interleaved pairs
        t1 = src["t1"]
        blobs = []
        for mark, sort in ((0, 0), (1, 1)):
            qc, bq, alone = Qc(lib, h), BaseQc(lib, h), BaseQc(lib, h)
            try:
                tag = "%s-%d%d" % (name, mark, sort)
                rc, bam = one_call_metrics(lib, h, opts, pes, t1, None, tmpdir, tag, qc, bq, sort=sort, mark_dup=mark, write_header=1)
                assert rc == 0
                recs = bam_file_records(bam)
                want = baseqc_py(recs, ref.contigs, ref.codes, ref.holes)
                got = bq.state()
                assert got == want, (tag, diff_states(got, want))
                assert qc.state() == qc_py(recs, len(ref.contigs)), "the record-level QC of the same call"
                rc0, bam0 = one_call_metrics(lib, h, opts, pes, t1, None, tmpdir, tag + "x", None, alone, sort=sort, mark_dup=mark, write_header=1)
                assert rc0 == 0 and bam0 == bam and alone.serialize() == bq.serialize(), "qc may be NULL; the file does not change"
                rc1, bam1 = one_call_metrics(lib, h, opts, pes, t1, None, tmpdir, tag + "y", None, None, sort=sort, mark_dup=mark, write_header=1)
                assert rc1 == 0 and bam1 == bam
                blobs.append(bq.serialize())
                # the two accumulators of one call against each other
                c, a = qc.state()["counts"], got["arrays"]
                assert c["records_without_nm"] == 0 and sum(a["mism"]) + c["ins_bases"] + c["del_bases"] == c["mismatches"]
                assert sum(a["aligned"]) + sum(a["ins"]) == c["bases_mapped_cigar"] and sum(a["soft"]) == c["bases_soft_clipped"] and sum(a["del_ev"]) == c["del_events"]
                assert sum(got["counts"]["records"]) == c["sequences"] and sum(a["qual_n"]) == c["total_length"] == sum(a["base"])
                assert sum(a["gcb_reads"]) + got["counts"]["gcb_skipped"] == sum(c["primary_mapped"]) > 0
                assert (got["counts"]["records"][1] > 0 and got["counts"]["records"][2] > 0) == paired
                check_reports(lib, h, bq, got, ref)
            finally:
                qc.free(), bq.free(), alone.free()
        assert blobs[0] == blobs[1], "marking and sorting do not change the block"
        # the stages of a batch: after encode, after mark, after sort
        b, bad = upload(lib, h, t1, None)
        assert b, bad
        bt = Batch(lib, h, opts, None, pes, b=b)
        qs = [BaseQc(lib, h) for _ in range(3)]
        try:
            plain = bt.encode(paired)
            assert qs[0].add_batch(bt.b) == 0 and qs[0].state() == baseqc_py(plain, ref.contigs, ref.codes, ref.holes)
            assert d.bwamem_hip_batch_mark_duplicates(bt.b, 1 if paired else 0, None) == 0 and qs[1].add_batch(bt.b) == 0
            assert d.bwamem_hip_batch_sort_bam(bt.b) == 0 and bt.download() != plain and qs[2].add_batch(bt.b) == 0
            assert qs[0].serialize() == qs[1].serialize() == qs[2].serialize() == blobs[0], "grouped by read and one record per item give the same block"
        finally:
            bt.free()
            for q in qs:
                q.free()


# ------------------------------------------------------------------------------------------ test 7: the reports
def reports_py(st, windows):
    """-> (CYCLES, GC) as csrc/sam_writer.cpp documents them"""
    ratio = lambda a, b: float(a) / float(b) if b else 0.0
    a = st["arrays"]
    o = ""
    for e in range(3):
        if not st["counts"]["records"][e]:
            continue
        o += "# end %d records %d\n" % (e, st["counts"]["records"][e])
        o += "cycle\tbases\tmean_quality\tA\tC\tG\tT\tN\taligned\tmismatch_rate\tinsertions\tdeletions\tsoft_clips\n"
        rows = [c for c in range(CYCLES) if any(a[t][e * CYCLES + c] for t in TABLES[1:8]) or any(a["base"][(e * CYCLES + c) * 5:(e * CYCLES + c) * 5 + 5])]
        for c in range(rows[-1] + 1 if rows else 0):
            w = e * CYCLES + c
            b = a["base"][w * 5:w * 5 + 5]
            o += "%d\t%d\t%.4f" % (c, sum(b), ratio(a["qual_sum"][w], a["qual_n"][w])) + "".join("\t%.6f" % ratio(x, sum(b)) for x in b)
            o += "\t%d\t%.6f\t%d\t%d\t%d\n" % (a["aligned"][w], ratio(a["mism"][w], a["aligned"][w]), a["ins"][w], a["del_ev"][w], a["soft"][w])
    g = "# gcb_skipped %d\ngc\twindows\treads\tnormalized_coverage\tmean_base_quality\n" % st["counts"]["gcb_skipped"]
    n_win, n_rd = sum(windows), sum(a["gcb_reads"])
    for k in range(GC_BINS):
        g += "%d\t%d\t%d\t%.6f\t%.4f\n" % (k, windows[k], a["gcb_reads"][k], ratio(a["gcb_reads"][k] * n_win, n_rd * windows[k]), ratio(a["gcb_qual_sum"][k], a["gcb_qual_n"][k]))
    g += "\ngc_percent\tend0\tend1\tend2\n"
    for k in range(GC_BINS):
        g += "%d\t%d\t%d\t%d\n" % (k, a["read_gc"][k], a["read_gc"][GC_BINS + k], a["read_gc"][2 * GC_BINS + k])
    return o, g


def check_reports(lib, h, bq, st, ref):
    want = reports_py(st, windows_np(ref))
    for kind in (REPORT_CYCLES, REPORT_GC):
        got = bq.report(kind)
        assert got == want[kind], [(x, y) for x, y in zip(got.splitlines(), want[kind].splitlines()) if x != y][:5]
    sz = ctypes.c_size_t(7)
    assert bindbq(lib).bwamem_hip_baseqc_report(bq.q, 2, ctypes.byref(sz)) is None and sz.value == 0, "an unknown report"


def check_report_edges(lib, h, ref):
    bq = BaseQc(lib, h)
    try:
        empty = bq.state()
        assert empty["counts"] == dict(records=(0, 0, 0), qcfail_skipped=0, gcb_skipped=0) and all(sum(empty["arrays"][t]) == 0 for t in TABLES)
        check_reports(lib, h, bq, empty, ref)
        assert bq.report(REPORT_CYCLES) == "" and bq.report(REPORT_GC).splitlines()[2].split("\t")[3:] == ["0.000000", "0.0000"], "no end has records; 0 over nothing"
        p = clear_stretch(ref, 0, 300)
        # end 2 only, without qualities, one cycle without any base between soft clips and a deletion: zero denominators inside a table
        bam = brec(b"a", 1 | 0x80, 0, p, "250H2S3M", b"TT" + ref_text(ref, 0, p, 3), qual=0xff) + brec(b"b", 1 | 0x80 | 4, seq=b"N")
        assert bq.add_records(bam) == 0
        st = bq.state()
        check_reports(lib, h, bq, st, ref)
        lines = bq.report(REPORT_CYCLES).splitlines()
        assert lines[0] == "# end 2 records 2" and len(lines) == 2 + 255 and lines[3] == "1\t0\t0.0000" + "\t0.000000" * 5 + "\t0\t0.000000\t0\t0\t0"
        assert lines[-1].split("\t")[:3] == ["254", "1", "0.0000"] and lines[2].split("\t")[7] == "1.000000"
    finally:
        bq.free()


# ------------------------------------------------------------------------------------------ test 5: errors and state
def bad_streams(ref):
    """(name, stream, the BASEQC_ERR_* the checker gives) -- each one refused; good: a stream that is taken"""
    p = clear_stretch(ref, 0, 300)
    r5 = ref_text(ref, 0, p, 5)
    good = [brec(b"g%d" % k, f, 0, p + k, "5M", ref_text(ref, 0, p + k, 5)) for k, f in enumerate((0, 0x10, 1 | 0x40, 1 | 0x80))] + [brec(b"gu", 4, seq=b"ACGTN")]
    bam = b"".join(good)
    length = ref.contigs[0][1]
    overrun, short, neg, contig = bytearray(bam), bytearray(bam), bytearray(bam), bytearray(bam)
    struct.pack_into("<i", overrun, 0, len(bam))
    struct.pack_into("<i", short, 0, 20)
    struct.pack_into("<i", neg, len(bam) - len(good[-1]) + 20, -1)
    struct.pack_into("<i", contig, 4, len(ref.contigs))
    mk = lambda *a, **kw: bam + brec(b"bad", *a, **kw)
    bad = [("truncated", bam[:-5], ERR_WALK), ("block_size overruns", bytes(overrun), ERR_WALK), ("block_size 20", bytes(short), ERR_WALK),
           ("l_seq -1 in the last record", bytes(neg), ERR_WALK), ("refID = n_contigs", bytes(contig), ERR_CONTIG),
           ("refID = n_contigs on a secondary record", mk(0x100, len(ref.contigs), 5, "5M", r5), ERR_CONTIG),
           ("a mapped primary without a CIGAR", mk(0, 0, p, "", r5), ERR_CIGAR), ("a CIGAR one base short", mk(0, 0, p, "4M", r5), ERR_CIGAR),
           ("a CIGAR one base long", mk(0, 0, p, "3M3I", r5), ERR_CIGAR), ("an H inside", mk(0, 0, p, "2M3H3M", r5), ERR_CIGAR),
           ("a QC-fail mapped primary with a bad CIGAR", mk(0x200, 0, p, "4M", r5), ERR_CIGAR),
           ("refID -1 on a mapped primary", mk(0, -1, 5, "5M", r5), ERR_RANGE), ("pos -1", mk(0, 0, -1, "5M", r5), ERR_RANGE),
           ("pos + span one base past the contig end", mk(0, 0, length - 4, "5M", r5), ERR_RANGE),
           ("a deletion that runs past the contig end", mk(0, 0, length - 5, "3M3D2M", r5), ERR_RANGE),
           ("a CIGAR and a range error in one stream", mk(0, 0, length - 4, "5M", r5) + brec(b"bad2", 0, 0, p, "4M", r5), ERR_CIGAR | ERR_RANGE)]
    fits = bam + brec(b"end", 0, 0, length - 5, "5M", ref_text(ref, 0, length - 5, 5)) + brec(b"u", 4, -1, -1, "4M", r5) + brec(b"s", 0x100, 0, length, "9M", r5)
    return good, bad, fits


def check_errors_and_state(lib, h, seqs, ref, tmpdir, other_img):
    d = bindbq(lib)
    good, bad, fits = bad_streams(ref)
    bq, qc = BaseQc(lib, h), Qc(lib, h)
    try:
        assert bq.add_records(fits) == 0 and isinstance(baseqc_py(fits, ref.contigs, ref.codes, ref.holes), dict), "ending exactly at the contig end; unchecked CIGARs of records that are not mapped primaries"
        assert bq.state() == baseqc_py(fits, ref.contigs, ref.codes, ref.holes)
        before = bq.serialize()
        for name, stream, code in bad:
            assert baseqc_py(stream, ref.contigs, ref.codes, ref.holes) == code, name
            assert bq.add_records(stream) != 0, name
            assert bq.serialize() == before, name
        # blobs of another index, of another version, truncated
        ho = lib.open_index(other_img)
        other = BaseQc(lib, ho)
        try:
            assert bq.add_serialized(other.serialize()) != 0 and bq.serialize() == before, "a blob of another n_contigs"
        finally:
            other.free()
            lib.destroy_index(ho)
        vers = bytearray(before)
        vers[8] ^= 3
        assert bq.add_serialized(bytes(vers)) != 0 and bq.add_serialized(before[:-8]) != 0 and bq.add_serialized(before[:16]) != 0 and bq.add_serialized(before + b"\0" * 8) != 0
        assert bq.add_serialized(qc.serialize()) != 0 and bq.serialize() == before, "the record-level QC's blob is another type"
        twice = BaseQc(lib, h)
        try:
            assert twice.add_serialized(before) == 0 and twice.serialize() == before and twice.add_serialized(before) == 0
            assert bq.add_records(fits) == 0 and bq.serialize() == twice.serialize(), "adding a blob is adding its records"
        finally:
            twice.free()
        before, qc_before = bq.serialize(), qc.serialize()
        # a batch without encoded records; calls that fail after the reduction leave both accumulators as they were
        reads, names, quals = planted_single(seqs)
        t1 = fastq_text(reads, names, quals)
        b, _ = upload(lib, h, t1, None)
        assert b
        bt = Batch(lib, h, lib.default_options(), None, b=b)
        try:
            assert bq.add_batch(bt.b) != 0 and bq.serialize() == before, "add_batch before encode"
        finally:
            bt.free()
        assert bq.add_batch(None) != 0
        rc, _ = one_call_metrics(lib, h, lib.default_options(), None, t1, None, tmpdir, "closed", qc, bq, closed_fd=True, sort=0, mark_dup=1, write_header=1)
        assert rc != 0 and bq.serialize() == before and qc.serialize() == qc_before, "a call that fails at the write leaves both untouched"
        rc, _ = one_call_metrics(lib, h, lib.default_options(), None, b"@r\nACGT\n+\n", None, tmpdir, "malformed", qc, bq, sort=0, mark_dup=0, write_header=1)
        assert rc != 0 and bq.serialize() == before and qc.serialize() == qc_before
        # an empty stream and an empty batch add nothing and succeed
        assert bq.add_records(b"") == 0 and bq.serialize() == before
    finally:
        bq.free(), qc.free()
    assert d.bwamem_hip_baseqc_counts(None, None) != 0 and d.bwamem_hip_baseqc_create(None) is None and d.bwamem_hip_index_gc_windows(None, None) != 0


# ------------------------------------------------------------------------------------------ CPU suite (emulation build)
@pytest.fixture(scope="module")
def emu_index(small_genome, tmp_path_factory):
    B.build_emu()
    emu = B.product_lib(emu=True)
    seqs, img = small_genome
    h = emu.open_index(img)
    before = untouched_bytes(emu, h, seqs, str(tmp_path_factory.mktemp("before")))     # (test 6: before any base-QC object exists in this module)
    yield emu, h, seqs, load_ref(img, seqs), before
    emu.destroy_index(h)


def test_baseqc_hand_made_records(emu_index):
    emu, h, _, ref, _ = emu_index
    check_hand_records(emu, h, ref)


@pytest.mark.parametrize("genome", ["small", "alt"])
def test_baseqc_random_records_against_the_checker(emu_index, alt_genome, genome):
    emu, h, _, ref, _ = emu_index
    if genome == "small":
        check_random_sets(emu, h, ref)
        return
    ha = emu.open_index(alt_genome[1])
    try:
        check_random_sets(emu, ha, load_ref(alt_genome[1], alt_genome[0]), seed0=900)
    finally:
        emu.destroy_index(ha)


def test_baseqc_windows_against_numpy(emu_index, alt_genome, tmp_path):
    emu, h, _, ref, _ = emu_index
    assert sum(check_windows(emu, h, ref)) > 0 and len(ref.holes) > 0
    for seqs, img in ((alt_genome[0], alt_genome[1]), tiny_genome(emu, str(tmp_path))):
        hx = emu.open_index(img)
        try:
            rx = load_ref(img, seqs)
            want = check_windows(emu, hx, rx)
            if img.endswith("tiny.fa.img"):
                assert sum(want) == (1500 - 701 - W + 1) + (700 - 3 - W + 1) + (4990 - 1620 - W + 1) + 1 + 2, "the contigs of 60 and 99 bases have no window, those of 100 and 101 one and two"
        finally:
            emu.destroy_index(hx)


def test_baseqc_end_to_end(emu_index, tmp_path):
    emu, h, seqs, ref, _ = emu_index
    check_end_to_end(emu, h, seqs, ref, str(tmp_path))


def test_baseqc_errors_and_state(emu_index, alt_genome, tmp_path):
    emu, h, seqs, ref, _ = emu_index
    check_errors_and_state(emu, h, seqs, ref, str(tmp_path), alt_genome[1])


def test_baseqc_earlier_calls_untouched(emu_index, tmp_path):
    """test 6: after base-QC objects have existed and taken batches in the process, the bytes of the calls that existed before are what
    they were"""
    emu, h, seqs, ref, before = emu_index
    bq = BaseQc(emu, h)
    try:
        name, opts, paired, pes, src = end_to_end_sets(emu, seqs)[0]
        assert one_call_metrics(emu, h, opts, pes, src["t1"], None, str(tmp_path), "q", None, bq, sort=1, mark_dup=1, write_header=1)[0] == 0
        assert sum(bq.state()["counts"]["records"]) > 0
    finally:
        bq.free()
    assert untouched_bytes(emu, h, seqs, str(tmp_path)) == before


def test_baseqc_reports(emu_index):
    emu, h, _, ref, _ = emu_index
    check_report_edges(emu, h, ref)
    bq = BaseQc(emu, h)
    try:
        bam = b"".join(random_records(257, 61, ref))
        assert bq.add_records(bam) == 0
        check_reports(emu, h, bq, baseqc_py(bam, ref.contigs, ref.codes, ref.holes), ref)
    finally:
        bq.free()


def test_baseqc_python_mirror(emu_index, small_genome, tmp_path):
    """BwaMemAligner.newBaseQc() and the base_qc= argument of alignFastqToBam / alignSeqsToBam over the emulation build, in a child process"""
    emu, h, seqs, ref, _ = emu_index
    _, img = small_genome
    reads, names, quals = planted_single(seqs)
    fq = str(tmp_path / "in.fq")
    with open(fq, "wb") as f:
        f.write(fastq_text(reads, names, quals))
    p = {k: str(tmp_path / k) for k in ("a.bam", "b.bam", "c.bam", "plain.bam")}
    r = subprocess.run([sys.executable, "-c", (
        "import sys; sys.path.insert(0, %r); import bwamem\n"
        "ix = bwamem.BwaMemIndex(%r); al = bwamem.BwaMemAligner(ix)\n"
        "reads, p, fq = %r, %r, %r\n"
        "a, b, both, qc = al.newBaseQc(), al.newBaseQc(), al.newBaseQc(), al.newQc()\n"
        "al.alignFastqToBam(fq, p['a.bam'], sort=True, mark_duplicates=True, qc=qc, base_qc=a)\n"
        "al.alignSeqsToBam(reads, p['b.bam'], device=True, base_qc=b)\n"
        "al.alignFastqToBam(fq, p['c.bam'], sort=True, base_qc=both); al.alignSeqsToBam(reads, p['c.bam'], device=True, base_qc=both)\n"
        "al.alignSeqsToBam(reads, p['plain.bam'], device=True)\n"
        "print('A', sorted(a.counts().items())); print('B', sorted(b.counts().items())); print('QC', qc.counts()['sequences'])\n"
        "print('ARR', a.array('aligned')[:90], a.array('gcb_reads'), len(a.array('base')))\n"
        "blob = both.serialize(); a.add(b.serialize()); print('SUM', a.serialize() == blob, a.counts() == both.counts())\n"
        "print('TEXT', repr(a.cycles()), repr(a.gcBias()))\n"
        "print('WIN', ix.gcWindows())\n"
        "cb = b.serialize()\n"
        "try:\n    al.alignSeqsToBam(reads, p['c.bam'] + 'x', base_qc=b)\nexcept ValueError:\n    print('host-framing-refused', 'kept' if b.serialize() == cb else 'changed')\n"
        "try:\n    a.array('nope')\nexcept ValueError:\n    print('unknown-array')\n"
        "try:\n    a.add(qc.serialize())\nexcept ValueError:\n    print('foreign-blob-refused')\n"
        "a.close(); b.close(); both.close(); qc.close(); al.close(); ix.close()\n") % (B.PKG, img, reads, p, fq)],
        env=dict(os.environ, LIBBWA_PATH=B.EMU_LIB), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "host-framing-refused kept" in r.stdout and "unknown-array" in r.stdout and "SUM True True" in r.stdout, (r.stdout[-1500:], r.stderr[-2000:])
    assert "foreign-blob-refused" in r.stdout and not os.path.exists(p["c.bam"] + "x")
    assert open(p["b.bam"], "rb").read() == open(p["plain.bam"], "rb").read(), "base_qc= does not change the file"
    want_a = baseqc_py(bam_file_records(open(p["a.bam"], "rb").read()), ref.contigs, ref.codes, ref.holes)
    want_b = baseqc_py(bam_file_records(open(p["b.bam"], "rb").read()), ref.contigs, ref.codes, ref.holes)
    lines = dict(ln.split(" ", 1) for ln in r.stdout.splitlines() if ln.split(" ", 1)[0] in ("A", "B", "QC", "ARR", "TEXT", "WIN"))
    as_items = lambda st: str(sorted(dict(st["counts"], records=list(st["counts"]["records"])).items()))
    assert lines["A"] == as_items(want_a) and lines["B"] == as_items(want_b) and int(lines["QC"]) == len(reads)
    assert lines["ARR"] == "%s %s %d" % (want_a["arrays"]["aligned"][:90], want_a["arrays"]["gcb_reads"], 3 * CYCLES * 5)
    windows = windows_np(ref)
    assert lines["TEXT"] == "%r %r" % reports_py(add_states(want_a, want_b), windows) and lines["WIN"] == str(windows)


def state_words(st):
    """a state as the 64-bit words the sanitizer driver compares: the counters in struct order, then the tables in BWAMEM_HIP_BASEQC_* order"""
    w = list(st["counts"]["records"]) + [st["counts"]["qcfail_skipped"], st["counts"]["gcb_skipped"]]
    for n in TABLES:
        w += st["arrays"][n]
    return struct.pack("<%dQ" % len(w), *w)


def test_baseqc_sanitizers(emu_index, small_genome, tmp_path):
    """the base-QC calls under AddressSanitizer + UBSan: a stand-alone driver (tests/bam_baseqc_sanitized_driver.cpp), compiled here with
    the sanitizers and linked against the sanitized emulation build (tests/emu `make asan`), run as a program.  It compares what the
    accumulator holds with the checker's words, written here, for record sets of tests 1, 2 and 5, and windows[] with numpy's."""
    B.make(os.path.join(B.ROOT, "tests", "emu"), "asan")
    _, _, seqs, ref, _ = emu_index
    _, img = small_genome
    manifest = []

    def add(kind, tag, bam):
        with open(str(tmp_path / (tag + ".bam")), "wb") as f:
            f.write(bam)
        if kind == "rec":
            with open(str(tmp_path / (tag + ".want")), "wb") as f:
                f.write(state_words(baseqc_py(bam, ref.contigs, ref.codes, ref.holes)))
        manifest.append("%s %s" % (kind, tag))
    good, bad, fits = bad_streams(ref)
    p = clear_stretch(ref, 0, 1100)
    hand = fits + b"".join(brec(b"l%d" % f, f, 0, p, "3H1030M2H", ref_text(ref, 0, p, 1030)) for f in (0, 0x10)) + brec(b"id", 0, 0, p, "2I3M2D4M", b"GG" + ref_text(ref, 0, p, 7))
    add("rec", "hand", hand)
    for k, n in enumerate((1, 33, 257)):
        add("rec", "rand%d" % k, b"".join(random_records(n, 2000 + k, ref)))
    for k, (name, stream, code) in enumerate(bad):
        add("bad", "bad%d" % k, stream)
    with open(str(tmp_path / "manifest.txt"), "w") as f:
        f.write("\n".join(manifest) + "\n")
    with open(str(tmp_path / "windows.want"), "wb") as f:
        f.write(struct.pack("<%dQ" % GC_BINS, *windows_np(ref)))
    emu_dir = os.path.join(B.ROOT, "tests", "emu", "_build")
    exe = str(tmp_path / "bam_baseqc_sanitized_driver")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(B.ROOT, "include"), os.path.join(B.ROOT, "tests", "bam_baseqc_sanitized_driver.cpp"), "-o", exe,
                    "-L", emu_dir, "-lbwamem_emu_asan", "-Wl,-rpath," + emu_dir], check=True)
    r = subprocess.run([exe, img, str(tmp_path)], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0"),
                       capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "sanitized-ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


# ------------------------------------------------------------------------------------------ GPU suite
@pytest.mark.gpu
def test_gpu_baseqc_small_cases(hip_lib, small_genome, alt_genome, tmp_path):
    """(a) tests 1-5 and the reports on the device"""
    seqs, img = small_genome
    h = hip_lib.open_index(img)
    ha = hip_lib.open_index(alt_genome[1])
    try:
        ref, ref_alt = load_ref(img, seqs), load_ref(alt_genome[1], alt_genome[0])
        check_hand_records(hip_lib, h, ref)
        check_random_sets(hip_lib, h, ref)
        check_random_sets(hip_lib, ha, ref_alt, seed0=900)
        check_windows(hip_lib, h, ref)
        check_windows(hip_lib, ha, ref_alt)
        check_end_to_end(hip_lib, h, seqs, ref, str(tmp_path))
        check_report_edges(hip_lib, h, ref)
        check_errors_and_state(hip_lib, h, seqs, ref, str(tmp_path), alt_genome[1])
    finally:
        hip_lib.destroy_index(h)
        hip_lib.destroy_index(ha)


def blobs_equal(hip_lib, h, emu, he, bam):
    a, b = BaseQc(hip_lib, h), BaseQc(emu, he)
    try:
        assert a.add_records(bam) == 0 and b.add_records(bam) == 0
        same = a.serialize() == b.serialize()
        return same, a.state()
    finally:
        a.free(), b.free()


@pytest.mark.gpu
def test_gpu_baseqc_equals_emulation_medium(hip_lib, medium_genome):
    """(b) the device's serialized accumulator is the emulation build's: random records on the medium genome, and a few hundred reads of
    2 to 10 kb (the wavefront form, the capped last bin)"""
    B.build_emu()
    emu = B.product_lib(emu=True)
    seqs, img = medium_genome
    h, he = hip_lib.open_index(img), emu.open_index(img)
    try:
        ref = load_ref(img, seqs)
        for n in (33, 1500):
            same, _ = blobs_equal(hip_lib, h, emu, he, b"".join(random_records(n, 3000 + n, ref)))
            assert same, n
        long_set = b"".join(random_records(300, 3100, ref, lengths=[2000, 3001, 5000, 7777, 10000], short=False))
        same, st = blobs_equal(hip_lib, h, emu, he, long_set)
        assert same and sum(st["arrays"]["aligned"][CYCLES - 1::CYCLES]) > 100 * 1000, "nearly every base of a long read is in the last bin"
    finally:
        hip_lib.destroy_index(h)
        emu.destroy_index(he)


@pytest.mark.gpu
def test_gpu_baseqc_grid_stride(hip_lib, small_genome):
    """(b) about 150 000 records of 50 bases: more items than one turn of the fixed grid takes.  The emulation build's block is computed
    once from a tenth of the records (the set is that tenth ten times, and blocks add)"""
    B.build_emu()
    emu = B.product_lib(emu=True)
    seqs, img = small_genome
    h, he = hip_lib.open_index(img), emu.open_index(img)
    try:
        ref = load_ref(img, seqs)
        tenth = b"".join(random_records(15000, 3200, ref, lengths=[50], short=False))
        a, b = BaseQc(hip_lib, h), BaseQc(emu, he)
        try:
            assert a.add_records(tenth * 10) == 0 and b.add_records(tenth) == 0
            part = b.serialize()
            for _ in range(9):
                assert b.add_serialized(part) == 0
            assert a.serialize() == b.serialize() and sum(a.state()["counts"]["records"]) > 120000
        finally:
            a.free(), b.free()
    finally:
        hip_lib.destroy_index(h)
        emu.destroy_index(he)


@pytest.mark.gpu
def test_gpu_baseqc_windows_medium(hip_lib, medium_genome):
    """(c) windows[] of the medium genome against numpy: more than one tile per workgroup"""
    seqs, img = medium_genome
    h = hip_lib.open_index(img)
    try:
        assert sum(check_windows(hip_lib, h, load_ref(img, seqs))) > 2900000
    finally:
        hip_lib.destroy_index(h)
