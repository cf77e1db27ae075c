"""Alignment QC on the device (csrc/bam_qc.h, the k_qc_* kernels in csrc/k_post.hip, the bwamem_hip_qc_* calls, the report writers in
csrc/sam_writer.cpp, bwamem_hip_fastq_to_bam_qc, BwaMemQc in bwamem.py).  The reference is qc_py below: the rule restated with dicts
and collections.Counter over parse_records / split_records, from the record bytes alone.  Every counter and every array element is
compared for exact equality; report text is compared as bytes, except its doubles (relative 1e-9: both sides do a handful of double
operations on exact integer sums).  Parity with samtools or Picard output is not checked: neither tool is where this suite runs.
CPU suite: the emulation build runs the kernels.  GPU suite (-m gpu): the same on the device, the medium genome, long reads, and the
device's serialized accumulator against the emulation build's."""
import collections
import ctypes
import math
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

import bwalib as B
from test_bam_dup import PES, DupCounts, bindd, end_to_end_sets, planted_single, repeat_every_tenth, seeded_quals, untouched_bytes
from test_bam_quals import Batch, quals_blob
from test_bam_sorted import TILE, split_records
from test_bam_tags import BamOptions, bindt
from test_bam_writer import CIG_OPS, _take, parse_records, reg2bin
from test_fastq_device import fastq_text, upload
from test_fastq_gz import bgzf_cut

PAIRS = ["total", "primary", "secondary", "supplementary", "duplicates", "primary_duplicates", "mapped", "primary_mapped", "paired", "read1", "read2",
         "properly_paired", "both_mapped", "singletons", "mate_diff_chr", "mate_diff_chr_mapq5"]
SINGLES = ["unplaced", "sequences", "total_length", "max_length", "reads_mq0", "bases_mapped", "bases_mapped_cigar", "bases_soft_clipped", "ins_events", "ins_bases",
           "del_events", "del_bases", "mismatches", "records_without_nm"]
ARRAYS = ["mapq_hist", "qual_hist", "isize_fr", "isize_rf", "isize_tandem", "contig_mapped", "contig_unmapped"]
ISIZE_BINS = 16384
FLAGSTAT, IDXSTATS, SUMMARY, INSERT_SIZE = range(4)
U32_MAX = 0xffffffff


class QcCounts(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_uint64 * 2) for n in PAIRS] + [(n, ctypes.c_uint64) for n in SINGLES]
                + [("isize_min", ctypes.c_uint64 * 3), ("isize_max", ctypes.c_uint64 * 3)])


# ------------------------------------------------------------------------------------------ bindings
def bindqc(lib):
    d = bindt(lib)
    bindd(lib)
    if getattr(d, "_qc_bound", False):
        return d
    vp, sz, cp, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_int
    d.bwamem_hip_qc_create.restype = vp
    d.bwamem_hip_qc_create.argtypes = [vp]
    d.bwamem_hip_qc_free.restype = None
    d.bwamem_hip_qc_free.argtypes = [vp]
    d.bwamem_hip_qc_add_batch.argtypes = [vp, vp]
    d.bwamem_hip_qc_add_records_device.argtypes = [vp, cp, sz]
    d.bwamem_hip_qc_counts.argtypes = [vp, ctypes.POINTER(QcCounts)]
    d.bwamem_hip_qc_array.restype = ctypes.c_int64
    d.bwamem_hip_qc_array.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_uint64), sz]
    d.bwamem_hip_qc_serialize.restype = vp
    d.bwamem_hip_qc_serialize.argtypes = [vp, ctypes.POINTER(sz)]
    d.bwamem_hip_qc_add_serialized.argtypes = [vp, cp, sz]
    d.bwamem_hip_qc_report.restype = vp
    d.bwamem_hip_qc_report.argtypes = [vp, ci, ctypes.POINTER(sz)]
    d.bwamem_hip_fastq_to_bam_qc.argtypes = [vp, vp, vp, cp, sz, cp, sz, ctypes.POINTER(BamOptions), ci, ci, ctypes.POINTER(DupCounts), vp]
    d._qc_bound = True
    return d


class Qc:
    """one accumulator of `lib` over the index h"""

    def __init__(self, lib, h):
        self.lib, self.d = lib, bindqc(lib)
        self.q = self.d.bwamem_hip_qc_create(h)
        assert self.q

    def add_records(self, bam):
        return self.d.bwamem_hip_qc_add_records_device(self.q, bytes(bam), len(bam))

    def add_batch(self, b):
        return self.d.bwamem_hip_qc_add_batch(self.q, b)

    def state(self):
        c = QcCounts()
        assert self.d.bwamem_hip_qc_counts(self.q, ctypes.byref(c)) == 0
        counts = {n: (int(getattr(c, n)[0]), int(getattr(c, n)[1])) for n in PAIRS}
        counts.update({n: int(getattr(c, n)) for n in SINGLES})
        counts["isize_min"], counts["isize_max"] = tuple(int(x) for x in c.isize_min), tuple(int(x) for x in c.isize_max)
        arrays = {}
        for k, name in enumerate(ARRAYS):
            n = self.d.bwamem_hip_qc_array(self.q, k, None, 0)
            buf = (ctypes.c_uint64 * max(n, 1))()
            assert self.d.bwamem_hip_qc_array(self.q, k, buf, n) == n
            arrays[name] = [int(x) for x in buf[:n]]
        assert self.d.bwamem_hip_qc_array(self.q, len(ARRAYS), None, 0) < 0
        return dict(counts=counts, arrays=arrays)

    def serialize(self):
        sz = ctypes.c_size_t()
        p = self.d.bwamem_hip_qc_serialize(self.q, ctypes.byref(sz))
        assert p
        return _take(self.lib, p, sz.value)

    def add_serialized(self, blob):
        return self.d.bwamem_hip_qc_add_serialized(self.q, blob, len(blob))

    def report(self, kind):
        sz = ctypes.c_size_t()
        p = self.d.bwamem_hip_qc_report(self.q, kind, ctypes.byref(sz))
        assert p
        return _take(self.lib, p, sz.value).decode()

    def free(self):
        self.d.bwamem_hip_qc_free(self.q)


# ------------------------------------------------------------------------------------------ the rule in Python (the issue's text)
def qc_py(bam, n_contigs):
    """-> dict(counts=..., arrays=...) of the record stream, shaped like Qc.state()"""
    flag = {n: [0, 0] for n in PAIRS}
    one = collections.Counter()
    mapq_hist, qual_hist, isize = collections.Counter(), collections.Counter(), [collections.Counter() for _ in range(3)]
    mapped_on, unmapped_on = collections.Counter(), collections.Counter()
    imin, imax, max_length = [U32_MAX] * 3, [0] * 3, 0
    for r in parse_records(bam):
        f, w = r["flag"], 1 if r["flag"] & 0x200 else 0
        assert r["refid"] < n_contigs and r["l_seq"] >= 0
        ops = [(CIG_OPS[c & 15], c >> 4) for c in r["cig"]]
        primary, mapped = not f & 0x900, not f & 4
        flag["total"][w] += 1
        if f & 0x100:
            flag["secondary"][w] += 1
        elif f & 0x800:
            flag["supplementary"][w] += 1
        else:
            flag["primary"][w] += 1
            if mapped:
                flag["primary_mapped"][w] += 1
            if f & 0x400:
                flag["primary_duplicates"][w] += 1
            if f & 1:
                flag["paired"][w] += 1
                if f & 2 and mapped:
                    flag["properly_paired"][w] += 1
                if f & 0x40:
                    flag["read1"][w] += 1
                if f & 0x80:
                    flag["read2"][w] += 1
                if f & 8 and mapped:
                    flag["singletons"][w] += 1
                if mapped and not f & 8:
                    flag["both_mapped"][w] += 1
                    if r["refid"] != r["nrid"]:
                        flag["mate_diff_chr"][w] += 1
                        if r["mapq"] >= 5:
                            flag["mate_diff_chr_mapq5"][w] += 1
        if mapped:
            flag["mapped"][w] += 1
        if f & 0x400:
            flag["duplicates"][w] += 1
        if r["refid"] < 0:
            one["unplaced"] += 1
        else:
            (mapped_on if mapped else unmapped_on)[r["refid"]] += 1
        if primary:
            one["sequences"] += 1
            one["total_length"] += r["l_seq"]
            max_length = max(max_length, r["l_seq"])
            if r["l_seq"] and r["qual"][0] != 0xff:
                qual_hist.update(min(q, 127) for q in r["qual"])
        if primary and mapped:
            one["reads_mq0"] += r["mapq"] == 0
            one["bases_mapped"] += r["l_seq"]
            one["bases_mapped_cigar"] += sum(n for o, n in ops if o in "MI=X")
            one["bases_soft_clipped"] += sum(n for o, n in ops if o == "S")
            one["ins_events"] += sum(1 for o, n in ops if o == "I")
            one["ins_bases"] += sum(n for o, n in ops if o == "I")
            one["del_events"] += sum(1 for o, n in ops if o == "D")
            one["del_bases"] += sum(n for o, n in ops if o == "D")
            first = r["tags"][0] if r["tags"] else None
            if first and first[0] == "NM" and first[1] in "cCsSiI":
                one["mismatches"] += max(first[2], 0)
            else:
                one["records_without_nm"] += 1
            mapq_hist[r["mapq"]] += 1
        if f & 1 and f & 0x40 and not f & 0xD0C and r["refid"] == r["nrid"] and r["tlen"] != 0:
            x = abs(r["tlen"])
            span = sum(n for o, n in ops if o in "MDN=X")
            if bool(f & 0x10) == bool(f & 0x20):
                o = 2
            elif not f & 0x10:
                o = 0 if r["tlen"] > 0 else 1
            else:
                o = 0 if r["npos"] + 1 < r["pos"] + span else 1
            isize[o][min(x, ISIZE_BINS - 1)] += 1
            imin[o], imax[o] = min(imin[o], x), max(imax[o], x)
    counts = {n: tuple(v) for n, v in flag.items()}
    counts.update({n: int(one[n]) for n in SINGLES})
    counts["max_length"] = max_length
    counts["isize_min"], counts["isize_max"] = tuple(imin), tuple(imax)
    dense = lambda c, n: [int(c[k]) for k in range(n)]
    arrays = dict(mapq_hist=dense(mapq_hist, 256), qual_hist=dense(qual_hist, 128), isize_fr=dense(isize[0], ISIZE_BINS), isize_rf=dense(isize[1], ISIZE_BINS),
                  isize_tandem=dense(isize[2], ISIZE_BINS), contig_mapped=dense(mapped_on, n_contigs), contig_unmapped=dense(unmapped_on, n_contigs))
    return dict(counts=counts, arrays=arrays)


def add_states(a, b):
    """what an accumulator holds after a and b"""
    c = {}
    for n in PAIRS:
        c[n] = (a["counts"][n][0] + b["counts"][n][0], a["counts"][n][1] + b["counts"][n][1])
    for n in SINGLES:
        c[n] = max(a["counts"][n], b["counts"][n]) if n == "max_length" else a["counts"][n] + b["counts"][n]
    c["isize_min"] = tuple(min(x, y) for x, y in zip(a["counts"]["isize_min"], b["counts"]["isize_min"]))
    c["isize_max"] = tuple(max(x, y) for x, y in zip(a["counts"]["isize_max"], b["counts"]["isize_max"]))
    return dict(counts=c, arrays={n: [x + y for x, y in zip(a["arrays"][n], b["arrays"][n])] for n in ARRAYS})


# ------------------------------------------------------------------------------------------ the reports in Python (the issue's text)
LABELS = ["in total (QC-passed reads + QC-failed reads)", "primary", "secondary", "supplementary", "duplicates", "primary duplicates", "mapped", "primary mapped",
          "paired in sequencing", "read1", "read2", "properly paired", "with itself and mate mapped", "singletons", "with mate mapped to a different chr",
          "with mate mapped to a different chr (mapQ>=5)"]
ISIZE_HEADER = ("PAIR_ORIENTATION\tREAD_PAIRS\tMIN_INSERT_SIZE\tMAX_INSERT_SIZE\tMEDIAN_INSERT_SIZE\tMEDIAN_ABSOLUTE_DEVIATION\tMEAN_INSERT_SIZE\t"
                "STANDARD_DEVIATION\n")


def median_of(pairs, n):
    """the median of the values v, each cnt times, of the ascending (v, cnt) list; n values in all"""
    want, got, seen = [(n - 1) // 2, n // 2], [], 0
    for v, cnt in pairs:
        seen += cnt
        while len(got) < 2 and seen > want[len(got)]:
            got.append(v)
    return (got[0] + got[1]) / 2


def isize_stats(h):
    n = sum(h)
    vals = [(v, c) for v, c in enumerate(h) if c]
    med = median_of(vals, n)
    dev = collections.Counter()
    for v, c in vals:
        dev[abs(v - med)] += c
    mad = median_of(sorted(dev.items()), n)
    kept = [(v, c) for v, c in vals if v <= med + 10 * mad]
    m, s, sq = sum(c for _, c in kept), sum(v * c for v, c in kept), sum(v * v * c for v, c in kept)
    mean = float(s) / float(m)
    sd = math.sqrt(float(m * sq - s * s) / float(m) / float(m - 1)) if m >= 2 else 0.0
    return n, med, mad, mean, sd


def reports_py(st, contigs):
    """the four texts of a state; contigs: (name, length) in index order"""
    c, a = st["counts"], st["arrays"]
    pct = lambda x, y: "%.2f%%" % (100.0 * x / y) if y else "N/A"
    flagstat = ""
    den = {"mapped": "total", "primary_mapped": "primary", "properly_paired": "paired", "singletons": "paired"}
    for name, label in zip(PAIRS, LABELS):
        flagstat += "%d + %d %s" % (c[name][0], c[name][1], label)
        if name in den:
            flagstat += " (%s : %s)" % (pct(c[name][0], c[den[name]][0]), pct(c[name][1], c[den[name]][1]))
        flagstat += "\n"
    idxstats = "".join("%s\t%d\t%d\t%d\n" % (nm, ln, a["contig_mapped"][k], a["contig_unmapped"][k]) for k, (nm, ln) in enumerate(contigs))
    idxstats += "*\t0\t0\t%d\n" % c["unplaced"]
    ratio = lambda x, y: "%.6f" % (float(x) / float(y)) if y else "N/A"
    qh = a["qual_hist"]
    summary = "".join("%s\t%d\n" % (n, c[n]) for n in SINGLES)
    summary += "error_rate\t%s\n" % ratio(c["mismatches"], c["bases_mapped_cigar"])
    summary += "average_length\t%s\n" % ratio(c["total_length"], c["sequences"])
    summary += "average_quality\t%s\n" % ratio(sum(q * n for q, n in enumerate(qh)), sum(qh))
    summary += "q20_bases\t%d\nq30_bases\t%d\n" % (sum(qh[20:]), sum(qh[30:]))
    summary += "percent_duplication\t%s\n" % ratio(sum(c["primary_duplicates"]), sum(c["primary_mapped"]))
    hs = [a["isize_fr"], a["isize_rf"], a["isize_tandem"]]
    ins = ISIZE_HEADER
    for k, name in enumerate(("FR", "RF", "TANDEM")):
        if sum(hs[k]):
            n, med, mad, mean, sd = isize_stats(hs[k])
            ins += "%s\t%d\t%d\t%d\t%.1f\t%.1f\t%.6f\t%.6f\n" % (name, n, c["isize_min"][k], c["isize_max"][k], med, mad, mean, sd)
    ins += "\ninsert_size\tFR\tRF\tTANDEM\n"
    ins += "".join("%d\t%d\t%d\t%d\n" % (v, hs[0][v], hs[1][v], hs[2][v]) for v in range(ISIZE_BINS) if hs[0][v] or hs[1][v] or hs[2][v])
    return [flagstat, idxstats, summary, ins]


def same_text(got, want):
    """equal as bytes, except fields that are doubles on both sides: those to a relative 1e-9"""
    gl, wl = got.split("\n"), want.split("\n")
    assert len(gl) == len(wl), (got[-400:], want[-400:])
    for x, y in zip(gl, wl):
        xf, yf = x.split("\t"), y.split("\t")
        assert len(xf) == len(yf), (x, y)
        for p, q in zip(xf, yf):
            if p != q:
                assert re.fullmatch(r"-?\d+\.\d+", p) and re.fullmatch(r"-?\d+\.\d+", q) and math.isclose(float(p), float(q), rel_tol=1e-9), (x, y)


def check_reports(qc, st, contigs):
    for kind, want in enumerate(reports_py(st, contigs)):
        got = qc.report(kind)
        if kind in (FLAGSTAT, IDXSTATS):
            assert got == want, (got, want)
        else:
            same_text(got, want)


def contigs_of(seqs):
    return [(n if isinstance(n, str) else n.decode(), len(s)) for n, s in seqs]


# ------------------------------------------------------------------------------------------ test 1: hand-made records
def qrec(name, flag, refid=-1, pos=-1, cigar="", qual=30, l_seq=None, nrid=-1, npos=-1, mapq=60, tlen=0, aux=b""):
    """rec() of test_bam_dup.py with mapq, tlen, aux bytes and any flag"""
    cig = [(int(n), CIG_OPS.index(o)) for n, o in re.findall(r"(\d+)([MIDNSHP=X])", cigar)]
    if l_seq is None:
        l_seq = sum(n for n, o in cig if CIG_OPS[o] in "MIS=X")
    q = bytes([qual]) * l_seq if isinstance(qual, int) else qual
    assert len(q) == l_seq
    span = sum(n for n, o in cig if CIG_OPS[o] in "MDN=X")
    nm = name + b"\0"
    body = struct.pack("<iiBBHHHiiii", refid, pos, len(nm), mapq, reg2bin(pos, pos + max(span, 1)) & 0xffff if pos >= 0 else 4680, len(cig), flag, l_seq, nrid, npos, tlen)
    body += nm + b"".join(struct.pack("<I", n << 4 | o) for n, o in cig) + b"\x11" * ((l_seq + 1) // 2) + q + aux
    return struct.pack("<i", len(body)) + body


def nm_aux(ty, v):
    return b"NM" + ty.encode() + struct.pack("<" + {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I"}[ty], v)


RG_AUX = b"RGZgrp\0"


def hand_records(n_contigs):
    """for each line of the rule a record that takes it and one that just misses it"""
    last = n_contigs - 1
    pair = lambda **kw: dict(dict(refid=0, pos=1000, cigar="50M", nrid=0, npos=1200, aux=nm_aux("C", 1)), **kw)
    r = []
    r.append(qrec(b"plain", 0, 0, 100, "100M", aux=nm_aux("C", 3)))
    r.append(qrec(b"qcfail", 0x200, 0, 100, "100M", aux=nm_aux("C", 2)))
    r.append(qrec(b"qcfail_pair", 0x200 | 1 | 2 | 0x40 | 0x20, **pair(tlen=250)))
    r.append(qrec(b"sec_and_sup", 0x100 | 0x800, 1, 100, "40M60S", aux=nm_aux("C", 9)))
    r.append(qrec(b"sup", 0x800, 1, 100, "60H40M", aux=nm_aux("C", 9)))
    r.append(qrec(b"sec", 0x100 | 0x400, 1, 100, "100M"))
    r.append(qrec(b"dup", 0x400, 1, 100, "100M", aux=nm_aux("C", 0)))
    r.append(qrec(b"dup_unmapped", 0x400 | 4, 1, 100, "", l_seq=20))
    r.append(qrec(b"proper_but_unmapped", 1 | 2 | 4 | 0x40, 0, 500, "", l_seq=30, nrid=0, npos=500))
    r.append(qrec(b"proper", 1 | 2 | 0x40 | 0x20, **pair(tlen=300)))
    r.append(qrec(b"proper2", 1 | 2 | 0x80 | 0x10, **pair(pos=1250, npos=1000, tlen=-300)))
    r.append(qrec(b"singleton", 1 | 8 | 0x40, 2, 300, "30M", nrid=2, npos=300, aux=nm_aux("C", 1)))
    r.append(qrec(b"singleton_missed", 1 | 8 | 4 | 0x80, 2, 300, "", l_seq=30, nrid=2, npos=300))
    r.append(qrec(b"both_unmapped", 1 | 8 | 4 | 0x40, l_seq=30))
    r.append(qrec(b"diff_chr_mq4", 1 | 0x40 | 0x20, 0, 100, "50M", nrid=1, npos=100, mapq=4, tlen=77, aux=nm_aux("C", 1)))
    r.append(qrec(b"diff_chr_mq5", 1 | 0x80 | 0x20, 0, 100, "50M", nrid=1, npos=100, mapq=5, aux=nm_aux("C", 1)))
    r.append(qrec(b"same_chr_mq5", 1 | 0x80 | 0x20, 0, 100, "50M", nrid=0, npos=100, mapq=5, aux=nm_aux("C", 1)))
    for k, (ty, v) in enumerate((("C", 200), ("S", 40000), ("I", 3000000000), ("c", -3), ("c", 100), ("s", -300), ("s", 300), ("i", -5), ("i", 70000))):
        r.append(qrec(b"nm%d" % k, 0, 1, 100 + k, "20M", aux=nm_aux(ty, v) + RG_AUX))
    r.append(qrec(b"no_aux", 0, 1, 200, "20M"))
    r.append(qrec(b"rg_first", 0, 1, 200, "20M", aux=RG_AUX + nm_aux("C", 7)))
    r.append(qrec(b"nm_as_text", 0, 1, 200, "20M", aux=b"NMZ7\0"))
    r.append(qrec(b"nm_unmapped", 4, 1, 200, "", l_seq=20, aux=nm_aux("C", 7)))
    r.append(qrec(b"no_quals", 0, 1, 300, "25M", qual=0xff, aux=nm_aux("C", 0)))
    r.append(qrec(b"quals_then_ff", 0, 1, 300, "4M", qual=b"\x05\xff\x7e\x7f", aux=nm_aux("C", 0)))
    r.append(qrec(b"high_quals", 0, 1, 300, "5M", qual=b"\x7e\x7f\x80\xc8\xfe", aux=nm_aux("C", 0)))
    r.append(qrec(b"secondary_quals", 0x100, 1, 300, "25M", qual=33))
    r.append(qrec(b"empty", 4, l_seq=0))
    r.append(qrec(b"empty_mapped", 0, 2, 10, "5D", aux=nm_aux("C", 5)))
    r.append(qrec(b"odd", 0, 2, 10, "7M", qual=bytes(range(7)), aux=nm_aux("C", 0)))
    r.append(qrec(b"no_cigar", 0, 2, 10, "", l_seq=10, mapq=0))
    r.append(qrec(b"long_cigar", 0, 2, 50, "1M1I1M1D" * 75, aux=nm_aux("S", 150)))
    r.append(qrec(b"all_ops", 0, 2, 50, "3H4S5M6I7D8N9=10X2P11M12S13H", aux=nm_aux("C", 10)))
    for k, t in enumerate((0, -200, 16382, 16383, 16384, 100000, -16384, 1)):
        r.append(qrec(b"tlen%d" % k, 1 | 0x40 | 0x20, **pair(tlen=t)))
    r.append(qrec(b"fwd_fwd", 1 | 0x40, **pair(tlen=410)))
    r.append(qrec(b"rev_rev", 1 | 0x40 | 0x10 | 0x20, **pair(tlen=-420)))
    r.append(qrec(b"fwd_rev_neg", 1 | 0x40 | 0x20, **pair(tlen=-430)))
    r.append(qrec(b"rev_fwd_inside", 1 | 0x40 | 0x10, **pair(pos=1000, cigar="20M10D20M", npos=1048, tlen=-440)))       # next_pos + 1 < pos + span (1050)
    r.append(qrec(b"rev_fwd_edge", 1 | 0x40 | 0x10, **pair(pos=1000, cigar="20M10D20M", npos=1049, tlen=-450)))         # next_pos + 1 == pos + span
    r.append(qrec(b"rev_fwd_past", 1 | 0x40 | 0x10, **pair(pos=1000, cigar="20M10I20M", npos=1040, tlen=460)))          # span 40: next_pos + 1 > pos + span
    r.append(qrec(b"isize_read2", 1 | 0x80 | 0x20, **pair(tlen=470)))
    r.append(qrec(b"isize_dup", 1 | 0x40 | 0x20 | 0x400, **pair(tlen=470)))
    r.append(qrec(b"isize_sec", 1 | 0x40 | 0x20 | 0x100, **pair(tlen=470)))
    r.append(qrec(b"isize_sup", 1 | 0x40 | 0x20 | 0x800, **pair(tlen=470)))
    r.append(qrec(b"isize_mate_unmapped", 1 | 0x40 | 0x20 | 8, **pair(tlen=470)))
    r.append(qrec(b"isize_unpaired", 0x40 | 0x20, **pair(tlen=470)))
    r.append(qrec(b"isize_other_contig", 1 | 0x40 | 0x20, **pair(nrid=last, tlen=470)))
    r.append(qrec(b"mq0", 0, last, 10, "10M", mapq=0, aux=nm_aux("C", 0)))
    r.append(qrec(b"mq255", 0, last, 10, "10M", mapq=255, aux=nm_aux("C", 0)))
    r.append(qrec(b"mq0_unmapped", 4, last, 10, "", l_seq=10, mapq=0))
    r.append(qrec(b"unplaced_mapped_flag", 0, -1, -1, "", l_seq=3))
    r.append(qrec(b"refid_minus_2", 4, -2, -1, "", l_seq=3))
    return r


def check_hand_records(lib, h, contigs):
    n_contigs = len(contigs)
    bam = b"".join(hand_records(n_contigs))
    want = qc_py(bam, n_contigs)
    c, a = want["counts"], want["arrays"]
    # the checker itself, on figures read off the list above
    assert c["total"] == (len(hand_records(n_contigs)) - 2, 2) and c["secondary"] == (4, 0) and c["supplementary"] == (2, 0) and c["duplicates"] == (4, 0)
    assert c["primary_duplicates"] == (3, 0) and c["properly_paired"] == (2, 1) and c["singletons"] == (2, 0)
    assert c["mate_diff_chr"] == (3, 0) and c["mate_diff_chr_mapq5"] == (2, 0) and c["unplaced"] == 4
    assert c["mismatches"] >= 200 + 40000 + 3000000000 + 100 + 300 + 70000 and c["max_length"] == 150 + 75
    assert c["isize_min"] == (1, 200, 410) and c["isize_max"] == (100000, 16384, 420)
    assert a["isize_fr"][16382] == 1 and a["isize_fr"][16383] == 3 and a["isize_rf"][16383] == 1 and a["isize_fr"][440] == 1 and a["isize_rf"][450] == 1 and a["isize_rf"][460] == 1
    assert a["isize_fr"][470] == 0 and a["isize_tandem"][410] == 1 and a["mapq_hist"][0] == 2 and a["mapq_hist"][255] == 1
    assert a["qual_hist"][127] == 6 and a["qual_hist"][126] == 2 and a["qual_hist"][33] == 0 and a["contig_unmapped"][n_contigs - 1] == 1
    qc = Qc(lib, h)
    try:
        assert qc.add_records(bam) == 0
        got = qc.state()
        assert got == want, diff_states(got, want)
        check_reports(qc, want, contigs)
        assert qc.add_records(bam) == 0 and qc.state() == add_states(want, want), "a second add doubles the sums and keeps the extremes"
        assert qc.add_records(b"") == 0 and qc.state() == add_states(want, want)
    finally:
        qc.free()
    return bam, want


def diff_states(got, want):
    out = [(n, got["counts"][n], want["counts"][n]) for n in want["counts"] if got["counts"][n] != want["counts"][n]]
    for n in ARRAYS:
        out += [(n, k, x, y) for k, (x, y) in enumerate(zip(got["arrays"][n], want["arrays"][n])) if x != y][:5]
    return out[:20]


# ------------------------------------------------------------------------------------------ test 2: random records
RANDOM_SIZES = [0, 1, 63, 64, 65, 257, TILE + 1]
READ_LENGTHS = [0, 1, 7, 150, 1001]
TLENS = [0, 0, 1, -1, 150, 300, -300, 301, 450, -450, 1023, 1024, -1025, 16382, 16383, -16384, 100000, -2 ** 31, 2 ** 31 - 1]


def random_records(n, seed, one_contig, n_contigs):
    """n records with seeded flags over all 12 bits; one_contig: all on contig 0 (the contention path), else spread over every
    contig and -1"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        l_seq = READ_LENGTHS[int(rng.choice(5, p=[0.05, 0.1, 0.25, 0.58, 0.02]))]
        refid = 0 if one_contig else int(rng.integers(-1, n_contigs))
        nrid = refid if rng.random() < 0.8 else int(rng.integers(-1, n_contigs))
        ops = ""
        if l_seq:
            s = int(rng.integers(0, min(3, l_seq)))
            m = l_seq - s
            ops = ("%dS" % s if s else "")
            if m >= 3 and rng.random() < 0.3:
                ops += "%dM%d%s%dM" % (1, int(rng.integers(1, 4)), "D" if rng.random() < 0.5 else "N", m - 1)
            elif m >= 3 and rng.random() < 0.3:
                ops += "1M1I%dM" % (m - 2)
            else:
                ops += "%dM" % m
        if rng.random() < 0.1:
            ops = ""
        u = rng.random()
        qual = 0xff if u < 0.1 else rng.integers(0, 200 if u < 0.2 else 45, size=l_seq, dtype=np.uint8).tobytes()
        aux = [b"", nm_aux("C", int(rng.integers(0, 256))), nm_aux("c", int(rng.integers(-128, 128))), nm_aux("S", int(rng.integers(0, 65536))),
               nm_aux("i", int(rng.integers(-1000, 100000))), RG_AUX + nm_aux("C", 3), nm_aux("C", 4) + RG_AUX][int(rng.integers(0, 7))]
        pos = int(rng.integers(0, 5000))
        out.append(qrec(b"x%d" % k, int(rng.integers(0, 4096)), refid, pos, ops, qual, l_seq=l_seq, nrid=nrid, npos=pos + int(rng.integers(-200, 200)),
                        mapq=int(rng.choice([0, 0, 4, 5, 60, 255, int(rng.integers(0, 256))])), tlen=TLENS[int(rng.integers(0, len(TLENS)))], aux=aux))
    return out


def check_random_sets(lib, h, n_contigs, one_contig, sizes=RANDOM_SIZES):
    sets = []
    for n in sizes:
        recs = random_records(n, 1000 + n + (7 if one_contig else 0), one_contig, n_contigs)
        bam = b"".join(recs)
        want = qc_py(bam, n_contigs)
        whole, halves, shuffled = Qc(lib, h), Qc(lib, h), Qc(lib, h)
        try:
            assert whole.add_records(bam) == 0
            got = whole.state()
            assert got == want, (n, one_contig, diff_states(got, want))
            assert halves.add_records(b"".join(recs[:n // 2])) == 0 and halves.add_records(b"".join(recs[n // 2:])) == 0
            assert halves.state() == want and halves.serialize() == whole.serialize(), (n, "two halves")
            order = np.random.default_rng(n).permutation(n)
            assert shuffled.add_records(b"".join(recs[i] for i in order)) == 0 and shuffled.serialize() == whole.serialize(), (n, "shuffled")
        finally:
            whole.free(), halves.free(), shuffled.free()
        sets.append((bam, want))
    if sizes == RANDOM_SIZES:
        big = sets[-1][1]
        assert all(big["counts"][p][0] > 0 and big["counts"][p][1] > 0 for p in PAIRS), "a flagstat line is never taken"
        assert all(sum(big["arrays"][k]) > 0 for k in ("isize_fr", "isize_rf", "isize_tandem")) and big["counts"]["max_length"] == 1001
        assert big["counts"]["records_without_nm"] > 0 and big["counts"]["mismatches"] > 0 and (one_contig or min(big["arrays"]["contig_mapped"]) > 0)
    return sets


# ------------------------------------------------------------------------------------------ test 3: end to end
def one_call_qc(lib, h, opts, pes, t1, t2, tmpdir, tag, qc, closed_fd=False, **kw):
    """bwamem_hip_fastq_to_bam_qc (qc: a Qc or None) -> (return code, the BAM bytes, the BAI bytes)"""
    d = bindqc(lib)
    ob = ctypes.create_string_buffer(bytes(opts), B.OPT_SIZE)
    pb = ctypes.create_string_buffer(pes, len(pes)) if pes is not None else None
    o = BamOptions(size=ctypes.sizeof(BamOptions), **kw)
    path, bpath = os.path.join(tmpdir, tag + ".bam"), os.path.join(tmpdir, tag + ".bai")
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    fb = os.open(bpath, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644) if kw.get("sort") else -1
    if closed_fd:
        os.close(fd)
    try:
        rc = d.bwamem_hip_fastq_to_bam_qc(h, ob, pb, t1, len(t1), t2, len(t2) if t2 is not None else 0, ctypes.byref(o), fd, fb, None, qc.q if qc is not None else None)
    finally:
        if not closed_fd:
            os.close(fd)
        if fb >= 0:
            os.close(fb)
    return rc, open(path, "rb").read(), open(bpath, "rb").read() if fb >= 0 else None


def batch_stages(lib, h, opts, paired, pes, t1, n_contigs):
    """one FASTQ batch: the accumulator after encode, after mark and after sort, each against qc_py of the downloaded bytes
    -> the state after mark, its serialized form"""
    d = bindqc(lib)
    b, bad = upload(lib, h, t1, None)
    assert b, bad
    bt = Batch(lib, h, opts, None, pes, b=b)
    qs = [Qc(lib, h) for _ in range(3)]
    try:
        plain = bt.encode(paired)
        assert qs[0].add_batch(bt.b) == 0 and qs[0].state() == qc_py(plain, n_contigs)
        assert d.bwamem_hip_batch_mark_duplicates(bt.b, 1 if paired else 0, None) == 0
        marked = bt.download()
        want = qc_py(marked, n_contigs)
        assert qs[1].add_batch(bt.b) == 0
        got = qs[1].state()
        assert got == want, diff_states(got, want)
        assert sum(want["counts"]["primary_duplicates"]) > 0 and qs[0].state()["counts"]["primary_duplicates"] == (0, 0)
        assert sum(want["arrays"]["qual_hist"]) == want["counts"]["total_length"] > 0, "with base qualities qual_hist sums to the bases"
        assert d.bwamem_hip_batch_sort_bam(bt.b) == 0
        srt = bt.download()
        assert srt != marked and qs[2].add_batch(bt.b) == 0
        assert qs[2].state() == qc_py(srt, n_contigs) == want and qs[2].serialize() == qs[1].serialize(), "the sorted layout gives the same block"
        return want, qs[1].serialize()
    finally:
        bt.free()
        for q in qs:
            q.free()


def check_end_to_end(lib, h, seqs, tmpdir):
    contigs = contigs_of(seqs)
    out = []
    for name, opts, paired, pes, src in end_to_end_sets(lib, seqs)[:2]:        # single-end, interleaved pairs: the planted-duplicate batches
        t1 = src["t1"]
        want, blob = batch_stages(lib, h, opts, paired, pes, t1, len(contigs))
        if paired:
            assert sum(want["arrays"]["isize_fr"]) > 0 and want["counts"]["properly_paired"][0] > 0
        kw = dict(sort=1, mark_dup=1, write_header=1)
        for tag, text in (("plain", t1), ("bgzf", bgzf_cut(t1, 4096))):
            qc = Qc(lib, h)
            try:
                rc, bam, bai = one_call_qc(lib, h, opts, pes, text, None, tmpdir, tag, qc, **kw)
                assert rc == 0 and qc.state() == want and qc.serialize() == blob, (name, tag)
                rc0, bam0, bai0 = one_call_qc(lib, h, opts, pes, text, None, tmpdir, tag + "0", None, **kw)
                assert rc0 == 0 and bam0 == bam and bai0 == bai and len(bam) > 28 and len(bai) > 8, (name, tag)
                check_reports(qc, want, contigs)
            finally:
                qc.free()
        out.append((want, blob))
    return out


# ------------------------------------------------------------------------------------------ test 4: reports of special accumulators
def check_report_edges(lib, h, contigs):
    qc = Qc(lib, h)
    try:
        empty = qc_py(b"", len(contigs))
        assert qc.state() == empty and empty["counts"]["isize_min"] == (U32_MAX,) * 3
        check_reports(qc, empty, contigs)
        assert qc.report(FLAGSTAT).count("(N/A : N/A)") == 4 and qc.report(SUMMARY).count("\tN/A\n") == 4
        assert qc.report(INSERT_SIZE) == ISIZE_HEADER + "\ninsert_size\tFR\tRF\tTANDEM\n"
        assert qc.report(IDXSTATS).splitlines()[-1] == "*\t0\t0\t0" and len(qc.report(IDXSTATS).splitlines()) == len(contigs) + 1
        pair = dict(refid=0, pos=1000, cigar="50M", nrid=0, npos=1200, aux=nm_aux("C", 1))
        bam = b"".join(qrec(b"e%d" % t, 1 | 0x40 | 0x20, tlen=t, **pair) for t in (100, 101, 103, 110))
        assert qc.add_records(bam) == 0
        st = qc_py(bam, len(contigs))
        check_reports(qc, st, contigs)
        line = qc.report(INSERT_SIZE).splitlines()[1].split("\t")
        assert line[:6] == ["FR", "4", "100", "110", "102.0", "1.5"], line         # an even count: the mean of 101 and 103; deviations 2 1 1 8
        far = qrec(b"far", 1 | 0x40 | 0x20, tlen=5000, **pair)
        assert qc.add_records(far) == 0
        line = qc.report(INSERT_SIZE).splitlines()[1].split("\t")
        assert line[:6] == ["FR", "5", "100", "5000", "103.0", "3.0"] and math.isclose(float(line[6]), 103.5, rel_tol=1e-9), "deviations 3 2 0 7 4897; 5000 lies beyond median + 10 MAD"
        check_reports(qc, add_states(st, qc_py(far, len(contigs))), contigs)
        bam = b"".join(qrec(b"h%d" % t, 1 | 0x40 | 0x20, tlen=t, **pair) for t in (200, 201))
        q2 = Qc(lib, h)
        try:
            assert q2.add_records(bam) == 0 and q2.report(INSERT_SIZE).splitlines()[1].split("\t")[4:6] == ["200.5", "0.5"]
        finally:
            q2.free()
    finally:
        qc.free()


# ------------------------------------------------------------------------------------------ test 5: errors and state
def check_errors_and_state(lib, h, seqs, tmpdir, other_img):
    d = bindqc(lib)
    n_contigs = len(seqs)
    good = hand_records(n_contigs)
    qc = Qc(lib, h)
    try:
        assert qc.add_records(b"".join(good)) == 0
        before = qc.serialize()
        bam = b"".join(good)
        overrun = bytearray(bam)
        struct.pack_into("<i", overrun, 0, len(bam))
        short = bytearray(bam)
        struct.pack_into("<i", short, 0, 20)
        neg = bytearray(bam)
        struct.pack_into("<i", neg, 20, -1)
        long_seq = bytearray(bam)
        struct.pack_into("<i", long_seq, 20, 1000)
        late = bytearray(bam)
        struct.pack_into("<i", late, len(bam) - len(good[-1]) + 20, -1)                 # (the last record: another workgroup's lane)
        contig = bytearray(bam)
        struct.pack_into("<i", contig, 4, n_contigs)
        for name, bad in (("truncated", bam[:-5]), ("cut inside the fixed fields", bam[:len(good[0]) + 30]), ("block_size overruns", overrun), ("block_size 20", short),
                          ("l_seq -1", neg), ("l_seq beyond the record", long_seq), ("l_seq -1 in the last record", late), ("refID = n_contigs", contig)):
            assert qc.add_records(bytes(bad)) != 0, name
            assert qc.serialize() == before, name
        # blobs of another index and of another version
        ho = lib.open_index(other_img)
        other = Qc(lib, ho)
        try:
            assert qc.add_serialized(other.serialize()) != 0 and qc.serialize() == before, "a blob of another n_contigs"
        finally:
            other.free()
            lib.destroy_index(ho)
        bad = bytearray(before)
        bad[8] ^= 1
        assert qc.add_serialized(bytes(bad)) != 0 and qc.add_serialized(before[:-8]) != 0 and qc.add_serialized(before[:16]) != 0 and qc.serialize() == before
        twice = Qc(lib, h)
        try:
            assert twice.add_serialized(before) == 0 and twice.serialize() == before and twice.add_serialized(before) == 0
            assert qc.add_records(bam) == 0 and qc.serialize() == twice.serialize(), "adding a blob is adding its records"
        finally:
            twice.free()
        before = qc.serialize()
        # a batch without encoded records, and the one-call entry point failing after the reduction
        reads, names, quals = planted_single(seqs)
        t1 = fastq_text(reads, names, quals)
        b, bad_rec = upload(lib, h, t1, None)
        assert b
        bt = Batch(lib, h, lib.default_options(), None, b=b)
        try:
            assert qc.add_batch(bt.b) != 0 and qc.serialize() == before, "add_batch before encode"
        finally:
            bt.free()
        assert qc.add_batch(None) != 0
        rc, _, _ = one_call_qc(lib, h, lib.default_options(), None, t1, None, tmpdir, "closed", qc, closed_fd=True, sort=0, mark_dup=1, write_header=1)
        assert rc != 0 and qc.serialize() == before, "a call that fails at the write leaves qc untouched"
        rc, _, _ = one_call_qc(lib, h, lib.default_options(), None, b"@r\nACGT\n+\n", None, tmpdir, "malformed", qc, sort=0, mark_dup=0, write_header=1)
        assert rc != 0 and qc.serialize() == before
    finally:
        qc.free()
    assert d.bwamem_hip_qc_counts(None, None) != 0 and d.bwamem_hip_qc_create(None) is None


# ------------------------------------------------------------------------------------------ CPU suite (emulation build)
@pytest.fixture(scope="module")
def emu_index(small_genome, tmp_path_factory):
    B.build_emu()
    emu = B.product_lib(emu=True)
    seqs, img = small_genome
    h = emu.open_index(img)
    before = untouched_bytes(emu, h, seqs, str(tmp_path_factory.mktemp("before")))     # (test 6: before any QC object exists in this module)
    yield emu, h, seqs, before
    emu.destroy_index(h)


def test_qc_hand_made_records(emu_index):
    emu, h, seqs, _ = emu_index
    check_hand_records(emu, h, contigs_of(seqs))


@pytest.mark.parametrize("one_contig", [True, False], ids=["one-contig", "every-contig"])
def test_qc_random_records_against_the_checker(emu_index, alt_genome, one_contig):
    emu, h, seqs, _ = emu_index
    if one_contig:
        check_random_sets(emu, h, len(seqs), True)
        return
    alt_seqs, img = alt_genome[0], alt_genome[1]
    ha = emu.open_index(img)
    try:
        assert len(alt_seqs) != len(seqs)
        check_random_sets(emu, ha, len(alt_seqs), False)
    finally:
        emu.destroy_index(ha)


def test_qc_end_to_end_planted_duplicates(emu_index, tmp_path):
    emu, h, seqs, _ = emu_index
    check_end_to_end(emu, h, seqs, str(tmp_path))


def test_qc_reports(emu_index):
    emu, h, seqs, _ = emu_index
    check_report_edges(emu, h, contigs_of(seqs))


def test_qc_errors_and_state(emu_index, alt_genome, tmp_path):
    emu, h, seqs, _ = emu_index
    check_errors_and_state(emu, h, seqs, str(tmp_path), alt_genome[1])


def test_qc_earlier_calls_untouched(emu_index, tmp_path):
    """test 6: after QC objects have existed and taken batches in the process, the bytes of the calls that existed before are what
    they were"""
    emu, h, seqs, before = emu_index
    qc = Qc(emu, h)
    try:
        name, opts, paired, pes, src = end_to_end_sets(emu, seqs)[0]
        assert one_call_qc(emu, h, opts, pes, src["t1"], None, str(tmp_path), "q", qc, sort=1, mark_dup=1, write_header=1)[0] == 0
        assert qc.state()["counts"]["total"][0] > 0
    finally:
        qc.free()
    assert untouched_bytes(emu, h, seqs, str(tmp_path)) == before


def test_qc_python_mirror(emu_index, small_genome, tmp_path):
    """BwaMemAligner.newQc() and the qc= argument of alignFastqToBam / alignSeqsToBam over the emulation build, in a child process"""
    emu, h, seqs, _ = emu_index
    _, img = small_genome
    reads, names, quals = planted_single(seqs)
    fq = str(tmp_path / "in.fq")
    with open(fq, "wb") as f:
        f.write(fastq_text(reads, names, quals))
    p = {k: str(tmp_path / k) for k in ("a.bam", "a.bam.bai", "b.bam", "c.bam", "plain.bam")}
    r = subprocess.run([sys.executable, "-c", (
        "import sys; sys.path.insert(0, %r); import bwamem\n"
        "ix = bwamem.BwaMemIndex(%r); al = bwamem.BwaMemAligner(ix)\n"
        "reads, p, fq = %r, %r, %r\n"
        "a, b, both = al.newQc(), al.newQc(), al.newQc()\n"
        "al.alignFastqToBam(fq, p['a.bam'], sort=True, index_path=p['a.bam.bai'], mark_duplicates=True, qc=a)\n"
        "al.alignSeqsToBam(reads, p['b.bam'], device=True, qc=b)\n"
        "al.alignFastqToBam(fq, p['c.bam'], sort=True, mark_duplicates=True, qc=both); al.alignSeqsToBam(reads, p['c.bam'], device=True, qc=both)\n"
        "al.alignSeqsToBam(reads, p['plain.bam'], device=True)\n"
        "print('A', sorted(a.counts().items())); print('B', sorted(b.counts().items()))\n"
        "print('ARR', a.array('qual_hist'), a.array('contig_mapped'))\n"
        "blob = both.serialize(); a.add(b.serialize()); print('SUM', a.serialize() == blob, a.counts() == both.counts())\n"
        "print('TEXT', repr(a.flagstat()), repr(a.idxstats()), len(a.summary()), len(a.insertSizeMetrics()))\n"
        "cb = b.counts()\n"
        "try:\n    al.alignSeqsToBam(reads, p['c.bam'] + 'x', qc=b)\nexcept ValueError:\n    print('host-framing-refused', 'kept' if b.counts() == cb else 'changed')\n"
        "try:\n    a.array('nope')\nexcept ValueError:\n    print('unknown-array')\n"
        "a.close(); b.close(); both.close(); al.close(); ix.close()\n") % (B.PKG, img, reads, p, fq)],
        env=dict(os.environ, LIBBWA_PATH=B.EMU_LIB), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "host-framing-refused kept" in r.stdout and "unknown-array" in r.stdout and "SUM True True" in r.stdout, (r.stdout[-1500:], r.stderr[-2000:])
    assert not os.path.exists(p["c.bam"] + "x")
    assert open(p["b.bam"], "rb").read() == open(p["plain.bam"], "rb").read(), "qc= does not change the file"
    opts = emu.default_options()
    contigs = contigs_of(seqs)
    want_a, _ = batch_stages(emu, h, opts, False, None, fastq_text(reads, names, quals), len(contigs))
    bt = Batch(emu, h, opts, B.pack_request(reads))
    try:
        want_b = qc_py(bt.encode(False), len(contigs))
    finally:
        bt.free()
    lines = dict(ln.split(" ", 1) for ln in r.stdout.splitlines() if ln.split(" ", 1)[0] in ("A", "B", "ARR", "TEXT"))
    assert lines["A"] == str(sorted(want_a["counts"].items())) and lines["B"] == str(sorted(want_b["counts"].items()))
    assert lines["ARR"] == "%s %s" % (want_a["arrays"]["qual_hist"], want_a["arrays"]["contig_mapped"])
    texts = reports_py(add_states(want_a, want_b), contigs)
    assert lines["TEXT"].startswith("%r %r " % (texts[0], texts[1]))


def _gather_worker(rank, world, port, img, n_contigs, q):
    os.environ["LIBBWA_PATH"] = B.EMU_LIB                              # (read by bwamem when it is imported)
    sys.path.insert(0, B.PKG)
    import torch.distributed as dist
    import bwamem
    import sharding
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    ix = bwamem.BwaMemIndex(img)
    qc = bwamem.BwaMemAligner(ix).newQc()
    bam = rank_records(rank, n_contigs)
    assert bwamem._lib.bwamem_hip_qc_add_records_device(qc._ptr(), bam, len(bam)) == 0
    got = sharding.gather_qc(dist, qc)
    if rank == 0:
        q.put(dict(counts=got.counts(), arrays={n: got.array(n) for n in ARRAYS}))
    else:
        assert got is None
    dist.barrier()
    qc.close()
    ix.close()
    dist.destroy_process_group()


def rank_records(rank, n_contigs):
    return b"".join(hand_records(n_contigs)) if rank == 0 else b"".join(random_records(300, 40 + rank, False, n_contigs))


def test_qc_gathered_over_two_ranks(emu_index, small_genome):
    """sharding.gather_qc: two gloo ranks reduce record sets of their own; rank 0 ends up with the accumulator of both"""
    import torch.multiprocessing as mp
    _, _, seqs, _ = emu_index
    _, img = small_genome
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33500 + os.getpid() % 2000
    procs = [ctx.Process(target=_gather_worker, args=(r, 2, port, img, len(seqs), q)) for r in range(2)]
    for p in procs:
        p.start()
    got = q.get(timeout=300)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = add_states(qc_py(rank_records(0, len(seqs)), len(seqs)), qc_py(rank_records(1, len(seqs)), len(seqs)))
    assert got == want, diff_states(got, want)


def state_words(st):
    """a state as the 64-bit words the sanitizer driver compares: the counters in struct order, then the arrays in BWAMEM_HIP_QC_* order"""
    c = st["counts"]
    w = [x for n in PAIRS for x in c[n]] + [c[n] for n in SINGLES] + list(c["isize_min"]) + list(c["isize_max"])
    for n in ARRAYS:
        w += st["arrays"][n]
    return struct.pack("<%dQ" % len(w), *w)


def test_qc_sanitizers(emu_index, small_genome, tmp_path):
    """the QC calls under AddressSanitizer + UBSan: a stand-alone driver (tests/bam_qc_sanitized_driver.cpp), compiled here with the
    sanitizers and linked against the sanitized emulation build (tests/emu `make asan`), run as a program.  It compares what the
    accumulator holds with the checker's words, written here, for the record sets of tests 1, 2 and 5."""
    B.make(os.path.join(B.ROOT, "tests", "emu"), "asan")
    seqs, img = small_genome
    n_contigs = len(seqs)
    manifest = []

    def add(kind, tag, bam):
        with open(str(tmp_path / (tag + ".bam")), "wb") as f:
            f.write(bam)
        if kind == "rec":
            with open(str(tmp_path / (tag + ".want")), "wb") as f:
                f.write(state_words(qc_py(bam, n_contigs)))
        manifest.append("%s %s" % (kind, tag))
    good = b"".join(hand_records(n_contigs))
    add("rec", "hand", good)
    for k, (n, one) in enumerate(((0, True), (1, True), (65, False), (257, True), (TILE + 1, False))):
        add("rec", "rand%d" % k, b"".join(random_records(n, 2000 + k, one, n_contigs)))
    neg, contig = bytearray(good), bytearray(good)
    struct.pack_into("<i", neg, 20, -1)
    struct.pack_into("<i", contig, 4, n_contigs)
    for k, bad in enumerate((good[:-5], good[:30], bytes(neg), bytes(contig))):
        add("bad", "bad%d" % k, bad)
    with open(str(tmp_path / "manifest.txt"), "w") as f:
        f.write("\n".join(manifest) + "\n")
    emu_dir = os.path.join(B.ROOT, "tests", "emu", "_build")
    exe = str(tmp_path / "bam_qc_sanitized_driver")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(B.ROOT, "include"), os.path.join(B.ROOT, "tests", "bam_qc_sanitized_driver.cpp"), "-o", exe,
                    "-L", emu_dir, "-lbwamem_emu_asan", "-Wl,-rpath," + emu_dir], check=True)
    r = subprocess.run([exe, img, str(tmp_path)], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0"),
                       capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "sanitized-ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


# ------------------------------------------------------------------------------------------ GPU suite
@pytest.mark.gpu
def test_gpu_qc_small_cases(hip_lib, small_genome, alt_genome, tmp_path):
    """test 9: tests 1-5 on the device"""
    seqs, img = small_genome
    h = hip_lib.open_index(img)
    ha = hip_lib.open_index(alt_genome[1])
    try:
        contigs = contigs_of(seqs)
        check_hand_records(hip_lib, h, contigs)
        check_random_sets(hip_lib, h, len(seqs), True)
        check_random_sets(hip_lib, ha, len(alt_genome[0]), False)
        check_end_to_end(hip_lib, h, seqs, str(tmp_path))
        check_report_edges(hip_lib, h, contigs)
        check_errors_and_state(hip_lib, h, seqs, str(tmp_path), alt_genome[1])
    finally:
        hip_lib.destroy_index(h)
        hip_lib.destroy_index(ha)


def check_batch_before_and_after_sort(lib, h, n_contigs, opts, paired, reads, quals):
    d = bindqc(lib)
    bt = Batch(lib, h, opts, B.pack_request(reads), PES if paired else None)
    a, b = Qc(lib, h), Qc(lib, h)
    try:
        assert bt.set_quals(quals) == 0
        bt.encode(paired)
        assert d.bwamem_hip_batch_mark_duplicates(bt.b, 1 if paired else 0, None) == 0
        want = qc_py(bt.download(), n_contigs)
        assert a.add_batch(bt.b) == 0
        got = a.state()
        assert got == want, diff_states(got, want)
        assert d.bwamem_hip_batch_sort_bam(bt.b) == 0 and b.add_batch(bt.b) == 0 and b.serialize() == a.serialize()
        return want
    finally:
        bt.free()
        a.free(), b.free()


@pytest.mark.gpu
def test_gpu_qc_medium_single_and_paired(hip_lib, medium_genome):
    """one medium-genome batch, single-end and paired-end, at TILE + 1 reads with every tenth template repeated: more than one
    workgroup per kernel, duplicates, insert sizes around 400"""
    seqs, img = medium_genome
    h = hip_lib.open_index(img)
    try:
        n = TILE + 1
        reads = B.simulate_reads(seqs, n * 10 // 11, length=150, seed=21, sub=0.02, indel=0.003)
        pairs = B.simulate_pairs(seqs, n * 10 // 22 + 1, length=150, seed=22, ins_mean=400, ins_sd=40)
        po = B.set_opt(hip_lib.default_options(), flag=B.MEM_F_PE)
        for rd, paired, opts, step in ((reads, False, hip_lib.default_options(), 1), (pairs, True, po, 2)):
            rd = repeat_every_tenth(rd, step)
            assert len(rd) >= n
            want = check_batch_before_and_after_sort(hip_lib, h, len(seqs), opts, paired, rd, quals_blob(seeded_quals(rd, 23)))
            c = want["counts"]
            assert c["total"][0] >= len(rd) - 2 and sum(c["primary_duplicates"]) >= len(rd) // step // 11 * 0.9 * step
            assert sum(want["arrays"]["qual_hist"]) == c["total_length"] and c["mismatches"] > 0 and c["records_without_nm"] == 0
            if paired:
                n_fr, median = isize_stats(want["arrays"]["isize_fr"])[:2]
                assert n_fr > len(rd) // 4 and 380 <= median <= 420, "the simulated inserts are 400 +- 40"
    finally:
        hip_lib.destroy_index(h)


@pytest.mark.gpu
def test_gpu_qc_long_reads(hip_lib, medium_genome):
    """a few 2 kb reads: max_length > 1000, so QUAL is read by a wavefront per read"""
    seqs, img = medium_genome
    h = hip_lib.open_index(img)
    try:
        reads = B.simulate_reads(seqs, 12, length=2000, seed=41, sub=0.03, indel=0.005) + [b"ACGT" * 300, b"A" * 7]
        want = check_batch_before_and_after_sort(hip_lib, h, len(seqs), hip_lib.default_options(), False, reads, quals_blob(seeded_quals(reads, 42)))
        assert want["counts"]["max_length"] == 2000 and sum(want["arrays"]["qual_hist"]) == want["counts"]["total_length"] >= 12 * 2000
    finally:
        hip_lib.destroy_index(h)


@pytest.mark.gpu
def test_gpu_qc_equals_emulation(hip_lib, small_genome):
    """the device's serialized accumulator is the emulation build's for the same records"""
    B.build_emu()
    emu = B.product_lib(emu=True)
    seqs, img = small_genome
    h, he = hip_lib.open_index(img), emu.open_index(img)
    try:
        sets = [b"".join(hand_records(len(seqs)))] + [b"".join(random_records(n, 3000 + n, n % 2 == 0, len(seqs))) for n in (65, 257, 1500)]
        for bam in sets:
            a, b = Qc(hip_lib, h), Qc(emu, he)
            try:
                assert a.add_records(bam) == 0 and b.add_records(bam) == 0 and a.serialize() == b.serialize()
            finally:
                a.free(), b.free()
    finally:
        hip_lib.destroy_index(h)
        emu.destroy_index(he)
