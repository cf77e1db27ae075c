"""Rate of alignment QC on the device next to the steps around it, on the batches of markdup_rate.py (the same
generator and seed: 10 % of the templates repeated, seeded base qualities): for a single-end and a paired-end batch resident in HBM
it times, in one process, bwamem_hip_batch_encode_bam, _mark_duplicates, bwamem_hip_qc_add_batch on the marked records (grouped by
read), _sort_bam, and bwamem_hip_qc_add_batch again on the sorted records, each by HIP events and by the host clock.  Every figure is
the median of --reps runs after one warm-up run of the same shape.  In the same run the accumulator is compared, once, with the rule of
csrc/bam_qc.h restated in Python (qc_py below), and the blocks before and after the sort with each other.  Two conditions, both
relative and measured here: (i) _qc_add_batch takes no longer than _mark_duplicates of the same batch; (ii) with no QC object,
_encode_bam, _mark_duplicates, _sort_bam and the marked file call are within the run-to-run spread of the parent commit's library
(--parent-lib), timed alternately in this process.  Kernel times proper: run under rocprofv3 --kernel-trace --stats with --skip-files
and --skip-check, in a run of its own.  Needs a GPU; there is no fallback.
usage: bam_qc_rate.py [--reads N] [--pairs N] [--genome-bp N] [--reps K] [--out FILE.json] [--skip-files] [--skip-check] [--parent-lib LIB.so]"""
import argparse
import collections
import ctypes
import json
import os
import statistics
import struct
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bam_rate as R  # noqa: E402  (the batch generator, the event timer)
import markdup_rate as M  # noqa: E402  (the bindings of the steps around)
from sort_rate import both  # noqa: E402
B = R.B

PAIRS = ["total", "primary", "secondary", "supplementary", "duplicates", "primary_duplicates", "mapped", "primary_mapped", "paired", "read1", "read2",
         "properly_paired", "both_mapped", "singletons", "mate_diff_chr", "mate_diff_chr_mapq5"]
SINGLES = ["unplaced", "sequences", "total_length", "max_length", "reads_mq0", "bases_mapped", "bases_mapped_cigar", "bases_soft_clipped", "ins_events", "ins_bases",
           "del_events", "del_bases", "mismatches", "records_without_nm"]
ARRAY_LEN = [256, 128, 16384, 16384, 16384, None, None]              # BWAMEM_HIP_QC_*; None: n_contigs


def qc_py(bam, n_contigs):
    """the rule at the top of csrc/bam_qc.h -> the 64-bit words of bwamem_qc_counts_t followed by the seven arrays"""
    flag = [[0, 0] for _ in PAIRS]
    one = dict.fromkeys(SINGLES, 0)
    mapq_hist, isize, contig = [0] * 256, [collections.Counter() for _ in range(3)], [[0] * n_contigs, [0] * n_contigs]
    imin, imax, quals = [0xffffffff] * 3, [0] * 3, []
    off, n = 0, len(bam)
    int_fmt = {99: "<b", 67: "<B", 115: "<h", 83: "<H", 105: "<i", 73: "<I"}
    while off < n:
        size, refid, pos, l_name, mapq, _, n_cig, f, l_seq, nrid, npos, tlen = struct.unpack_from("<iiiBBHHHiiii", bam, off)
        w = 1 if f & 0x200 else 0
        mapped, primary = not f & 4, not f & 0x900
        took = [0]
        if f & 0x100:
            took.append(2)
        elif f & 0x800:
            took.append(3)
        else:
            took.append(1)
            if mapped:
                took.append(7)
            if f & 0x400:
                took.append(5)
            if f & 1:
                took.append(8)
                if f & 2 and mapped:
                    took.append(11)
                if f & 0x40:
                    took.append(9)
                if f & 0x80:
                    took.append(10)
                if f & 8 and mapped:
                    took.append(13)
                if mapped and not f & 8:
                    took.append(12)
                    if refid != nrid:
                        took.append(14)
                        if mapq >= 5:
                            took.append(15)
        if mapped:
            took.append(6)
        if f & 0x400:
            took.append(4)
        for k in took:
            flag[k][w] += 1
        if refid < 0:
            one["unplaced"] += 1
        else:
            contig[0 if mapped else 1][refid] += 1
        q = off + 36 + l_name + 4 * n_cig + (l_seq + 1) // 2
        span = 0
        if primary:
            one["sequences"] += 1
            one["total_length"] += l_seq
            one["max_length"] = max(one["max_length"], l_seq)
            if l_seq and bam[q] != 0xff:
                quals.append(bam[q:q + l_seq])
        if primary and mapped:
            one["reads_mq0"] += mapq == 0
            one["bases_mapped"] += l_seq
            for c in struct.unpack_from("<%dI" % n_cig, bam, off + 36 + l_name):
                op, ln = c & 15, c >> 4
                if op in (0, 7, 8):
                    one["bases_mapped_cigar"] += ln; span += ln
                elif op == 1:
                    one["bases_mapped_cigar"] += ln; one["ins_events"] += 1; one["ins_bases"] += ln
                elif op == 2:
                    one["del_events"] += 1; one["del_bases"] += ln; span += ln
                elif op == 3:
                    span += ln
                elif op == 4:
                    one["bases_soft_clipped"] += ln
            a = q + l_seq
            if a + 3 <= off + 4 + size and bam[a:a + 2] == b"NM" and bam[a + 2] in int_fmt:
                one["mismatches"] += max(struct.unpack_from(int_fmt[bam[a + 2]], bam, a + 3)[0], 0)
            else:
                one["records_without_nm"] += 1
            mapq_hist[mapq] += 1
            if f & 1 and f & 0x40 and not f & 0xD0C and refid == nrid and tlen != 0:
                x = abs(tlen)
                o = 2 if bool(f & 0x10) == bool(f & 0x20) else (0 if tlen > 0 else 1) if not f & 0x10 else 0 if npos + 1 < pos + span else 1
                isize[o][min(x, 16383)] += 1
                imin[o], imax[o] = min(imin[o], x), max(imax[o], x)
        off += 4 + size
    qual_hist = np.bincount(np.minimum(np.frombuffer(b"".join(quals), dtype=np.uint8), 127), minlength=128).tolist() if quals else [0] * 128
    words = [x for p in flag for x in p] + [one[k] for k in SINGLES] + imin + imax + mapq_hist + qual_hist
    for o in range(3):
        words += [isize[o][v] for v in range(16384)]
    return words + contig[0] + contig[1]


class QcCounts(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64 * 2) for n in PAIRS] + [(n, ctypes.c_uint64) for n in SINGLES] + [("isize_min", ctypes.c_uint64 * 3), ("isize_max", ctypes.c_uint64 * 3)]


def words_of(d, q, n_contigs):
    c = QcCounts()
    assert d.bwamem_hip_qc_counts(q, ctypes.byref(c)) == 0
    words = list(np.frombuffer(bytes(c), dtype=np.uint64))
    for which, n in enumerate(ARRAY_LEN):
        buf = (ctypes.c_uint64 * (n or n_contigs))()
        assert d.bwamem_hip_qc_array(q, which, buf, len(buf)) == len(buf)
        words += list(buf)
    return [int(x) for x in words]


def measure(lib, d, ev, h, parent, req, quals, n_reads, n_contigs, paired, reps, skip_files, skip_check):
    opts = B.set_opt(lib.default_options(), flag=B.MEM_F_PE if paired else 0)
    ob = ctypes.create_string_buffer(bytes(opts), B.OPT_SIZE)
    pe = 1 if paired else 0

    def batch(dd, hh):
        b = dd.bwamem_hip_batch_upload(hh, req, len(req))
        assert b and dd.bwamem_hip_batch_keep_offsets(b, 1) == 0 and dd.bwamem_hip_batch_set_qualities(b, quals, len(quals)) == 0
        return b
    b = batch(d, h)
    assert d.bwamem_hip_batch_align(h, ob, None, b, 0) == 0
    steps = ("encode", "mark", "qc_grouped", "sort", "qc_sorted")
    t = {k + "_" + c: [] for k in steps for c in ("events", "wall")}
    marked = blob_grouped = blob_sorted = got = None
    for rep in range(reps + 1):                                   # rep 0 warms every shape up
        qa, qb = d.bwamem_hip_qc_create(h), d.bwamem_hip_qc_create(h)
        assert qa and qb
        row = []
        rc, ms, wall = both(ev, lambda: d.bwamem_hip_batch_encode_bam(b, pe, None, None)); assert rc == 0; row += [ms, wall]
        rc, ms, wall = both(ev, lambda: d.bwamem_hip_batch_mark_duplicates(b, pe, None)); assert rc == 0; row += [ms, wall]
        m = d.bwamem_hip_batch_bam_bytes(b)
        if marked is None and not skip_check:
            marked = np.empty(m, dtype=np.uint8)
            assert d.bwamem_hip_batch_bam_download(b, marked.ctypes.data) == 0
        rc, ms, wall = both(ev, lambda: d.bwamem_hip_qc_add_batch(qa, b)); assert rc == 0; row += [ms, wall]
        rc, ms, wall = both(ev, lambda: d.bwamem_hip_batch_sort_bam(b)); assert rc == 0; row += [ms, wall]
        rc, ms, wall = both(ev, lambda: d.bwamem_hip_qc_add_batch(qb, b)); assert rc == 0; row += [ms, wall]
        if rep == 0:
            sz = ctypes.c_size_t()
            for q, name in ((qa, "grouped"), (qb, "sorted")):
                p = d.bwamem_hip_qc_serialize(q, ctypes.byref(sz))
                assert p
                if name == "grouped":
                    blob_grouped = ctypes.string_at(p, sz.value)
                else:
                    blob_sorted = ctypes.string_at(p, sz.value)
                lib._free(p)
            got = words_of(d, qa, n_contigs)
        else:
            for k, v in zip(t, row):
                t[k].append(v)
        d.bwamem_hip_qc_free(qa); d.bwamem_hip_qc_free(qb)
    assert blob_grouped == blob_sorted, "the block of the sorted records differs from that of the same records grouped by read"
    med = {k: statistics.median(v) for k, v in t.items()}
    out = dict(reads=n_reads, paired=paired, reps=reps, bam_bytes=int(m), records=got[0] + got[1], **{"ms_" + k: v for k, v in med.items()},
               qc_gb_per_s=dict(grouped=m / med["qc_grouped_events"] / 1e6, sorted=m / med["qc_sorted_events"] / 1e6),
               qc_within_mark=bool(max(med["qc_grouped_wall"], med["qc_sorted_wall"]) <= med["mark_wall"]), sorted_block_equals_grouped=True, all_runs_ms=t)
    if not skip_check:
        t0 = time.perf_counter()
        want = qc_py(marked.tobytes(), n_contigs)
        bad = [k for k, (x, y) in enumerate(zip(got, want)) if x != y]
        assert len(got) == len(want) and not bad, ("the accumulator is not the rule's", bad[:10])
        out["checked_against_python"] = True
        out["python_restatement_s"] = time.perf_counter() - t0
    # ---- (ii) no QC object: this build and the parent's, alternately, on batches of their own
    if parent:
        plib, pd, ph = parent
        pb = batch(pd, ph)
        assert pd.bwamem_hip_batch_align(ph, ob, None, pb, 0) == 0
        u = {k + s: [] for k in ("encode", "mark", "sort") for s in ("", "_parent")}
        for rep in range(reps + 1):
            for who in (("this", "parent"), ("parent", "this"))[rep & 1]:      # alternating: whichever runs second finds the device busy already
                dd, bb, sfx = (d, b, "") if who == "this" else (pd, pb, "_parent")
                rc, ms, _ = both(ev, lambda: dd.bwamem_hip_batch_encode_bam(bb, pe, None, None)); assert rc == 0
                rc1, ms1, _ = both(ev, lambda: dd.bwamem_hip_batch_mark_duplicates(bb, pe, None)); assert rc1 == 0
                rc2, ms2, _ = both(ev, lambda: dd.bwamem_hip_batch_sort_bam(bb)); assert rc2 == 0
                if rep:
                    u["encode" + sfx].append(ms); u["mark" + sfx].append(ms1); u["sort" + sfx].append(ms2)
        pd.bwamem_hip_batch_free(pb)
        for k in ("encode", "mark", "sort"):
            a, p = u[k], u[k + "_parent"]
            out["off_" + k] = dict(this_ms=statistics.median(a), parent_ms=statistics.median(p), spread_ms=dict(this=max(a) - min(a), parent=max(p) - min(p)),
                                   not_slower_than_parent=bool(statistics.median(a) - statistics.median(p) <= max(max(a) - min(a), max(p) - min(p))), runs=dict(this=a, parent=p))
    d.bwamem_hip_batch_free(b)
    if skip_files:
        return out
    with tempfile.TemporaryDirectory() as tmp:
        path, bpath = os.path.join(tmp, "out.bam"), os.path.join(tmp, "out.bam.bai")
        calls = [("file_marked_sorted_indexed", lambda fd, fb: d.bwamem_hip_align_to_marked_bam(h, ob, None, req, len(req), None, 1, fd, fb, 1, None))]
        if parent:
            calls.append(("file_marked_sorted_indexed_parent", lambda fd, fb: parent[1].bwamem_hip_align_to_marked_bam(parent[2], ob, None, req, len(req), None, 1, fd, fb, 1, None)))
        secs = {k: [] for k, _ in calls}
        for rep in range(reps + 1):
            for key, call in (calls if rep & 1 else calls[::-1]):
                fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
                fb = os.open(bpath, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
                t0 = time.perf_counter()
                rc = call(fd, fb)
                dt = time.perf_counter() - t0
                os.close(fd); os.close(fb)
                assert rc == 0
                if rep:
                    secs[key].append(dt)
        for key, v in secs.items():
            out[key] = dict(seconds=statistics.median(v), reads_per_s=n_reads / statistics.median(v), spread_s=max(v) - min(v), runs_s=v)
        if parent:
            a, p = out["file_marked_sorted_indexed"], out["file_marked_sorted_indexed_parent"]
            out["file_not_slower_than_parent"] = bool(a["seconds"] - p["seconds"] <= max(a["spread_s"], p["spread_s"]))
    return out


def bind(d):
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    M.bind(d)
    if hasattr(d, "bwamem_hip_qc_create"):
        d.bwamem_hip_qc_create.restype = vp; d.bwamem_hip_qc_create.argtypes = [vp]
        d.bwamem_hip_qc_free.restype = None; d.bwamem_hip_qc_free.argtypes = [vp]
        d.bwamem_hip_qc_add_batch.argtypes = [vp, vp]
        d.bwamem_hip_qc_counts.argtypes = [vp, ctypes.POINTER(QcCounts)]
        d.bwamem_hip_qc_array.restype = ctypes.c_int64; d.bwamem_hip_qc_array.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_uint64), sz]
        d.bwamem_hip_qc_serialize.restype = vp; d.bwamem_hip_qc_serialize.argtypes = [vp, ctypes.POINTER(sz)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--genome-bp", type=int, default=3_000_000, help="the suite's medium genome, as markdup_rate.py")
    ap.add_argument("--reps", type=int, default=4, help="even, so that the two orders of the parent comparison are timed equally often")
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-files", action="store_true", help="batch figures only (the profiler run)")
    ap.add_argument("--skip-check", action="store_true", help="do not compare the accumulator with the rule in Python (the profiler run)")
    ap.add_argument("--parent-lib", default=None, help="libbwamem_hip.so of the parent commit, timed in the same process")
    args = ap.parse_args()
    lib = B.product_lib()
    d = lib.dll
    d.bwamem_hip_device_count.restype = ctypes.c_int
    assert d.bwamem_hip_device_count() > 0, "no GPU: this script measures on the device only"
    bind(d)
    plib = B.Lib(args.parent_lib, "jnibwa_") if args.parent_lib else None
    if plib:
        bind(plib.dll)

    rng = np.random.default_rng(0xBA4)
    with tempfile.TemporaryDirectory() as tmp:
        seqs = B.synth_genome(args.genome_bp, n_contigs=6, seed=11, repeat_frac=0.08)
        fa = os.path.join(tmp, "g.fa")
        B.write_fasta(fa, seqs)
        assert d.jnibwa_createReferenceIndex(fa.encode(), fa.encode(), b"auto") == 0 and lib.create_index_file(fa, fa + ".img") == 0
        h = lib.open_index(fa + ".img")
        assert h
        parent = None
        if plib:
            ph = plib.open_index(fa + ".img")
            assert ph
            parent = (plib, plib.dll, ph)
        ev = R.Events()
        L = args.read_len
        g = np.frombuffer(b"".join(s for _, s in seqs), dtype=np.uint8)
        bounds = np.cumsum([0] + [len(s) for _, s in seqs])

        def starts(n, span):                                          # uniform over the contigs, never across a boundary
            ci = rng.integers(0, len(seqs), size=n)
            return bounds[ci] + (rng.random(n) * (np.diff(bounds)[ci] - span)).astype(np.int64)

        def repeat(a):                                                # the last tenth of the templates are copies of the first tenth
            k = len(a) // 10
            if k:
                a[len(a) - k:] = a[:k]
            return a

        def quals_of(n):
            q = np.zeros((n, L + 1), dtype=np.uint8)
            q[:, :L] = rng.integers(33 + 2, 33 + 42, size=(n, L), dtype=np.uint8)
            return q.tobytes()
        results = []
        if args.reads:
            rows = R.gather_reads(g, repeat(starts(args.reads, L)), L, repeat(rng.random(args.reads) < 0.5), 0.01, rng)
            results.append(measure(lib, d, ev, h, parent, R.request_of(rows), quals_of(args.reads), args.reads, len(seqs), False, args.reps, args.skip_files, args.skip_check))
            del rows
        if args.pairs:
            isz = repeat(np.clip(rng.normal(400, 50, size=args.pairs), L, 1000).astype(np.int64))
            st = repeat(starts(args.pairs, 1001))
            none = np.zeros(args.pairs, dtype=bool)
            r1 = R.gather_reads(g, st, L, none, 0.01, rng)
            r2 = R.gather_reads(g, st + isz - L, L, ~none, 0.01, rng)
            rows = np.empty((2 * args.pairs, L), dtype=np.uint8)
            rows[0::2], rows[1::2] = r1, r2
            results.append(measure(lib, d, ev, h, parent, R.request_of(rows), quals_of(2 * args.pairs), 2 * args.pairs, len(seqs), True, args.reps, args.skip_files, args.skip_check))
        lib.destroy_index(h)
        if parent:
            plib.destroy_index(parent[2])
    doc = dict(what="alignment QC on the device next to encode, mark and sort (tests/gpu_units/bam_qc_rate.py)", genome_bp=args.genome_bp, read_len=L,
               repeated_fraction=0.1, parent_lib_measured=bool(plib), batches=results)
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({k: v for k, v in doc.items() if k != "batches"}))
    for r in results:
        print(json.dumps({k: v for k, v in r.items() if not k.startswith("all_runs_ms")}))


if __name__ == "__main__":
    main()
