"""Rate of base-level QC on the device next to the steps around it, on the batches of bam_qc_rate.py (the same
generator and seed).  For a single-end and a paired-end batch resident in HBM it times, in one process, by HIP events and by the host
clock, medians of --reps runs after one warm-up run of every shape:
 (i)   bwamem_hip_baseqc_add_batch on the marked records (grouped by read) and on the sorted ones, bwamem_hip_qc_add_batch and
       bwamem_hip_batch_compress_bam of the same batch.  Condition: base-level QC stays below the compression.  Also reported: the byte
       bound -- SEQ (half a byte per base) + QUAL + the touched reference words (the aligned bases at four per byte, and eight words per
       GC-bias window) over the rate of a device-to-device copy measured here (bytes read plus bytes written per second).
 (ii)  with no base-QC object: bwamem_hip_batch_encode_bam, bwamem_hip_qc_add_batch and the file call bwamem_hip_fastq_to_bam_qc of this
       build and of the parent commit's library (--parent-lib), alternately in this process.  Condition: the difference of the medians
       lies within the spread of the runs.
 (iii) --windows-image IMG: bwamem_hip_index_gc_windows on that index (bench.py --keep-image IMG --dump-only writes the bench's), once:
       the call computes windows[] once per handle.
In the same run the two blocks are compared with each other, and the accumulator's totals with the record-level QC of the same batch.
Kernel times proper: run under rocprofv3 --kernel-trace --stats with --skip-files, in a run of its own.  Needs a GPU; there is no
fallback.
usage: baseqc_rate.py [--reads N] [--pairs N] [--genome-bp N] [--reps K] [--out FILE.json] [--skip-files] [--parent-lib LIB.so] [--windows-image IMG]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bam_rate as R  # noqa: E402  (the batch generator, the event timer)
import bam_qc_rate as Q  # noqa: E402  (the bindings of the QC calls and of the steps around)
from sort_rate import both  # noqa: E402
B = R.B

TABLES = ["base", "qual_sum", "qual_n", "aligned", "mism", "ins", "del_ev", "soft", "read_gc", "gcb_reads", "gcb_qual_sum", "gcb_qual_n"]   # BWAMEM_HIP_BASEQC_*


class BamOptions(ctypes.Structure):
    """bwamem_bam_options_t"""
    _fields_ = [("size", ctypes.c_size_t), ("rg_line", ctypes.c_char_p), ("sort", ctypes.c_int), ("mark_dup", ctypes.c_int), ("tags", ctypes.c_uint), ("write_header", ctypes.c_int)]


class BaseQcCounts(ctypes.Structure):
    _fields_ = [("records", ctypes.c_uint64 * 3), ("qcfail_skipped", ctypes.c_uint64), ("gcb_skipped", ctypes.c_uint64)]


def bind(d):
    vp, sz, ci, cp = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_char_p
    Q.bind(d)
    d.bwamem_hip_fastq_to_bam_qc.argtypes = [vp, vp, vp, cp, sz, cp, sz, ctypes.POINTER(BamOptions), ci, ci, vp, vp]
    if hasattr(d, "bwamem_hip_baseqc_create"):
        d.bwamem_hip_baseqc_create.restype = vp; d.bwamem_hip_baseqc_create.argtypes = [vp]
        d.bwamem_hip_baseqc_free.restype = None; d.bwamem_hip_baseqc_free.argtypes = [vp]
        d.bwamem_hip_baseqc_add_batch.argtypes = [vp, vp]
        d.bwamem_hip_baseqc_counts.argtypes = [vp, ctypes.POINTER(BaseQcCounts)]
        d.bwamem_hip_baseqc_array.restype = ctypes.c_int64; d.bwamem_hip_baseqc_array.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_uint64), sz]
        d.bwamem_hip_baseqc_serialize.restype = vp; d.bwamem_hip_baseqc_serialize.argtypes = [vp, ctypes.POINTER(sz)]
        d.bwamem_hip_index_gc_windows.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]


def table_sums(d, q):
    out = {}
    for which, name in enumerate(TABLES):
        n = d.bwamem_hip_baseqc_array(q, which, None, 0)
        buf = (ctypes.c_uint64 * n)()
        assert d.bwamem_hip_baseqc_array(q, which, buf, n) == n
        out[name] = int(np.frombuffer(buf, dtype=np.uint64).sum())
    return out


def copy_rate(ev, n_bytes=1 << 28, reps=5):
    """bytes read plus bytes written per second of a device-to-device copy of n_bytes"""
    hip = ev.hip
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    a, b = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(a), n_bytes) == 0 and hip.hipMalloc(ctypes.byref(b), n_bytes) == 0
    ms = []
    for rep in range(reps + 1):
        rc, t = ev.time(lambda: hip.hipMemcpy(b, a, n_bytes, 3))     # hipMemcpyDeviceToDevice
        assert rc == 0
        if rep:
            ms.append(t)
    hip.hipFree(a); hip.hipFree(b)
    return 2 * n_bytes / (statistics.median(ms) * 1e-3)


def fastq_of(rows, quals, L, paired):
    """FASTQ text of the rows: the names are the template's number"""
    n = rows.shape[0]
    tmpl = np.arange(n, dtype=np.int64) // (2 if paired else 1)
    digits = (tmpl[:, None] // 10 ** np.arange(8, -1, -1, dtype=np.int64)[None, :] % 10 + 48).astype(np.uint8)
    q = np.frombuffer(quals, dtype=np.uint8).reshape(n, L + 1)[:, :L]
    text = np.empty((n, 1 + 9 + 1 + L + 3 + L + 1), dtype=np.uint8)
    text[:, 0] = ord("@"); text[:, 1:10] = digits; text[:, 10] = 10
    text[:, 11:11 + L] = rows; text[:, 11 + L:14 + L] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    text[:, 14 + L:14 + 2 * L] = q; text[:, 14 + 2 * L] = 10
    return text.tobytes()


def spread(v):
    return max(v) - min(v)


def measure(lib, d, ev, h, parent, rows, quals, n_reads, paired, reps, skip_files, rate):
    opts = B.set_opt(lib.default_options(), flag=B.MEM_F_PE if paired else 0)
    ob = ctypes.create_string_buffer(bytes(opts), B.OPT_SIZE)
    pe = 1 if paired else 0
    req = R.request_of(rows)

    def batch(dd, hh):
        b = dd.bwamem_hip_batch_upload(hh, req, len(req))
        assert b and dd.bwamem_hip_batch_keep_offsets(b, 1) == 0 and dd.bwamem_hip_batch_set_qualities(b, quals, len(quals)) == 0
        assert dd.bwamem_hip_batch_align(hh, ob, None, b, 0) == 0
        return b
    b = batch(d, h)
    steps = ("encode", "mark", "baseqc_grouped", "qc_grouped", "sort", "baseqc_sorted", "compress")
    t = {k + "_" + c: [] for k in steps for c in ("events", "wall")}
    sums = counts = qc_counts = None
    for rep in range(reps + 1):                                   # rep 0 warms every shape up
        qa, qb, qq = d.bwamem_hip_baseqc_create(h), d.bwamem_hip_baseqc_create(h), d.bwamem_hip_qc_create(h)
        assert qa and qb and qq
        row = []
        for fn in (lambda: d.bwamem_hip_batch_encode_bam(b, pe, None, None), lambda: d.bwamem_hip_batch_mark_duplicates(b, pe, None),
                   lambda: d.bwamem_hip_baseqc_add_batch(qa, b), lambda: d.bwamem_hip_qc_add_batch(qq, b), lambda: d.bwamem_hip_batch_sort_bam(b),
                   lambda: d.bwamem_hip_baseqc_add_batch(qb, b), lambda: d.bwamem_hip_batch_compress_bam(b, 1)):
            rc, ms, wall = both(ev, fn)
            assert rc == 0
            row += [ms, wall]
        m = d.bwamem_hip_batch_bam_bytes(b)
        if rep == 0:
            sz = ctypes.c_size_t()
            blobs = []
            for q in (qa, qb):
                p = d.bwamem_hip_baseqc_serialize(q, ctypes.byref(sz))
                assert p
                blobs.append(ctypes.string_at(p, sz.value))
                lib._free(p)
            assert blobs[0] == blobs[1], "the block of the sorted records differs from that of the same records grouped by read"
            sums = table_sums(d, qa)
            c = BaseQcCounts()
            assert d.bwamem_hip_baseqc_counts(qa, ctypes.byref(c)) == 0
            counts = dict(records=[int(x) for x in c.records], qcfail_skipped=int(c.qcfail_skipped), gcb_skipped=int(c.gcb_skipped))
            qc_counts = Q.QcCounts()
            assert d.bwamem_hip_qc_counts(qq, ctypes.byref(qc_counts)) == 0
            assert sums["base"] == qc_counts.total_length == sums["qual_n"] and sums["aligned"] + sums["ins"] == qc_counts.bases_mapped_cigar
            assert qc_counts.records_without_nm == 0 and sums["mism"] + qc_counts.ins_bases + qc_counts.del_bases == qc_counts.mismatches
            assert sum(counts["records"]) == qc_counts.sequences and sums["gcb_reads"] + counts["gcb_skipped"] == sum(qc_counts.primary_mapped)
        else:
            for k, v in zip(t, row):
                t[k].append(v)
        d.bwamem_hip_baseqc_free(qa); d.bwamem_hip_baseqc_free(qb); d.bwamem_hip_qc_free(qq)
    med = {k: statistics.median(v) for k, v in t.items()}
    bound_bytes = 1.5 * sums["base"] + sums["aligned"] / 4 + 32 * sums["gcb_reads"]
    worst = max(med["baseqc_grouped_wall"], med["baseqc_sorted_wall"])
    out = dict(reads=n_reads, paired=paired, reps=reps, bam_bytes=int(m), counts=counts, table_sums=sums, **{"ms_" + k: v for k, v in med.items()},
               baseqc_below_compress=bool(worst < med["compress_wall"]), baseqc_over_compress=worst / med["compress_wall"],
               baseqc_over_qc=med["baseqc_grouped_wall"] / med["qc_grouped_wall"], copy_bytes_per_s=rate, byte_bound_bytes=bound_bytes, byte_bound_ms=bound_bytes / rate * 1e3,
               baseqc_over_byte_bound=dict(grouped=med["baseqc_grouped_events"] / (bound_bytes / rate * 1e3), sorted=med["baseqc_sorted_events"] / (bound_bytes / rate * 1e3)),
               sorted_block_equals_grouped=True, totals_equal_record_level_qc=True, all_runs_ms=t)
    # ---- (ii) no base-QC object: this build and the parent's, alternately, on batches of their own
    if parent:
        plib, pd, ph = parent
        pb = batch(pd, ph)
        u = {k + s: [] for k in ("encode", "qc_add_batch") for s in ("", "_parent")}
        for rep in range(reps + 1):
            for who in (("this", "parent"), ("parent", "this"))[rep & 1]:      # alternating: whichever runs second finds the device busy already
                dd, hh, bb, sfx = (d, h, b, "") if who == "this" else (pd, ph, pb, "_parent")
                qq = dd.bwamem_hip_qc_create(hh)
                rc, ms, _ = both(ev, lambda: dd.bwamem_hip_batch_encode_bam(bb, pe, None, None)); assert rc == 0
                rc1, ms1, _ = both(ev, lambda: dd.bwamem_hip_qc_add_batch(qq, bb)); assert rc1 == 0
                dd.bwamem_hip_qc_free(qq)
                if rep:
                    u["encode" + sfx].append(ms); u["qc_add_batch" + sfx].append(ms1)
        pd.bwamem_hip_batch_free(pb)
        for k in ("encode", "qc_add_batch"):
            a, p = u[k], u[k + "_parent"]
            out["off_" + k] = dict(this_ms=statistics.median(a), parent_ms=statistics.median(p), spread_ms=dict(this=spread(a), parent=spread(p)),
                                   within_spread=bool(abs(statistics.median(a) - statistics.median(p)) <= max(spread(a), spread(p))), runs=dict(this=a, parent=p))
    d.bwamem_hip_batch_free(b)
    if skip_files:
        return out
    text = fastq_of(rows, quals, rows.shape[1], paired)
    o = BamOptions(size=ctypes.sizeof(BamOptions), rg_line=None, sort=1, mark_dup=1, tags=0, write_header=1)
    with tempfile.TemporaryDirectory() as tmp:
        path, bpath = os.path.join(tmp, "out.bam"), os.path.join(tmp, "out.bam.bai")
        calls = [("file_fastq_to_bam_qc", d, h)] + ([("file_fastq_to_bam_qc_parent", parent[1], parent[2])] if parent else [])
        secs = {k: [] for k, _, _ in calls}
        for rep in range(reps + 1):
            for key, dd, hh in (calls if rep & 1 else calls[::-1]):
                qq = dd.bwamem_hip_qc_create(hh)
                fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
                fb = os.open(bpath, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
                t0 = time.perf_counter()
                rc = dd.bwamem_hip_fastq_to_bam_qc(hh, ob, None, text, len(text), None, 0, ctypes.byref(o), fd, fb, None, qq)
                dt = time.perf_counter() - t0
                os.close(fd); os.close(fb)
                dd.bwamem_hip_qc_free(qq)
                assert rc == 0
                if rep:
                    secs[key].append(dt)
        for key, v in secs.items():
            out[key] = dict(seconds=statistics.median(v), reads_per_s=n_reads / statistics.median(v), spread_s=spread(v), runs_s=v)
        if parent:
            a, p = out["file_fastq_to_bam_qc"], out["file_fastq_to_bam_qc_parent"]
            out["file_within_spread"] = bool(abs(a["seconds"] - p["seconds"]) <= max(a["spread_s"], p["spread_s"]))
    return out


def windows_time(lib, d, ev, img):
    t0 = time.perf_counter()
    h = lib.open_index(img)
    assert h
    t_open = time.perf_counter() - t0
    out = (ctypes.c_uint64 * 101)()
    rc, ms, wall = both(ev, lambda: d.bwamem_hip_index_gc_windows(h, out))
    assert rc == 0
    rc, ms2, wall2 = both(ev, lambda: d.bwamem_hip_index_gc_windows(h, out))
    assert rc == 0
    lib.destroy_index(h)
    w = [int(x) for x in out]
    return dict(image=os.path.basename(img), open_index_s=t_open, first_call_ms_events=ms, first_call_ms_wall=wall, kept_call_ms_wall=wall2, windows_total=sum(w),
                mean_gc=sum(g * x for g, x in enumerate(w)) / max(sum(w), 1), windows=w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--genome-bp", type=int, default=3_000_000, help="the suite's medium genome, as bam_qc_rate.py")
    ap.add_argument("--reps", type=int, default=4, help="even, so that the two orders of the parent comparison are timed equally often")
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-files", action="store_true", help="batch figures only (the profiler run)")
    ap.add_argument("--parent-lib", default=None, help="libbwamem_hip.so of the parent commit, timed in the same process")
    ap.add_argument("--windows-image", default=None, help="an index image to time bwamem_hip_index_gc_windows on")
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
    results = []
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
        rate = copy_rate(ev)
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
        if args.reads:
            rows = R.gather_reads(g, repeat(starts(args.reads, L)), L, repeat(rng.random(args.reads) < 0.5), 0.01, rng)
            results.append(measure(lib, d, ev, h, parent, rows, quals_of(args.reads), args.reads, False, args.reps, args.skip_files, rate))
            del rows
        if args.pairs:
            isz = repeat(np.clip(rng.normal(400, 50, size=args.pairs), L, 1000).astype(np.int64))
            st = repeat(starts(args.pairs, 1001))
            none = np.zeros(args.pairs, dtype=bool)
            r1 = R.gather_reads(g, st, L, none, 0.01, rng)
            r2 = R.gather_reads(g, st + isz - L, L, ~none, 0.01, rng)
            rows = np.empty((2 * args.pairs, L), dtype=np.uint8)
            rows[0::2], rows[1::2] = r1, r2
            results.append(measure(lib, d, ev, h, parent, rows, quals_of(2 * args.pairs), 2 * args.pairs, True, args.reps, args.skip_files, rate))
        lib.destroy_index(h)
        if parent:
            plib.destroy_index(parent[2])
        win = windows_time(lib, d, ev, args.windows_image) if args.windows_image else None
    doc = dict(what="base-level QC on the device next to QC, sort and compression (tests/gpu_units/baseqc_rate.py)", genome_bp=args.genome_bp, read_len=L,
               repeated_fraction=0.1, parent_lib_measured=bool(plib), batches=results, gc_windows=win)
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({k: v for k, v in doc.items() if k not in ("batches", "gc_windows")}))
    for r in results:
        print(json.dumps({k: v for k, v in r.items() if not k.startswith("all_runs_ms")}))
    if win:
        print(json.dumps({k: v for k, v in win.items() if k != "windows"}))


if __name__ == "__main__":
    main()
