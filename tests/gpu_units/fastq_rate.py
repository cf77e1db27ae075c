"""Rates of the FASTQ path on the device next to the steps it must not slow down, on the batches of bam_rate.py /
sort_rate.py (the same generator and seed): for a single-end and a paired-end batch it times, in one process,
  * bwamem_hip_batch_encode_bam without qualities and without a read group (the default path), and with both;
  * bwamem_hip_batch_upload_fastq of the same reads as FASTQ text (names, qualities), against bwamem_hip_batch_upload of the request,
    and the plain host-to-device copy of the text (hipMemcpy into a device buffer), which gives the copy rate of this run;
  * bwamem_hip_align_fastq_to_bam (sorted, indexed, with a read group) to a file against bwamem_hip_align_to_sorted_bam on the same
    reads with caller names; the allowance for the difference is the extra text bytes over the copy rate measured here.
Every figure is the median of --reps runs after one warm-up run of the same shape, by HIP events and by the host clock.  The
per-kernel device time of the parse comes from bwamem_hip_stats (HIP events around each launch); kernel times proper: run under
rocprofv3 --kernel-trace --stats with --skip-files, in a run of its own.  --parent-lib names a build of the parent commit: its
default encode and its file call are then timed in the same process, alternating with this build's.  In the same run the records of
the FASTQ-built batch are compared with the host-API path's, once.  Needs a GPU; there is no fallback.
usage: fastq_rate.py [--reads N] [--pairs N] [--genome-bp N] [--reps K] [--out FILE.json] [--skip-files] [--parent-lib LIB.so]"""
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
B = R.B
RG = b"@RG\tID:rate\tSM:sample"


class Stats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("n_reads", "n_ext", "n_lf", "n_sa", "n_dp_cells")] + \
               [(n, ctypes.c_double) for n in ("ms_encode", "ms_seed", "ms_sa", "ms_chain", "ms_extend", "ms_post", "ms_final", "ms_pack", "ms_other")] + \
               [(n, ctypes.c_uint64) for n in ("n_launch_seed", "n_launch_sa", "n_launch_extend", "n_tiles", "n_retries")]


def bind(d, new):
    vp, sz, i64, cp = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int64, ctypes.c_char_p
    d.bwamem_hip_batch_upload.restype = vp; d.bwamem_hip_batch_upload.argtypes = [vp, cp, sz]
    d.bwamem_hip_batch_align.argtypes = [vp, vp, vp, vp, i64]
    d.bwamem_hip_batch_free.argtypes = [vp]; d.bwamem_hip_batch_free.restype = None
    d.bwamem_hip_batch_keep_offsets.argtypes = [vp, ctypes.c_int]
    d.bwamem_hip_batch_encode_bam.argtypes = [vp, ctypes.c_int, cp, ctypes.POINTER(i64)]
    d.bwamem_hip_batch_bam_bytes.restype = sz; d.bwamem_hip_batch_bam_bytes.argtypes = [vp]
    d.bwamem_hip_batch_bam_download.argtypes = [vp, vp]
    d.bwamem_hip_align_to_sorted_bam.argtypes = [vp, vp, vp, cp, sz, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    d.bwamem_hip_stats_enable.argtypes = [ctypes.c_int]; d.bwamem_hip_stats_get.argtypes = [ctypes.POINTER(Stats)]
    d.jnibwa_createReferenceIndex.argtypes = [cp] * 3
    if new:
        d.bwamem_hip_batch_set_qualities.argtypes = [vp, cp, sz]
        d.bwamem_hip_batch_set_read_group.argtypes = [vp, cp]
        d.bwamem_hip_batch_upload_fastq.restype = vp; d.bwamem_hip_batch_upload_fastq.argtypes = [vp, cp, sz, cp, sz, ctypes.POINTER(i64)]
        d.bwamem_hip_align_fastq_to_bam.argtypes = [vp, vp, vp, cp, sz, cp, sz, cp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]


def both(ev, fn):
    t0 = time.perf_counter()
    r, ms = ev.time(fn)
    return r, ms, (time.perf_counter() - t0) * 1e3


def fastq_of(rows, quals, names):
    """fixed-width records: '@' name '\\n' bases '\\n+\\n' qualities '\\n'"""
    n, L = rows.shape
    w = names.shape[1]
    t = np.empty((n, 1 + w + 1 + L + 3 + L + 1), dtype=np.uint8)
    t[:, 0] = ord("@"); t[:, 1:1 + w] = names; t[:, 1 + w] = 10
    t[:, 2 + w:2 + w + L] = rows
    t[:, 2 + w + L:5 + w + L] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    t[:, 5 + w + L:5 + w + 2 * L] = quals
    t[:, -1] = 10
    return t.tobytes()


def names_of(n, per):
    """fixed-width names, `per` consecutive reads sharing one"""
    idx = np.arange(n, dtype=np.int64) // per
    digits = (idx[:, None] // 10 ** np.arange(8, -1, -1, dtype=np.int64)[None, :]) % 10
    out = np.empty((n, 11), dtype=np.uint8)
    out[:, 0], out[:, 1] = ord("R"), ord(":")
    out[:, 2:] = digits + ord("0")
    return out


def med(v):
    return statistics.median(v)


def measure(new, parent, ev, hip, rows, paired, reps, skip_files):
    lib, d, h = new
    n, L = rows.shape
    rng = np.random.default_rng(0xF0)
    quals = rng.integers(33, 127, size=(n, L), dtype=np.uint8)
    names = names_of(n, 2 if paired else 1)
    req = R.request_of(rows)
    qblob = np.zeros((n, L + 1), dtype=np.uint8); qblob[:, :L] = quals; qblob = qblob.tobytes()
    nblob = names.tobytes()
    noff = (ctypes.c_int64 * (n + 1))(*range(0, 11 * (n + 1), 11))
    if paired:
        t1, t2 = fastq_of(rows[0::2], quals[0::2], names[0::2]), fastq_of(rows[1::2], quals[1::2], names[1::2])
    else:
        t1, t2 = fastq_of(rows, quals, names), None
    text_bytes = len(t1) + (len(t2) if t2 else 0)
    opts = B.set_opt(lib.default_options(), flag=B.MEM_F_PE if paired else 0)
    ob = ctypes.create_string_buffer(bytes(opts), B.OPT_SIZE)
    pe = 1 if paired else 0
    out = dict(reads=n, paired=paired, reps=reps, request_bytes=len(req), fastq_bytes=text_bytes)
    stats = Stats()

    def other_ms(fn):
        d.bwamem_hip_stats_get(ctypes.byref(stats)); a = stats.ms_other
        r = fn()
        d.bwamem_hip_stats_get(ctypes.byref(stats))
        return r, stats.ms_other - a

    # ---- the batches: this build's from the request, from FASTQ text, and the parent's from the request
    b = d.bwamem_hip_batch_upload(h, req, len(req))
    assert b and d.bwamem_hip_batch_keep_offsets(b, 1) == 0
    d.bwamem_hip_stats_get(ctypes.byref(stats)); fp0 = stats.ms_final + stats.ms_pack
    rc, ms_align, _ = both(ev, lambda: d.bwamem_hip_batch_align(h, ob, None, b, 0)); assert rc == 0
    d.bwamem_hip_stats_get(ctypes.byref(stats)); fp = stats.ms_final + stats.ms_pack - fp0
    pb = None
    if parent:
        plib, pd, ph = parent
        pb = pd.bwamem_hip_batch_upload(ph, req, len(req))
        assert pb and pd.bwamem_hip_batch_keep_offsets(pb, 1) == 0 and pd.bwamem_hip_batch_align(ph, ob, None, pb, 0) == 0
    t = {k: [] for k in ("encode_default", "encode_default_parent", "encode_names", "encode_names_quals_rg", "upload_request", "upload_fastq", "copy_text", "parse_kernels")}
    dev = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(dev), ctypes.c_size_t(text_bytes + 64)) == 0
    bad = ctypes.c_int64()
    fb = None
    for rep in range(reps + 1):                                   # rep 0 warms every shape up
        row = {}
        assert d.bwamem_hip_batch_set_qualities(b, None, 0) == 0 and d.bwamem_hip_batch_set_read_group(b, None) == 0
        for who in (("this", "parent"), ("parent", "this"))[rep & 1]:          # alternating: whichever runs second finds the device busy already
            if who == "this":
                rc, ms, _ = both(ev, lambda: d.bwamem_hip_batch_encode_bam(b, pe, None, None)); assert rc == 0; row["encode_default"] = ms
            elif pb:
                rc, ms, _ = both(ev, lambda: pd.bwamem_hip_batch_encode_bam(pb, pe, None, None)); assert rc == 0; row["encode_default_parent"] = ms
        rc, ms, _ = both(ev, lambda: d.bwamem_hip_batch_encode_bam(b, pe, nblob, noff)); assert rc == 0; row["encode_names"] = ms
        assert d.bwamem_hip_batch_set_qualities(b, qblob, len(qblob)) == 0 and d.bwamem_hip_batch_set_read_group(b, RG) == 0
        rc, ms, _ = both(ev, lambda: d.bwamem_hip_batch_encode_bam(b, pe, nblob, noff)); assert rc == 0; row["encode_names_quals_rg"] = ms
        ub, ms, _ = both(ev, lambda: d.bwamem_hip_batch_upload(h, req, len(req))); assert ub; row["upload_request"] = ms
        d.bwamem_hip_batch_free(ub)
        if fb:
            d.bwamem_hip_batch_free(fb)
        (fb, ms, _), k_ms = other_ms(lambda: both(ev, lambda: d.bwamem_hip_batch_upload_fastq(h, t1, len(t1), t2, len(t2) if t2 else 0, ctypes.byref(bad))))
        assert fb, bad.value
        row["upload_fastq"], row["parse_kernels"] = ms, k_ms
        rc, ms, _ = both(ev, lambda: hip.hipMemcpy(dev, t1, ctypes.c_size_t(len(t1)), 1) or (hip.hipMemcpy(ctypes.c_void_p(dev.value + len(t1)), t2, ctypes.c_size_t(len(t2)), 1) if t2 else 0))
        assert rc == 0; row["copy_text"] = ms
        print("rep %d %s" % (rep, json.dumps({k: round(v, 3) for k, v in row.items()})), file=sys.stderr, flush=True)
        if rep:
            for k, v in row.items():
                t[k].append(v)
    assert hip.hipFree(dev) == 0
    # the records of the FASTQ-built batch against the host-API path's, once
    m = d.bwamem_hip_batch_bam_bytes(b)
    want = np.empty(m, dtype=np.uint8)
    assert d.bwamem_hip_batch_bam_download(b, want.ctypes.data) == 0
    assert d.bwamem_hip_batch_keep_offsets(fb, 1) == 0 and d.bwamem_hip_batch_align(h, ob, None, fb, 0) == 0
    assert d.bwamem_hip_batch_set_read_group(fb, RG) == 0 and d.bwamem_hip_batch_encode_bam(fb, pe, None, None) == 0
    got = np.empty(d.bwamem_hip_batch_bam_bytes(fb), dtype=np.uint8)
    assert d.bwamem_hip_batch_bam_download(fb, got.ctypes.data) == 0
    assert got.size == want.size and np.array_equal(got, want), "the FASTQ-built batch's records differ from the host-API path's"
    d.bwamem_hip_batch_free(fb); d.bwamem_hip_batch_free(b)
    if pb:
        pd.bwamem_hip_batch_free(pb)
    out.update({"ms_" + k: med(v) for k, v in t.items() if v}, all_runs_ms=t, records_checked=True, bam_bytes=int(m), ms_align=ms_align,
               ms_final_plus_pack=fp)
    if fp > 0:
        out["encode_default_over_final_pack"] = out["ms_encode_default"] / fp
        out["encode_names_quals_rg_over_final_pack"] = out["ms_encode_names_quals_rg"] / fp
    if t["encode_default_parent"]:
        a, p = t["encode_default"], t["encode_default_parent"]
        out["encode_default_spread_ms"] = dict(this=max(a) - min(a), parent=max(p) - min(p))
        out["encode_default_not_slower_than_parent"] = bool(med(a) - med(p) <= max(max(a) - min(a), max(p) - min(p)))
    copy_rate = text_bytes / (out["ms_copy_text"] * 1e-3)
    out["copy_bytes_per_s"] = copy_rate
    # the parse and copy kernels read the text and the line index and write payload, qualities and names: bytes moved over their time
    moved = text_bytes + 8 * (4 * n) * 2 + 2 * len(req) + len(nblob) + 8 * 4 * n
    out["parse_bytes_moved"] = moved
    out["parse_bytes_per_s"] = moved / (out["ms_parse_kernels"] * 1e-3) if out["ms_parse_kernels"] > 0 else None
    if skip_files:
        return out
    arr = (ctypes.c_char_p * n)(*[bytes(x) for x in names])
    with tempfile.TemporaryDirectory() as tmp:
        path, bpath = os.path.join(tmp, "out.bam"), os.path.join(tmp, "out.bam.bai")
        calls = [("file_fastq", lambda fd, fb_: d.bwamem_hip_align_fastq_to_bam(h, ob, None, t1, len(t1), t2, len(t2) if t2 else 0, RG, 1, fd, fb_, 1)),
                 ("file_request", lambda fd, fb_: d.bwamem_hip_align_to_sorted_bam(h, ob, None, req, len(req), arr, fd, fb_, 1))]
        if parent:
            calls.append(("file_request_parent", lambda fd, fb_: pd.bwamem_hip_align_to_sorted_bam(ph, ob, None, req, len(req), arr, fd, fb_, 1)))
        secs = {k: [] for k, _ in calls}
        sizes = {}
        for rep in range(reps + 1):
            for key, call in calls:                                   # alternating
                fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
                fb_ = os.open(bpath, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
                t0 = time.perf_counter()
                rc = call(fd, fb_)
                dt = time.perf_counter() - t0
                os.close(fd); os.close(fb_)
                assert rc == 0
                sizes[key] = os.path.getsize(path)
                print("file %s rep %d %.3f s" % (key, rep, dt), file=sys.stderr, flush=True)
                if rep:
                    secs[key].append(dt)
        for key, v in secs.items():
            out[key] = dict(seconds=med(v), reads_per_s=n / med(v), bam_file_bytes=sizes[key], all_seconds=v)
        base = "file_request_parent" if parent else "file_request"
        out["file_fastq_extra_ms"] = (out["file_fastq"]["seconds"] - out[base]["seconds"]) * 1e3
        out["file_fastq_allowance_ms"] = (text_bytes - len(req)) / copy_rate * 1e3
        out["file_fastq_against"] = base
        out["file_fastq_within_allowance"] = bool(out["file_fastq_extra_ms"] <= out["file_fastq_allowance_ms"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--genome-bp", type=int, default=3_000_000, help="the suite's medium genome, as bam_rate.py")
    ap.add_argument("--reps", type=int, default=4, help="even, so that the two orders of the parent comparison are timed equally often")
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-files", action="store_true", help="batch figures only (the profiler run)")
    ap.add_argument("--parent-lib", default=None, help="libbwamem_hip.so of the parent commit, timed in the same process")
    args = ap.parse_args()
    lib = B.product_lib()
    d = lib.dll
    d.bwamem_hip_device_count.restype = ctypes.c_int
    assert d.bwamem_hip_device_count() > 0, "no GPU: this script measures on the device only"
    bind(d, True)
    d.bwamem_hip_stats_enable(1)
    plib = None
    if args.parent_lib:
        plib = B.Lib(args.parent_lib, "jnibwa_")
        bind(plib.dll, False)
    rng = np.random.default_rng(0xBA4)
    with tempfile.TemporaryDirectory() as tmp:
        seqs = B.synth_genome(args.genome_bp, n_contigs=6, seed=11, repeat_frac=0.08)
        fa = os.path.join(tmp, "g.fa")
        B.write_fasta(fa, seqs)
        assert d.jnibwa_createReferenceIndex(fa.encode(), fa.encode(), b"auto") == 0 and lib.create_index_file(fa, fa + ".img") == 0
        h = lib.open_index(fa + ".img")
        assert h
        new = (lib, d, h)
        parent = None
        if plib:
            ph = plib.open_index(fa + ".img")
            assert ph
            parent = (plib, plib.dll, ph)
        ev = R.Events()
        hip = ev.hip
        hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]
        hip.hipFree.argtypes = [ctypes.c_void_p]
        L = args.read_len
        g = np.frombuffer(b"".join(s for _, s in seqs), dtype=np.uint8)
        bounds = np.cumsum([0] + [len(s) for _, s in seqs])

        def starts(n, span):                                          # uniform over the contigs, never across a boundary
            ci = rng.integers(0, len(seqs), size=n)
            return bounds[ci] + (rng.random(n) * (np.diff(bounds)[ci] - span)).astype(np.int64)
        results = []
        if args.reads:
            rows = R.gather_reads(g, starts(args.reads, L), L, rng.random(args.reads) < 0.5, 0.01, rng)
            results.append(measure(new, parent, ev, hip, rows, False, args.reps, args.skip_files))
            del rows
        if args.pairs:
            isz = np.clip(rng.normal(400, 50, size=args.pairs), L, 1000).astype(np.int64)
            st = starts(args.pairs, 1001)
            none = np.zeros(args.pairs, dtype=bool)
            r1 = R.gather_reads(g, st, L, none, 0.01, rng)
            r2 = R.gather_reads(g, st + isz - L, L, ~none, 0.01, rng)
            rows = np.empty((2 * args.pairs, L), dtype=np.uint8)
            rows[0::2], rows[1::2] = r1, r2
            results.append(measure(new, parent, ev, hip, rows, True, args.reps, args.skip_files))
        lib.destroy_index(h)
        if parent:
            plib.destroy_index(parent[2])
    doc = dict(what="FASTQ parsed on the device, qualities and read groups in BAM records, next to the default path (tests/gpu_units/fastq_rate.py)",
               genome_bp=args.genome_bp, read_len=L, parent_lib_measured=bool(plib), batches=results)
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({k: v for k, v in doc.items() if k != "batches"}))
    for r in results:
        print(json.dumps({k: v for k, v in r.items() if not k.startswith("all_runs_ms")}))


if __name__ == "__main__":
    main()
