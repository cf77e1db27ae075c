"""Rates of BGZF compression on the device against the host path it replaces, on the batches of bam_rate.py (the same
generator and seed): for a single-end and a paired-end batch resident in HBM it times, in one process,
  (a) bwamem_hip_batch_align and (b) bwamem_hip_batch_encode_bam,
  (c) bwamem_hip_batch_compress_bam, by HIP events and by the host clock,
  (d) the download of the compressed bytes,
  (e) the host path: the download of the raw records plus bwamem_hip_bgzf_compress at level 1 with 16 threads,
  (f) bwamem_hip_align_to_bam (level 1) and bwamem_hip_align_to_bam_device to a file,
and records the compressed bytes per read of both.  Every figure is the median of --reps runs after one warm-up run of the same
shape.  ms_other of bwamem_hip_stats_get is the time of the two kernels alone.  The device's stream is inflated with Python's gzip
and compared with the records once.  Kernel times proper: run under rocprofv3 --kernel-trace --stats with --skip-host, in a run of
its own.  Needs a GPU; there is no fallback.
usage: bgzf_rate.py [--reads N] [--pairs N] [--genome-bp N] [--reps K] [--out FILE.json] [--skip-host]"""
import argparse
import ctypes
import gzip
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bam_rate as R  # noqa: E402  (the batch generator, the event timer, the stats reader)
B = R.B


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


def measure(lib, d, ev, h, req, n_reads, paired, reps, skip_host):
    sz = ctypes.c_size_t
    opts = B.set_opt(lib.default_options(), flag=B.MEM_F_PE if paired else 0)
    ob = ctypes.create_string_buffer(bytes(opts), B.OPT_SIZE)
    b = d.bwamem_hip_batch_upload(h, req, len(req))
    assert b and d.bwamem_hip_batch_keep_offsets(b, 1) == 0
    d.bwamem_hip_stats_enable(1)
    t = dict(align=[], encode=[], compress_events=[], compress_wall=[], compress_kernels=[], download_bgzf=[], download_raw=[])
    bam = z = None
    for rep in range(reps + 1):                                   # rep 0 warms every shape up
        rc, ms_a = ev.time(lambda: d.bwamem_hip_batch_align(h, ob, None, b, 0))
        assert rc == 0
        rc, ms_b = ev.time(lambda: d.bwamem_hip_batch_encode_bam(b, 1 if paired else 0, None, None))
        assert rc == 0
        d.bwamem_hip_stats_reset()
        (rc, ms_c), wall_c = timed(lambda: ev.time(lambda: d.bwamem_hip_batch_compress_bam(b, 1)))
        assert rc == 0
        ms_k = R.stats_get(d)["ms_other"]
        m, nz = d.bwamem_hip_batch_bam_bytes(b), d.bwamem_hip_batch_bgzf_bytes(b)
        if bam is None:
            bam, z = np.empty(m, dtype=np.uint8), np.empty(nz, dtype=np.uint8)
        assert m == bam.size and nz == z.size
        rc, ms_d = timed(lambda: d.bwamem_hip_batch_bgzf_download(b, z.ctypes.data))
        assert rc == 0
        rc, ms_e = timed(lambda: d.bwamem_hip_batch_bam_download(b, bam.ctypes.data))
        assert rc == 0
        if rep:
            for k, v in zip(t, (ms_a, ms_b, ms_c, wall_c, ms_k, ms_d, ms_e)):
                t[k].append(v)
    d.bwamem_hip_batch_free(b)
    d.bwamem_hip_stats_enable(0)
    assert gzip.decompress(z.tobytes()) == bam.tobytes(), "the device's BGZF stream does not inflate to the records"
    med = {k: statistics.median(v) for k, v in t.items()}
    out = dict(reads=n_reads, paired=paired, reps=reps, bam_bytes=int(bam.size), bam_bytes_per_read=bam.size / n_reads,
               device_bgzf_bytes=int(z.size), device_bgzf_bytes_per_read=z.size / n_reads, device_ratio=z.size / bam.size,
               ms_align=med["align"], ms_encode_bam=med["encode"], ms_compress_events=med["compress_events"], ms_compress_wall=med["compress_wall"],
               ms_compress_kernels=med["compress_kernels"], ms_download_bgzf=med["download_bgzf"], ms_download_raw=med["download_raw"],
               ms_device_path=med["compress_wall"] + med["download_bgzf"], compress_GBps_input=bam.size / med["compress_wall"] / 1e6,
               compress_keeps_up_with_aligner=bool(med["compress_wall"] <= med["align"]), all_runs_ms=t)
    if skip_host:
        return out
    try:
        ctypes.CDLL("libz.so.1")
    except OSError:
        out["libz"] = False
        return out
    out["libz"] = True
    ms, zbytes = [], 0
    for rep in range(reps + 1):
        n_out = sz()
        p, dt = timed(lambda: d.bwamem_hip_bgzf_compress(bam.ctypes.data_as(ctypes.c_char_p), bam.size, 1, 16, 1, ctypes.byref(n_out)))
        assert p
        lib._free(p)
        zbytes = n_out.value
        if rep:
            ms.append(dt)
    ms_host = statistics.median(ms)
    out.update(host_level1_threads=16, ms_host_level1=ms_host, host_level1_bytes=int(zbytes), host_level1_bytes_per_read=zbytes / n_reads,
               ms_host_path=med["download_raw"] + ms_host, device_path_faster_than_host_path=bool(out["ms_device_path"] < med["download_raw"] + ms_host),
               device_bytes_over_host_level1=z.size / zbytes, all_runs_ms_host_level1=ms)
    with tempfile.TemporaryDirectory() as tmp:
        for key, call in (("file_host_level1", lambda fd: d.bwamem_hip_align_to_bam(h, ob, None, req, len(req), None, 1, fd, 1)),
                          ("file_device", lambda fd: d.bwamem_hip_align_to_bam_device(h, ob, None, req, len(req), None, fd, 1))):
            secs = []
            for rep in range(reps + 1):
                fd = os.open(os.path.join(tmp, "out.bam"), os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
                rc, dt = timed(lambda: call(fd))
                os.close(fd)
                assert rc == 0
                if rep:
                    secs.append(dt / 1e3)
            s = statistics.median(secs)
            out[key] = dict(seconds=s, reads_per_s=n_reads / s, bytes=os.path.getsize(os.path.join(tmp, "out.bam")))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--genome-bp", type=int, default=3_000_000, help="the suite's medium genome, as bam_rate.py")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-host", action="store_true", help="device figures only (the profiler run)")
    args = ap.parse_args()
    lib = B.product_lib()
    d = lib.dll
    vp, sz, i64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int64
    d.bwamem_hip_device_count.restype = ctypes.c_int
    assert d.bwamem_hip_device_count() > 0, "no GPU: this script measures on the device only"
    d.bwamem_hip_batch_upload.restype = vp; d.bwamem_hip_batch_upload.argtypes = [vp, ctypes.c_char_p, sz]
    d.bwamem_hip_batch_align.argtypes = [vp, vp, vp, vp, i64]
    d.bwamem_hip_batch_free.argtypes = [vp]; d.bwamem_hip_batch_free.restype = None
    d.bwamem_hip_batch_keep_offsets.argtypes = [vp, ctypes.c_int]
    d.bwamem_hip_batch_encode_bam.argtypes = [vp, ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(i64)]
    d.bwamem_hip_batch_bam_bytes.restype = sz; d.bwamem_hip_batch_bam_bytes.argtypes = [vp]
    d.bwamem_hip_batch_bam_download.argtypes = [vp, vp]
    d.bwamem_hip_batch_compress_bam.argtypes = [vp, ctypes.c_int]
    d.bwamem_hip_batch_bgzf_bytes.restype = sz; d.bwamem_hip_batch_bgzf_bytes.argtypes = [vp]
    d.bwamem_hip_batch_bgzf_download.argtypes = [vp, vp]
    d.bwamem_hip_bgzf_compress.restype = vp; d.bwamem_hip_bgzf_compress.argtypes = [ctypes.c_char_p, sz, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(sz)]
    d.bwamem_hip_align_to_bam.argtypes = [vp, vp, vp, ctypes.c_char_p, sz, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    d.bwamem_hip_align_to_bam_device.argtypes = [vp, vp, vp, ctypes.c_char_p, sz, vp, ctypes.c_int, ctypes.c_int]
    d.bwamem_hip_stats_get.argtypes = [vp]
    d.jnibwa_createReferenceIndex.argtypes = [ctypes.c_char_p] * 3

    rng = np.random.default_rng(0xBA4)
    with tempfile.TemporaryDirectory() as tmp:
        seqs = B.synth_genome(args.genome_bp, n_contigs=6, seed=11, repeat_frac=0.08)
        fa = os.path.join(tmp, "g.fa")
        B.write_fasta(fa, seqs)
        assert d.jnibwa_createReferenceIndex(fa.encode(), fa.encode(), b"auto") == 0 and lib.create_index_file(fa, fa + ".img") == 0
        h = lib.open_index(fa + ".img")
        assert h
        ev = R.Events()
        L = args.read_len
        g = np.frombuffer(b"".join(s for _, s in seqs), dtype=np.uint8)
        bounds = np.cumsum([0] + [len(s) for _, s in seqs])

        def starts(n, span):                                          # uniform over the contigs, never across a boundary
            ci = rng.integers(0, len(seqs), size=n)
            return bounds[ci] + (rng.random(n) * (np.diff(bounds)[ci] - span)).astype(np.int64)
        results = []
        if args.reads:
            rows = R.gather_reads(g, starts(args.reads, L), L, rng.random(args.reads) < 0.5, 0.01, rng)
            results.append(measure(lib, d, ev, h, R.request_of(rows), args.reads, False, args.reps, args.skip_host))
            del rows
        if args.pairs:
            isz = np.clip(rng.normal(400, 50, size=args.pairs), L, 1000).astype(np.int64)
            st = starts(args.pairs, 1001)
            none = np.zeros(args.pairs, dtype=bool)
            r1 = R.gather_reads(g, st, L, none, 0.01, rng)
            r2 = R.gather_reads(g, st + isz - L, L, ~none, 0.01, rng)
            rows = np.empty((2 * args.pairs, L), dtype=np.uint8)
            rows[0::2], rows[1::2] = r1, r2
            results.append(measure(lib, d, ev, h, R.request_of(rows), 2 * args.pairs, True, args.reps, args.skip_host))
        lib.destroy_index(h)
    doc = dict(what="BGZF on the device against host level 1 (tests/gpu_units/bgzf_rate.py)", genome_bp=args.genome_bp, read_len=L, batches=results)
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({k: v for k, v in doc.items() if k != "batches"}))
    for r in results:
        print(json.dumps({k: v for k, v in r.items() if not k.startswith("all_runs_ms")}))


if __name__ == "__main__":
    main()
