"""Rates of the coordinate sort and the BAI index on the device next to the steps around them, on the batches of
bam_rate.py / bgzf_rate.py (the same generator and seed): for a single-end and a paired-end batch resident in HBM it times, in one
process, bwamem_hip_batch_align, _encode_bam, _sort_bam, _compress_bam and _index_bam, each by HIP events and by the host clock,
and bwamem_hip_align_to_sorted_bam (with its index) against bwamem_hip_align_to_bam_device to a file.  Every figure is the median
of --reps runs after one warm-up run of the same shape.  In the same run the sorted stream is inflated with Python's gzip and
compared with the records sorted in Python, once.  The condition the sort is held to is relative, measured here: _sort_bam plus
_index_bam take no longer than _compress_bam of the same batch.  Kernel times proper: run under rocprofv3 --kernel-trace --stats
with --skip-files, in a run of its own.  Needs a GPU; there is no fallback.
usage: sort_rate.py [--reads N] [--pairs N] [--genome-bp N] [--reps K] [--out FILE.json] [--skip-files]"""
import argparse
import ctypes
import gzip
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
B = R.B


def both(ev, fn):
    """(result, device ms between null-stream events, host ms)"""
    t0 = time.perf_counter()
    r, ms = ev.time(fn)
    return r, ms, (time.perf_counter() - t0) * 1e3


def python_sorted(bam):
    recs, off = [], 0
    while off < len(bam):
        size = 4 + struct.unpack_from("<i", bam, off)[0]
        refid, pos = struct.unpack_from("<ii", bam, off + 4)
        recs.append((refid & 0xffffffff, pos, off, size))
        off += size
    recs.sort(key=lambda t: t[:2])
    return b"".join(bam[o:o + s] for _, _, o, s in recs), len(recs)


def measure(lib, d, ev, h, req, n_reads, paired, reps, skip_files):
    sz = ctypes.c_size_t
    opts = B.set_opt(lib.default_options(), flag=B.MEM_F_PE if paired else 0)
    ob = ctypes.create_string_buffer(bytes(opts), B.OPT_SIZE)
    b = d.bwamem_hip_batch_upload(h, req, len(req))
    assert b and d.bwamem_hip_batch_keep_offsets(b, 1) == 0
    steps = ("align", "encode", "sort", "compress", "index")
    t = {k + "_" + c: [] for k in steps for c in ("events", "wall")}
    unsorted = z = None
    n_bai = 0
    for rep in range(reps + 1):                                   # rep 0 warms every shape up
        row = []
        rc, ms, wall = both(ev, lambda: d.bwamem_hip_batch_align(h, ob, None, b, 0)); assert rc == 0; row += [ms, wall]
        rc, ms, wall = both(ev, lambda: d.bwamem_hip_batch_encode_bam(b, 1 if paired else 0, None, None)); assert rc == 0; row += [ms, wall]
        m = d.bwamem_hip_batch_bam_bytes(b)
        if unsorted is None:
            unsorted = np.empty(m, dtype=np.uint8)
            assert d.bwamem_hip_batch_bam_download(b, unsorted.ctypes.data) == 0
        rc, ms, wall = both(ev, lambda: d.bwamem_hip_batch_sort_bam(b)); assert rc == 0; row += [ms, wall]
        rc, ms, wall = both(ev, lambda: d.bwamem_hip_batch_compress_bam(b, 1)); assert rc == 0; row += [ms, wall]
        n_out = sz()
        p, ms, wall = both(ev, lambda: d.bwamem_hip_batch_index_bam(b, 0, ctypes.byref(n_out))); assert p; row += [ms, wall]
        lib._free(p)
        n_bai = n_out.value
        if rep:
            for k, v in zip(t, row):
                t[k].append(v)
    nz = d.bwamem_hip_batch_bgzf_bytes(b)
    z = np.empty(nz, dtype=np.uint8)
    assert d.bwamem_hip_batch_bgzf_download(b, z.ctypes.data) == 0
    d.bwamem_hip_batch_free(b)
    want, n_rec = python_sorted(unsorted.tobytes())
    assert gzip.decompress(z.tobytes()) == want, "the sorted stream does not inflate to the records sorted in Python"
    med = {k: statistics.median(v) for k, v in t.items()}
    out = dict(reads=n_reads, paired=paired, reps=reps, records=n_rec, bam_bytes=int(unsorted.size), bgzf_bytes=int(nz), bai_bytes=int(n_bai),
               sorted_stream_checked=True, **{"ms_" + k: v for k, v in med.items()},
               ms_sort_plus_index_wall=med["sort_wall"] + med["index_wall"],
               sort_plus_index_within_compress=bool(med["sort_wall"] + med["index_wall"] <= med["compress_wall"]), all_runs_ms=t)
    if skip_files:
        return out
    with tempfile.TemporaryDirectory() as tmp:
        path, bpath = os.path.join(tmp, "out.bam"), os.path.join(tmp, "out.bam.bai")
        for key, call in (("file_device", lambda fd, fb: d.bwamem_hip_align_to_bam_device(h, ob, None, req, len(req), None, fd, 1)),
                          ("file_sorted_indexed", lambda fd, fb: d.bwamem_hip_align_to_sorted_bam(h, ob, None, req, len(req), None, fd, fb, 1))):
            secs = []
            for rep in range(reps + 1):
                fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
                fb = os.open(bpath, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
                t0 = time.perf_counter()
                rc = call(fd, fb)
                dt = time.perf_counter() - t0
                os.close(fd); os.close(fb)
                assert rc == 0
                if rep:
                    secs.append(dt)
            s = statistics.median(secs)
            out[key] = dict(seconds=s, reads_per_s=n_reads / s, bytes=os.path.getsize(path), bai_bytes=os.path.getsize(bpath))
        extra = out["file_sorted_indexed"]["seconds"] - out["file_device"]["seconds"]
        out["file_sorted_extra_ms"] = extra * 1e3
        out["file_sorted_within_compress_margin"] = bool(extra * 1e3 <= med["compress_wall"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--genome-bp", type=int, default=3_000_000, help="the suite's medium genome, as bam_rate.py")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-files", action="store_true", help="batch figures only (the profiler run)")
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
    d.bwamem_hip_batch_sort_bam.argtypes = [vp]
    d.bwamem_hip_batch_compress_bam.argtypes = [vp, ctypes.c_int]
    d.bwamem_hip_batch_bgzf_bytes.restype = sz; d.bwamem_hip_batch_bgzf_bytes.argtypes = [vp]
    d.bwamem_hip_batch_bgzf_download.argtypes = [vp, vp]
    d.bwamem_hip_batch_index_bam.restype = vp; d.bwamem_hip_batch_index_bam.argtypes = [vp, i64, ctypes.POINTER(sz)]
    d.bwamem_hip_align_to_bam_device.argtypes = [vp, vp, vp, ctypes.c_char_p, sz, vp, ctypes.c_int, ctypes.c_int]
    d.bwamem_hip_align_to_sorted_bam.argtypes = [vp, vp, vp, ctypes.c_char_p, sz, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int]
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
            results.append(measure(lib, d, ev, h, R.request_of(rows), args.reads, False, args.reps, args.skip_files))
            del rows
        if args.pairs:
            isz = np.clip(rng.normal(400, 50, size=args.pairs), L, 1000).astype(np.int64)
            st = starts(args.pairs, 1001)
            none = np.zeros(args.pairs, dtype=bool)
            r1 = R.gather_reads(g, st, L, none, 0.01, rng)
            r2 = R.gather_reads(g, st + isz - L, L, ~none, 0.01, rng)
            rows = np.empty((2 * args.pairs, L), dtype=np.uint8)
            rows[0::2], rows[1::2] = r1, r2
            results.append(measure(lib, d, ev, h, R.request_of(rows), 2 * args.pairs, True, args.reps, args.skip_files))
        lib.destroy_index(h)
    doc = dict(what="coordinate sort and BAI index on the device next to encode and compress (tests/gpu_units/sort_rate.py)", genome_bp=args.genome_bp,
               read_len=L, batches=results)
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({k: v for k, v in doc.items() if k != "batches"}))
    for r in results:
        print(json.dumps({k: v for k, v in r.items() if not k.startswith("all_runs_ms")}))


if __name__ == "__main__":
    main()
