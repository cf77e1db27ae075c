"""What the SA / MC / MQ tags cost on the device ("SA, MC and MQ"): for a single-end and a paired-end batch resident in
HBM, aligned once, it times bwamem_hip_batch_encode_bam without tags and with all three (the side-text kernels, one more scan, the
tagged size and emit kernels; still two host waits).  Taken like bam_rate.py's figures: HIP events on the null stream around a call
that ends in a device synchronise; every run after one warm-up run is kept, and the median, the smallest and the largest are
reported.  --chimeric: the share of single-end reads made of two distant halves, so that SA has something to say.
A library without bwamem_hip_batch_set_tags (--lib: an earlier build) is measured without tags only: the same script gives the
untagged encode time before and after the feature.  Needs a GPU; there is no fallback.
usage: bam_tags_rate.py [--lib FILE.so] [--reads N] [--pairs N] [--genome-bp N] [--reps K] [--chimeric F] [--out FILE.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_rate as R  # noqa: E402
from bam_rate import B  # noqa: E402


def measure(lib, d, ev, h, req, n_reads, paired, reps, masks):
    opts = B.set_opt(lib.default_options(), flag=B.MEM_F_PE if paired else 0)
    ob = ctypes.create_string_buffer(bytes(opts), B.OPT_SIZE)
    b = d.bwamem_hip_batch_upload(h, req, len(req))
    assert b and d.bwamem_hip_batch_keep_offsets(b, 1) == 0
    d.bwamem_hip_batch_align(h, ob, None, b, 0)                      # warms the aligner up
    rc, ms_align = ev.time(lambda: d.bwamem_hip_batch_align(h, ob, None, b, 0))
    assert rc == 0
    out = dict(reads=n_reads, paired=paired, reps=reps, ms_align=ms_align, encode={})
    for mask in masks:
        if mask:
            assert d.bwamem_hip_batch_set_tags(b, mask) == 0
        runs = []
        for rep in range(reps + 1):                                   # rep 0 warms the shape up
            rc, ms = ev.time(lambda: d.bwamem_hip_batch_encode_bam(b, 1 if paired else 0, None, None))
            assert rc == 0
            if rep:
                runs.append(ms)
        out["encode"]["tags_%d" % mask] = dict(ms_median=statistics.median(runs), ms_min=min(runs), ms_max=max(runs), bam_bytes=int(d.bwamem_hip_batch_bam_bytes(b)),
                                               all_runs_ms=runs)
    d.bwamem_hip_batch_free(b)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="the library to measure (default: the tree's)")
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--genome-bp", type=int, default=3_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--chimeric", type=float, default=0.02)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.lib:
        B.HIP_LIB = os.path.abspath(args.lib)
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
    d.jnibwa_createReferenceIndex.argtypes = [ctypes.c_char_p] * 3
    masks = [0]
    if hasattr(d, "bwamem_hip_batch_set_tags"):
        d.bwamem_hip_batch_set_tags.argtypes = [vp, ctypes.c_uint]
        masks.append(7)

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
            n_ch = int(args.chimeric * args.reads)
            if n_ch:                                                  # the second half of the first n_ch reads comes from elsewhere
                rows[:n_ch, L // 2:] = R.gather_reads(g, starts(n_ch, L), L, np.zeros(n_ch, dtype=bool), 0.01, rng)[:, L // 2:]
            results.append(measure(lib, d, ev, h, R.request_of(rows), args.reads, False, args.reps, masks))
            del rows
        if args.pairs:
            isz = np.clip(rng.normal(400, 50, size=args.pairs), L, 1000).astype(np.int64)
            st = starts(args.pairs, 1001)
            none = np.zeros(args.pairs, dtype=bool)
            rows = np.empty((2 * args.pairs, L), dtype=np.uint8)
            rows[0::2] = R.gather_reads(g, st, L, none, 0.01, rng)
            rows[1::2] = R.gather_reads(g, st + isz - L, L, ~none, 0.01, rng)
            results.append(measure(lib, d, ev, h, R.request_of(rows), 2 * args.pairs, True, args.reps, masks))
        lib.destroy_index(h)
    doc = dict(what="cost of the SA / MC / MQ tags (tests/gpu_units/bam_tags_rate.py)", lib=args.lib or "tree", genome_bp=args.genome_bp, read_len=L,
               chimeric=args.chimeric, batches=results)
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    for r in results:
        print(json.dumps(dict(reads=r["reads"], paired=r["paired"], ms_align=r["ms_align"],
                              **{k: {x: v[x] for x in ("ms_median", "ms_min", "ms_max", "bam_bytes")} for k, v in r["encode"].items()})))


if __name__ == "__main__":
    main()
