"""Rates of the BAM path on the device ("BAM output"): for a single-end and a paired-end batch resident in HBM it times
  (a) bwamem_hip_batch_align,
  (b) bwamem_hip_batch_encode_bam (the size kernel, the scan, the emit kernel, two small read-backs),
  (c) the download of the records,
  (d) BGZF framing on the host at level 0 and level 1 with 16 threads,
and the whole of bwamem_hip_align_to_bam to a file at both levels.  (a)-(c) are taken with HIP events on the null stream around
calls that end in a device synchronise, (d) and the file runs with the host clock.  Every figure is the median of --reps runs
after one warm-up run of the same shape.  ms_final and ms_pack of the same batch come from bwamem_hip_stats_get: the encoder writes
the very records those two stages wrote, so (b) is reported next to their sum.  Kernel times proper: run this script under
rocprofv3 --kernel-trace --stats (bam_rate.sh does, in a run of its own).  Needs a GPU; there is no fallback.
usage: bam_rate.py [--reads N] [--pairs N] [--genome-bp N] [--reps K] [--out FILE.json] [--skip-host]"""
import argparse
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
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bwalib as B  # noqa: E402

COMP = np.zeros(256, dtype=np.uint8)
for a, b in zip(b"ACGTN", b"TGCAN"):
    COMP[a] = b


def hip_runtime():
    """the HIP runtime the product library itself is linked against (already loaded with it)"""
    for ln in open("/proc/self/maps"):
        if "libamdhip64" in ln:
            return ctypes.CDLL(ln.split()[-1])
    raise RuntimeError("the HIP runtime is not loaded")


class Events:
    def __init__(self):
        self.hip = hip_runtime()
        self.hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
        self.hip.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self.hip.hipEventSynchronize.argtypes = [ctypes.c_void_p]
        self.a, self.b = ctypes.c_void_p(), ctypes.c_void_p()
        assert self.hip.hipEventCreate(ctypes.byref(self.a)) == 0 and self.hip.hipEventCreate(ctypes.byref(self.b)) == 0

    def time(self, fn):
        """device milliseconds between two null-stream events around fn (fn's work runs on blocking streams and ends synchronised)"""
        assert self.hip.hipEventRecord(self.a, None) == 0
        r = fn()
        assert self.hip.hipEventRecord(self.b, None) == 0 and self.hip.hipEventSynchronize(self.b) == 0
        ms = ctypes.c_float()
        assert self.hip.hipEventElapsedTime(ctypes.byref(ms), self.a, self.b) == 0
        return r, float(ms.value)


def gather_reads(g, pos, length, rc, sub, rng):
    idx = pos[:, None] + np.arange(length, dtype=np.int64)[None, :]
    r = g[idx]
    mut = rng.random(r.shape) < sub
    r[mut] = B.BASES[(np.searchsorted(B.BASES, r[mut]) + rng.integers(1, 4, size=int(mut.sum()))) % 4]
    r[rc] = COMP[r[rc][:, ::-1]]
    return r


def request_of(rows):
    n, length = rows.shape
    buf = np.zeros((n, length + 1), dtype=np.uint8)
    buf[:, :length] = rows
    return struct.pack("<i", n) + buf.tobytes()


def stats_get(d):
    buf = (ctypes.c_uint64 * 32)()
    d.bwamem_hip_stats_get(buf)
    dbl = (ctypes.c_double * 9).from_buffer_copy(bytes(buf)[40:112])
    return dict(zip(("ms_encode", "ms_seed", "ms_sa", "ms_chain", "ms_extend", "ms_post", "ms_final", "ms_pack", "ms_other"), dbl))


def measure(lib, d, ev, h, req, n_reads, paired, reps, skip_host):
    vp, sz, i64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int64
    opts = B.set_opt(lib.default_options(), flag=B.MEM_F_PE if paired else 0)
    ob = ctypes.create_string_buffer(bytes(opts), B.OPT_SIZE)
    b = d.bwamem_hip_batch_upload(h, req, len(req))
    assert b and d.bwamem_hip_batch_keep_offsets(b, 1) == 0
    d.bwamem_hip_stats_enable(1)
    t = dict(align=[], encode=[], download=[], final_plus_pack=[], ms_final=[], ms_pack=[])
    bam = None
    for rep in range(reps + 1):                                   # rep 0 warms every shape up
        d.bwamem_hip_stats_reset()
        rc, ms_a = ev.time(lambda: d.bwamem_hip_batch_align(h, ob, None, b, 0))
        assert rc == 0
        st = stats_get(d)
        rc, ms_b = ev.time(lambda: d.bwamem_hip_batch_encode_bam(b, 1 if paired else 0, None, None))
        assert rc == 0
        m = d.bwamem_hip_batch_bam_bytes(b)
        if bam is None:
            bam = np.empty(m, dtype=np.uint8)
        assert m == bam.size
        rc, ms_c = ev.time(lambda: d.bwamem_hip_batch_bam_download(b, bam.ctypes.data))
        assert rc == 0
        if rep:
            t["align"].append(ms_a); t["encode"].append(ms_b); t["download"].append(ms_c)
            t["ms_final"].append(st["ms_final"]); t["ms_pack"].append(st["ms_pack"]); t["final_plus_pack"].append(st["ms_final"] + st["ms_pack"])
    resp_bytes = d.bwamem_hip_batch_result_bytes(b)
    d.bwamem_hip_batch_free(b)
    d.bwamem_hip_stats_enable(0)
    med = {k: statistics.median(v) for k, v in t.items()}
    out = dict(reads=n_reads, paired=paired, reps=reps, response_bytes=int(resp_bytes), bam_bytes=int(bam.size), bam_bytes_per_read=bam.size / n_reads,
               ms_align=med["align"], ms_encode_bam=med["encode"], ms_download=med["download"], ms_final=med["ms_final"], ms_pack=med["ms_pack"],
               ms_final_plus_pack=med["final_plus_pack"], encode_le_final_plus_pack=bool(med["encode"] <= med["final_plus_pack"]),
               encode_GBps_output=bam.size / med["encode"] / 1e6, download_GBps=bam.size / med["download"] / 1e6,
               aligner_reads_per_s=n_reads / med["align"] * 1e3, all_runs_ms=t)
    if skip_host:
        return out
    have_z = True
    try:
        ctypes.CDLL("libz.so.1")
    except OSError:
        have_z = False
    out["libz"] = have_z
    for level in [0] + ([1] if have_z else []):
        secs, zbytes = [], 0
        for rep in range(reps + 1):
            n_out = sz()
            t0 = time.perf_counter()
            p = d.bwamem_hip_bgzf_compress(bam.ctypes.data_as(ctypes.c_char_p), bam.size, level, 16, 1, ctypes.byref(n_out))
            dt = time.perf_counter() - t0
            assert p
            lib._free(p)
            zbytes = n_out.value
            if rep:
                secs.append(dt)
        s = statistics.median(secs)
        out["bgzf_level%d" % level] = dict(threads=16, seconds=s, GBps_input=bam.size / s / 1e9, bytes=int(zbytes), reads_per_s=n_reads / s,
                                           keeps_up_with_aligner=bool(s * 1e3 <= med["align"]))
        # the whole path to a file: upload, align, encode, download, BGZF, write
        secs = []
        with tempfile.TemporaryDirectory() as tmp:
            for rep in range(reps + 1):
                fd = os.open(os.path.join(tmp, "out.bam"), os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
                t0 = time.perf_counter()
                rc = d.bwamem_hip_align_to_bam(h, ob, None, req, len(req), None, level, fd, 1)
                dt = time.perf_counter() - t0
                os.close(fd)
                assert rc == 0
                if rep:
                    secs.append(dt)
        s = statistics.median(secs)
        out["file_level%d" % level] = dict(seconds=s, reads_per_s=n_reads / s)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--genome-bp", type=int, default=3_000_000, help="the suite's medium genome by default (built from a FASTA file through jnibwa_createReferenceIndex; bench.py's 3.1 Gbp image needs its torch generators)")
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
    d.bwamem_hip_batch_result_bytes.restype = sz; d.bwamem_hip_batch_result_bytes.argtypes = [vp]
    d.bwamem_hip_batch_free.argtypes = [vp]; d.bwamem_hip_batch_free.restype = None
    d.bwamem_hip_batch_keep_offsets.argtypes = [vp, ctypes.c_int]
    d.bwamem_hip_batch_encode_bam.argtypes = [vp, ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(i64)]
    d.bwamem_hip_batch_bam_bytes.restype = sz; d.bwamem_hip_batch_bam_bytes.argtypes = [vp]
    d.bwamem_hip_batch_bam_download.argtypes = [vp, vp]
    d.bwamem_hip_bgzf_compress.restype = vp; d.bwamem_hip_bgzf_compress.argtypes = [ctypes.c_char_p, sz, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(sz)]
    d.bwamem_hip_align_to_bam.argtypes = [vp, vp, vp, ctypes.c_char_p, sz, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int]
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
        ev = Events()
        L = args.read_len
        g = np.frombuffer(b"".join(s for _, s in seqs), dtype=np.uint8)
        bounds = np.cumsum([0] + [len(s) for _, s in seqs])

        def starts(n, span):                                          # uniform over the contigs, never across a boundary
            ci = rng.integers(0, len(seqs), size=n)
            return bounds[ci] + (rng.random(n) * (np.diff(bounds)[ci] - span)).astype(np.int64)
        results = []
        if args.reads:
            rows = gather_reads(g, starts(args.reads, L), L, rng.random(args.reads) < 0.5, 0.01, rng)
            results.append(measure(lib, d, ev, h, request_of(rows), args.reads, False, args.reps, args.skip_host))
            del rows
        if args.pairs:
            isz = np.clip(rng.normal(400, 50, size=args.pairs), L, 1000).astype(np.int64)
            st = starts(args.pairs, 1001)
            none = np.zeros(args.pairs, dtype=bool)
            r1 = gather_reads(g, st, L, none, 0.01, rng)
            r2 = gather_reads(g, st + isz - L, L, ~none, 0.01, rng)
            rows = np.empty((2 * args.pairs, L), dtype=np.uint8)
            rows[0::2], rows[1::2] = r1, r2
            results.append(measure(lib, d, ev, h, request_of(rows), 2 * args.pairs, True, args.reps, args.skip_host))
        lib.destroy_index(h)
    doc = dict(what="BAM path rates (tests/gpu_units/bam_rate.py)", genome_bp=args.genome_bp, read_len=L, batches=results)
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({k: v for k, v in doc.items() if k != "batches"}))
    for r in results:
        print(json.dumps({k: v for k, v in r.items() if k != "all_runs_ms"}))


if __name__ == "__main__":
    main()
