"""Rates of compressed FASTQ in (csrc/bgzf_inflate.h) on the batches of fastq_rate.py (the same generator and seed), as
BGZF at zlib level 6 in members of 0xff00 bytes of text, under two quality models: seeded uniform 33..126 (the worst case for any
compressor) and four binned values with runs (nearer what current sequencers write).  In one process, per batch and model:
  * bwamem_hip_batch_upload_fastq_gz of the streams: compressed upload, inflate kernel, parse;
  * what a caller would do otherwise: sixteen host threads inflating the same members with zlib, then bwamem_hip_batch_upload_fastq
    of the text.  The threads are Python's, around zlib.decompress (one call per member, which releases the interpreter lock while
    it inflates); the join of the pieces is not timed.  It is this harness's figure, not the best a native thread pool could do;
  * bwamem_hip_batch_upload_fastq of the plain text, this build and -- with --parent-lib -- the parent commit's, alternating, and
    with --files bwamem_hip_align_fastq_to_bam the same way: nothing existing may have moved.
Every figure is the median of --reps runs after one warm-up, by HIP events and by the host clock.  The inflate kernel's device time
is the difference of the library's per-launch HIP-event time (bwamem_hip_stats: ms_other) between the gz upload and the plain
upload of the same text; kernel times proper: fastq_gz_rate.sh runs this script under rocprofv3 --kernel-trace --stats in a run of
its own, each step under its own time limit.  The batches of the
gz path are compared with the plain path's (offsets and payload sizes) once.  Needs a GPU; there is no fallback.
usage: fastq_gz_rate.py [--reads N] [--pairs N] [--genome-bp N] [--reps K] [--out FILE.json] [--files] [--parent-lib LIB.so]"""
import argparse
import ctypes
import json
import os
import struct
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fastq_rate as F  # noqa: E402  (bindings, text builder, the event timer of bam_rate.py)
R, B = F.R, F.B
BLOCK, THREADS = 0xff00, 16


def member(piece):
    o = zlib.compressobj(6, zlib.DEFLATED, -15, 9)
    dfl = o.compress(piece) + o.flush()
    return b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(dfl) + 25) + dfl + struct.pack("<II", zlib.crc32(piece), len(piece))


def bgzf(pool, text):
    ms = list(pool.map(member, (text[at:at + BLOCK] for at in range(0, len(text), BLOCK))))
    return b"".join(ms) + bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0]), ms


def host_inflate(pool, ms):
    return list(pool.map(lambda m: zlib.decompress(m[18:-8], -15, BLOCK), ms))       # (one call per member, the output buffer sized at once)


def quals_of(model, n, L, rng):
    if model == "uniform":
        return rng.integers(33, 127, size=(n, L), dtype=np.uint8)
    runs = rng.choice(np.frombuffer(b"#5AF", dtype=np.uint8), size=(n, (L + 9) // 10), p=[0.04, 0.08, 0.18, 0.7])
    return np.repeat(runs, 10, axis=1)[:, :L].copy()


def measure(new, parent, ev, pool, rows, paired, model, reps, files):
    lib, d, h = new
    n, L = rows.shape
    quals = quals_of(model, n, L, np.random.default_rng(0xF0))
    names = F.names_of(n, 2 if paired else 1)
    if paired:
        texts = [F.fastq_of(rows[0::2], quals[0::2], names[0::2]), F.fastq_of(rows[1::2], quals[1::2], names[1::2])]
    else:
        texts = [F.fastq_of(rows, quals, names)]
    zs, members = zip(*[bgzf(pool, t) for t in texts])
    t2, z2 = (texts[1], zs[1]) if paired else (None, None)
    n2, nz2 = (len(t2), len(z2)) if paired else (0, 0)
    out = dict(reads=n, paired=paired, quality_model=model, reps=reps, text_bytes=sum(map(len, texts)), bgzf_bytes=sum(map(len, zs)), members=sum(map(len, members)))
    stats = F.Stats()
    bad, bm = ctypes.c_int64(), ctypes.c_int64()

    def other_ms(fn):
        d.bwamem_hip_stats_get(ctypes.byref(stats)); a = stats.ms_other
        r = fn()
        d.bwamem_hip_stats_get(ctypes.byref(stats))
        return r, stats.ms_other - a
    keys = ("upload_fastq_gz", "host_inflate_16", "upload_fastq", "upload_fastq_parent", "kernels_gz", "kernels_plain")
    t = {k: [] for k in keys}
    for rep in range(reps + 1):                                       # rep 0 warms every shape up
        row = {}
        (b, ko), ms, wall = F.both(ev, lambda: other_ms(lambda: d.bwamem_hip_batch_upload_fastq_gz(h, zs[0], len(zs[0]), z2, nz2, ctypes.byref(bad), ctypes.byref(bm))))
        assert b, (bad.value, bm.value)
        row["upload_fastq_gz"], row["kernels_gz"] = wall, ko
        t0 = time.perf_counter()
        pieces = [host_inflate(pool, m) for m in members]
        row["host_inflate_16"] = (time.perf_counter() - t0) * 1e3
        if rep == 0:
            assert [b"".join(p) for p in pieces] == texts
        del pieces
        for who in (("this", "parent"), ("parent", "this"))[rep & 1]:
            if who == "this":
                (b2, ko), ms, wall = F.both(ev, lambda: other_ms(lambda: d.bwamem_hip_batch_upload_fastq(h, texts[0], len(texts[0]), t2, n2, ctypes.byref(bad))))
                assert b2
                row["upload_fastq"], row["kernels_plain"] = wall, ko
            elif parent:
                pd, ph = parent[1], parent[2]
                pb, ms, wall = F.both(ev, lambda: pd.bwamem_hip_batch_upload_fastq(ph, texts[0], len(texts[0]), t2, n2, ctypes.byref(bad)))
                assert pb
                row["upload_fastq_parent"] = wall
                pd.bwamem_hip_batch_free(pb)
        d.bwamem_hip_batch_free(b); d.bwamem_hip_batch_free(b2)
        print("%s %s rep %d %s" % ("pairs" if paired else "reads", model, rep, {k: round(v, 2) for k, v in row.items()}), file=sys.stderr, flush=True)
        if rep:
            for k, v in row.items():
                t[k].append(v)
    for k, v in t.items():
        if v:
            out[k + "_ms"] = dict(median=F.med(v), all=v)
    inflate_ms = out["kernels_gz_ms"]["median"] - out["kernels_plain_ms"]["median"]
    out["inflate_kernel_ms"] = inflate_ms
    out["inflate_text_GB_per_s"] = out["text_bytes"] / inflate_ms / 1e6 if inflate_ms > 0 else None
    out["alternative_ms"] = out["host_inflate_16_ms"]["median"] + out["upload_fastq_ms"]["median"]
    out["condition_ii_device_path_is_lower"] = bool(out["upload_fastq_gz_ms"]["median"] < out["alternative_ms"])
    if parent:
        pv = out["upload_fastq_parent_ms"]["all"]
        out["condition_i_upload_within_parent_spread"] = bool(out["upload_fastq_ms"]["median"] <= max(pv))
    if files:
        opts = B.set_opt(lib.default_options(), flag=B.MEM_F_PE if paired else 0)
        ob = ctypes.create_string_buffer(bytes(opts), B.OPT_SIZE)
        calls = [("file_fastq", lambda fd: d.bwamem_hip_align_fastq_to_bam(h, ob, None, texts[0], len(texts[0]), t2, n2, None, 0, fd, -1, 1)),
                 ("file_fastq_gz", lambda fd: d.bwamem_hip_align_fastq_gz_to_marked_bam(h, ob, None, zs[0], len(zs[0]), z2, nz2, None, 0, fd, -1, 1, 0, None))]
        if parent:
            calls.append(("file_fastq_parent", lambda fd: parent[1].bwamem_hip_align_fastq_to_bam(parent[2], ob, None, texts[0], len(texts[0]), t2, n2, None, 0, fd, -1, 1)))
        secs = {k: [] for k, _ in calls}
        with tempfile.TemporaryDirectory() as tmp:
            for rep in range(reps + 1):
                for key, call in (calls if rep & 1 else calls[::-1]):
                    fd = os.open(os.path.join(tmp, "o.bam"), os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
                    t0 = time.perf_counter()
                    rc = call(fd)
                    dt = time.perf_counter() - t0
                    os.close(fd)
                    assert rc == 0
                    if rep:
                        secs[key].append(dt)
        for k, v in secs.items():
            out[k + "_s"] = dict(median=F.med(v), all=v)
        if parent:
            out["condition_i_file_within_parent_spread"] = bool(out["file_fastq_s"]["median"] <= max(out["file_fastq_parent_s"]["all"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--genome-bp", type=int, default=3_000_000)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--out", default=None)
    ap.add_argument("--files", action="store_true", help="time the file calls as well")
    ap.add_argument("--parent-lib", default=None, help="libbwamem_hip.so of the parent commit, timed in the same process")
    args = ap.parse_args()
    lib = B.product_lib()
    d = lib.dll
    d.bwamem_hip_device_count.restype = ctypes.c_int
    assert d.bwamem_hip_device_count() > 0, "no GPU: this script measures on the device only"
    F.bind(d, True)
    vp, sz, cp, ci, i64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_int, ctypes.c_int64
    d.bwamem_hip_batch_upload_fastq_gz.restype = vp
    d.bwamem_hip_batch_upload_fastq_gz.argtypes = [vp, cp, sz, cp, sz, ctypes.POINTER(i64), ctypes.POINTER(i64)]
    d.bwamem_hip_align_fastq_gz_to_marked_bam.argtypes = [vp, vp, vp, cp, sz, cp, sz, cp, ci, ci, ci, ci, ci, vp]
    d.bwamem_hip_stats_enable(1)
    plib = None
    if args.parent_lib:
        plib = B.Lib(args.parent_lib, "jnibwa_")
        F.bind(plib.dll, True)
    rng = np.random.default_rng(0xBA4)
    pool = ThreadPoolExecutor(THREADS)
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

        def starts(n, span):
            ci_ = rng.integers(0, len(seqs), size=n)
            return bounds[ci_] + (rng.random(n) * (np.diff(bounds)[ci_] - span)).astype(np.int64)
        results = []
        if args.reads:
            rows = R.gather_reads(g, starts(args.reads, L), L, rng.random(args.reads) < 0.5, 0.01, rng)
            results += [measure((lib, d, h), parent, ev, pool, rows, False, model, args.reps, args.files) for model in ("uniform", "binned")]
            del rows
        if args.pairs:
            isz = np.clip(rng.normal(400, 50, size=args.pairs), L, 1000).astype(np.int64)
            st = starts(args.pairs, 1001)
            none = np.zeros(args.pairs, dtype=bool)
            rows = np.empty((2 * args.pairs, L), dtype=np.uint8)
            rows[0::2], rows[1::2] = R.gather_reads(g, st, L, none, 0.01, rng), R.gather_reads(g, st + isz - L, L, ~none, 0.01, rng)
            results += [measure((lib, d, h), parent, ev, pool, rows, True, model, args.reps, args.files) for model in ("uniform", "binned")]
        lib.destroy_index(h)
        if parent:
            plib.destroy_index(parent[2])
    doc = dict(what="compressed FASTQ in: BGZF members inflated on the device against sixteen host threads of zlib (tests/gpu_units/fastq_gz_rate.py)",
               genome_bp=args.genome_bp, read_len=L, host_threads=THREADS, parent_lib_measured=bool(plib), batches=results)
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
