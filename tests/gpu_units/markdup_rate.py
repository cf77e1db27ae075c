"""Rate of duplicate marking on the device next to the steps around it, on the batches of sort_rate.py (the same
generator and seed) with 10 % of the templates repeated and seeded base qualities: for a single-end and a paired-end batch resident
in HBM it times, in one process, bwamem_hip_batch_align, _encode_bam, _mark_duplicates, _sort_bam, _compress_bam and _index_bam,
each by HIP events and by the host clock, and the marked, sorted and indexed file call against the sorted one.  Every figure is the
median of --reps runs after one warm-up run of the same shape.  In the same run the marked records are compared, once, with the rule
of csrc/bam_dup.h restated in Python (mark_py below).  Two conditions, both relative and measured here: (i) _mark_duplicates plus
_sort_bam plus _index_bam take no longer than _compress_bam of the same batch; (ii) with marking off, _encode_bam, _sort_bam and the
sorted file call are within the run-to-run spread of the parent commit's library (--parent-lib), timed alternately in this process.
Kernel times proper: run under rocprofv3 --kernel-trace --stats with --skip-files, in a run of its own.  Needs a GPU; there is no
fallback.
usage: markdup_rate.py [--reads N] [--pairs N] [--genome-bp N] [--reps K] [--out FILE.json] [--skip-files] [--skip-check] [--parent-lib LIB.so]"""
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
sys.path.insert(0, HERE)
import bam_rate as R  # noqa: E402  (the batch generator, the event timer)
from sort_rate import both  # noqa: E402
B = R.B

COUNT_NAMES = ["unpaired_reads_examined", "read_pairs_examined", "secondary_or_supplementary", "unmapped_reads", "unpaired_read_duplicates",
               "read_pair_duplicates"]
_SCORE = bytes(b if 15 <= b != 0xff else 0 for b in range(256))


class DupCounts(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in COUNT_NAMES]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n in COUNT_NAMES}


def mark_py(bam, paired):
    """the rule at the top of csrc/bam_dup.h on the records of a batch with its default names (the records of a read are the
    consecutive ones with its name and first / second flag; a template is a name) -> (the marked bytes, the counts)"""
    counts = dict.fromkeys(COUNT_NAMES, 0)
    frags, pairs, places, ends = {}, {}, [], []
    off, t, prev_name, n = 0, -1, None, len(bam)

    def close(t, ends):
        if paired and len(ends) == 2:
            pairs.setdefault(tuple(sorted(e for e, _ in ends)), []).append((-(ends[0][1] + ends[1][1]), t))
    while off < n:
        size, refid, pos, l_name, _, _, n_cig, flag, l_seq = struct.unpack_from("<iiiBBHHHi", bam, off)
        name = bam[off + 36:off + 36 + l_name]
        if name != prev_name:
            close(t, ends)
            t, prev_name, ends = t + 1, name, []
            places.append([])
        places[t].append(off)
        if flag & 0x900:
            counts["secondary_or_supplementary"] += 1
        elif flag & 4:
            counts["unmapped_reads"] += 1
        else:
            cig = struct.unpack_from("<%dI" % n_cig, bam, off + 36 + l_name)
            if flag & 0x10:
                u, k = pos - 1 + sum(c >> 4 for c in cig if c & 15 in (0, 2, 3, 7, 8)), n_cig
                while k > 1 and cig[k - 1] & 15 in (4, 5):
                    u, k = u + (cig[k - 1] >> 4), k - 1
            else:
                u, k = pos, 0
                while k < n_cig and cig[k] & 15 in (4, 5):
                    u, k = u - (cig[k] >> 4), k + 1
            q = off + 36 + l_name + 4 * n_cig + (l_seq + 1) // 2
            score = min(sum(bam[q:q + l_seq].translate(_SCORE)), 16383)
            end = (refid, u, 1 if flag & 0x10 else 0)
            is_paired = bool(flag & 1) and not flag & 8
            ends.append((end, score))
            frags.setdefault(end, []).append((0 if is_paired else 1, -score, t))
            counts["unpaired_reads_examined"] += not is_paired
        off += 4 + size
    close(t, ends)
    dup = set()
    for g in pairs.values():
        counts["read_pairs_examined"] += len(g)
        for _, t in sorted(g)[1:]:
            dup.add(t)
            counts["read_pair_duplicates"] += 1
    for g in frags.values():
        g.sort()
        for k, (alone, _, t) in enumerate(g):
            if alone and k:
                dup.add(t)
                counts["unpaired_read_duplicates"] += 1
    out = bytearray(bam)
    for t, offs in enumerate(places):
        for o in offs:
            out[o + 19] = (out[o + 19] & ~4) | (4 if t in dup else 0)
    return bytes(out), counts


def measure(lib, d, ev, h, parent, req, quals, n_reads, paired, reps, skip_files, skip_check):
    sz = ctypes.c_size_t
    opts = B.set_opt(lib.default_options(), flag=B.MEM_F_PE if paired else 0)
    ob = ctypes.create_string_buffer(bytes(opts), B.OPT_SIZE)
    pe = 1 if paired else 0

    def batch(dd, hh):
        b = dd.bwamem_hip_batch_upload(hh, req, len(req))
        assert b and dd.bwamem_hip_batch_keep_offsets(b, 1) == 0 and dd.bwamem_hip_batch_set_qualities(b, quals, len(quals)) == 0
        return b
    b = batch(d, h)
    steps = ("align", "encode", "mark", "sort", "compress", "index")
    t = {k + "_" + c: [] for k in steps for c in ("events", "wall")}
    plain = marked = None
    c = DupCounts()
    for rep in range(reps + 1):                                   # rep 0 warms every shape up
        row = []
        rc, ms, wall = both(ev, lambda: d.bwamem_hip_batch_align(h, ob, None, b, 0)); assert rc == 0; row += [ms, wall]
        rc, ms, wall = both(ev, lambda: d.bwamem_hip_batch_encode_bam(b, pe, None, None)); assert rc == 0; row += [ms, wall]
        m = d.bwamem_hip_batch_bam_bytes(b)
        if plain is None and not skip_check:
            plain = np.empty(m, dtype=np.uint8)
            assert d.bwamem_hip_batch_bam_download(b, plain.ctypes.data) == 0
        rc, ms, wall = both(ev, lambda: d.bwamem_hip_batch_mark_duplicates(b, pe, ctypes.byref(c))); assert rc == 0; row += [ms, wall]
        if marked is None and not skip_check:
            marked = np.empty(m, dtype=np.uint8)
            assert d.bwamem_hip_batch_bam_download(b, marked.ctypes.data) == 0
        rc, ms, wall = both(ev, lambda: d.bwamem_hip_batch_sort_bam(b)); assert rc == 0; row += [ms, wall]
        rc, ms, wall = both(ev, lambda: d.bwamem_hip_batch_compress_bam(b, 1)); assert rc == 0; row += [ms, wall]
        n_out = sz()
        p, ms, wall = both(ev, lambda: d.bwamem_hip_batch_index_bam(b, 0, ctypes.byref(n_out))); assert p; row += [ms, wall]
        lib._free(p)
        if rep:
            for k, v in zip(t, row):
                t[k].append(v)
    med = {k: statistics.median(v) for k, v in t.items()}
    total = med["mark_wall"] + med["sort_wall"] + med["index_wall"]
    out = dict(reads=n_reads, paired=paired, reps=reps, bam_bytes=int(m), counts=c.as_dict(), **{"ms_" + k: v for k, v in med.items()},
               ms_mark_plus_sort_plus_index_wall=total, mark_sort_index_within_compress=bool(total <= med["compress_wall"]), all_runs_ms=t)
    if not skip_check:
        want, counts = mark_py(plain.tobytes(), paired)
        assert marked.tobytes() == want and c.as_dict() == counts, "the marked records are not the rule's"
        out["marks_checked"] = True
    # ---- (ii) marking off: this build and the parent's, alternately, on batches of their own
    if parent:
        plib, pd, ph = parent
        pb = batch(pd, ph)
        assert d.bwamem_hip_batch_align(h, ob, None, b, 0) == 0 and pd.bwamem_hip_batch_align(ph, ob, None, pb, 0) == 0
        u = {k: [] for k in ("encode", "encode_parent", "sort", "sort_parent")}
        for rep in range(reps + 1):
            for who in (("this", "parent"), ("parent", "this"))[rep & 1]:      # alternating: whichever runs second finds the device busy already
                dd, bb, sfx = (d, b, "") if who == "this" else (pd, pb, "_parent")
                rc, ms, _ = both(ev, lambda: dd.bwamem_hip_batch_encode_bam(bb, pe, None, None)); assert rc == 0
                rc2, ms2, _ = both(ev, lambda: dd.bwamem_hip_batch_sort_bam(bb)); assert rc2 == 0
                if rep:
                    u["encode" + sfx].append(ms); u["sort" + sfx].append(ms2)
        pd.bwamem_hip_batch_free(pb)
        for k in ("encode", "sort"):
            a, p = u[k], u[k + "_parent"]
            out["off_" + k] = dict(this_ms=statistics.median(a), parent_ms=statistics.median(p), spread_ms=dict(this=max(a) - min(a), parent=max(p) - min(p)),
                                   not_slower_than_parent=bool(statistics.median(a) - statistics.median(p) <= max(max(a) - min(a), max(p) - min(p))), runs=dict(this=a, parent=p))
    d.bwamem_hip_batch_free(b)
    if skip_files:
        return out
    with tempfile.TemporaryDirectory() as tmp:
        path, bpath = os.path.join(tmp, "out.bam"), os.path.join(tmp, "out.bam.bai")
        calls = [("file_sorted_indexed", lambda fd, fb: d.bwamem_hip_align_to_sorted_bam(h, ob, None, req, len(req), None, fd, fb, 1)),
                 ("file_marked_sorted_indexed", lambda fd, fb: d.bwamem_hip_align_to_marked_bam(h, ob, None, req, len(req), None, 1, fd, fb, 1, None))]
        if parent:
            calls.append(("file_sorted_indexed_parent", lambda fd, fb: parent[1].bwamem_hip_align_to_sorted_bam(parent[2], ob, None, req, len(req), None, fd, fb, 1)))
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
        out["file_marked_extra_ms"] = (out["file_marked_sorted_indexed"]["seconds"] - out["file_sorted_indexed"]["seconds"]) * 1e3
        if parent:
            a, p = out["file_sorted_indexed"], out["file_sorted_indexed_parent"]
            out["file_sorted_not_slower_than_parent"] = bool(a["seconds"] - p["seconds"] <= max(a["spread_s"], p["spread_s"]))
    return out


def bind(d):
    vp, sz, i64, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int64, ctypes.c_int
    d.bwamem_hip_batch_upload.restype = vp; d.bwamem_hip_batch_upload.argtypes = [vp, ctypes.c_char_p, sz]
    d.bwamem_hip_batch_align.argtypes = [vp, vp, vp, vp, i64]
    d.bwamem_hip_batch_free.argtypes = [vp]; d.bwamem_hip_batch_free.restype = None
    d.bwamem_hip_batch_keep_offsets.argtypes = [vp, ci]
    d.bwamem_hip_batch_set_qualities.argtypes = [vp, ctypes.c_char_p, sz]
    d.bwamem_hip_batch_encode_bam.argtypes = [vp, ci, ctypes.c_char_p, ctypes.POINTER(i64)]
    d.bwamem_hip_batch_bam_bytes.restype = sz; d.bwamem_hip_batch_bam_bytes.argtypes = [vp]
    d.bwamem_hip_batch_bam_download.argtypes = [vp, vp]
    d.bwamem_hip_batch_sort_bam.argtypes = [vp]
    d.bwamem_hip_batch_compress_bam.argtypes = [vp, ci]
    d.bwamem_hip_batch_index_bam.restype = vp; d.bwamem_hip_batch_index_bam.argtypes = [vp, i64, ctypes.POINTER(sz)]
    d.bwamem_hip_align_to_sorted_bam.argtypes = [vp, vp, vp, ctypes.c_char_p, sz, vp, ci, ci, ci]
    if hasattr(d, "bwamem_hip_batch_mark_duplicates"):
        d.bwamem_hip_batch_mark_duplicates.argtypes = [vp, ci, ctypes.POINTER(DupCounts)]
        d.bwamem_hip_align_to_marked_bam.argtypes = [vp, vp, vp, ctypes.c_char_p, sz, vp, ci, ci, ci, ci, ctypes.POINTER(DupCounts)]
    d.jnibwa_createReferenceIndex.argtypes = [ctypes.c_char_p] * 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--genome-bp", type=int, default=3_000_000, help="the suite's medium genome, as sort_rate.py")
    ap.add_argument("--reps", type=int, default=4, help="even, so that the two orders of the parent comparison are timed equally often")
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-files", action="store_true", help="batch figures only (the profiler run)")
    ap.add_argument("--skip-check", action="store_true", help="do not compare the marks with the rule in Python (the profiler run)")
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
            results.append(measure(lib, d, ev, h, parent, R.request_of(rows), quals_of(args.reads), args.reads, False, args.reps, args.skip_files, args.skip_check))
            del rows
        if args.pairs:
            isz = repeat(np.clip(rng.normal(400, 50, size=args.pairs), L, 1000).astype(np.int64))
            st = repeat(starts(args.pairs, 1001))
            none = np.zeros(args.pairs, dtype=bool)
            r1 = R.gather_reads(g, st, L, none, 0.01, rng)
            r2 = R.gather_reads(g, st + isz - L, L, ~none, 0.01, rng)
            rows = np.empty((2 * args.pairs, L), dtype=np.uint8)
            rows[0::2], rows[1::2] = r1, r2
            results.append(measure(lib, d, ev, h, parent, R.request_of(rows), quals_of(2 * args.pairs), 2 * args.pairs, True, args.reps, args.skip_files, args.skip_check))
        lib.destroy_index(h)
        if parent:
            plib.destroy_index(parent[2])
    doc = dict(what="duplicate marking on the device next to encode, sort, compress and index (tests/gpu_units/markdup_rate.py)", genome_bp=args.genome_bp,
               read_len=L, repeated_fraction=0.1, parent_lib_measured=bool(plib), batches=results)
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({k: v for k, v in doc.items() if k != "batches"}))
    for r in results:
        print(json.dumps({k: v for k, v in r.items() if not k.startswith("all_runs_ms")}))


if __name__ == "__main__":
    main()
