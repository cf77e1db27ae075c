"""k_seed's probe phase (k_seed.hip: short SMEM candidates are probed one at a time before the row walk, and the ones that
cannot reach min_seed_len are dropped) against the oracle's interval lists and seeds, with the probe on and off.  The switch
is launch_seed's BWAMEM_HIP_SEED_PROBE, so every run here goes through launch_seed (useed_seed's mode 1).  Every comparison
is exact equality; n_ext (the extensions k_seed made) is read next to the results.  The emulation flavour runs in the CPU
suite, the hipcc flavour is its GPU twin at larger sizes.  SEED_PROBE_RECORD=<file> appends the counts to a JSON-lines file
(that is how profiles/seed_probe_n_ext.jsonl was made)."""
import ctypes
import json
import os

import numpy as np
import pytest

import bwalib as B
from test_units_seed import (CODE, Oracle, Units, _chimera, _compare_seed, _p, _pass2_candidates, _repeat_reads, _seed_reference,  # noqa: F401
                             _small_reads, emu_units, hip_units)


def _run(units, h, opts, reads, seeds_cap=1 << 21):
    """useed_seed through launch_seed -> (the arrays _compare_seed looks at, n_ext)"""
    n = len(reads)
    off = np.zeros(n + 1, dtype=np.int64); off[1:] = np.cumsum([len(r) + 1 for r in reads])
    req = b"".join(r + b"\0" for r in reads)
    max_len = max(len(r) for r in reads)
    intv_cap, smem_cap, grid = max(64, max_len + 8), max_len + 2, (n + 63) // 64
    ob = ctypes.create_string_buffer(bytes(opts), 168)
    n_intv, n_seeds, l_rep = (np.zeros(n, dtype=np.int32) for _ in range(3))
    intv = np.zeros((n, intv_cap, 3), dtype=np.uint64); iso = np.zeros((n, intv_cap), dtype=np.int32)
    seed_off = np.zeros(n + 1, dtype=np.int64)
    rbeg = np.zeros(seeds_cap, dtype=np.int64); qbeg, slen, rid = (np.zeros(seeds_cap, dtype=np.int32) for _ in range(3))
    err = np.zeros(1, dtype=np.int32); cnt = np.zeros(3, dtype=np.uint64)
    rc = units.dll.useed_seed(h, ob, n, req, _p(off), 1, 16, 4, 1, grid, intv_cap, smem_cap, _p(n_intv), _p(intv), _p(iso), _p(n_seeds), _p(l_rep), _p(seed_off),
                              seeds_cap, _p(rbeg), _p(qbeg), _p(slen), _p(rid), _p(err), _p(cnt))
    assert rc == 0, "useed_seed returned %d" % rc
    n_occ = int(seed_off[n])
    got = dict(n_intv=n_intv, intv=intv, iso=iso, n_seeds=n_seeds, l_rep=l_rep, seed_off=seed_off, rbeg=rbeg[:n_occ], qbeg=qbeg[:n_occ], slen=slen[:n_occ], rid=rid[:n_occ],
               err=int(err[0]), n_lf=int(cnt[1]), n_sa=int(cnt[2]))
    return got, int(cnt[0])


def _on_off(units, h, monkeypatch, opts, reads, ref, what):
    """both settings of the switch against the same reference -> (n_ext with the probe, n_ext without)"""
    monkeypatch.delenv("BWAMEM_HIP_SEED_PROBE", raising=False)
    on, ext_on = _run(units, h, opts, reads)
    _compare_seed(on, ref, (what, "probe"))
    monkeypatch.setenv("BWAMEM_HIP_SEED_PROBE", "0")
    off, ext_off = _run(units, h, opts, reads)
    monkeypatch.delenv("BWAMEM_HIP_SEED_PROBE")
    _compare_seed(off, ref, (what, "no probe"))
    return ext_on, ext_off


def _record(flavour, what, n_reads, ext_on, ext_off, **more):
    line = dict(flavour=flavour, case=what, reads=n_reads, n_ext_probe=ext_on, n_ext_no_probe=ext_off, **more)
    print(json.dumps(line))
    path = os.environ.get("SEED_PROBE_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(line) + "\n")


# ------------------------------------------------------------------------------------------ 1. small genome, simulated reads
def _check_small(units, oracle, small_genome, monkeypatch, n_sim, length):
    seqs, img = small_genome
    O = Oracle(oracle, img); h = units.open(img, 1)
    reads = _small_reads(seqs, n_sim, length)
    flavour = "emu" if units.emu else "gpu"
    # min_seed_len 70: beyond the candidate mask, no probing at all; split_factor 1.0: more pass-2 searches, min_intv > 1
    for kw in (dict(), dict(min_seed_len=12), dict(min_seed_len=30), dict(min_seed_len=70), dict(split_width=0), dict(max_mem_intv=0), dict(split_factor=1.0)):
        opts = B.set_opt(oracle.default_options(), **kw)
        ref = _seed_reference(O, opts, reads)
        ext_on, ext_off = _on_off(units, h, monkeypatch, opts, reads, ref, kw)
        _record(flavour, "small genome %s" % (kw or "default"), len(reads), ext_on, ext_off)
        if not kw:
            assert sum(len(iv) for iv in ref["intv"]) > n_sim
            assert ext_on < ext_off, "the probe saved nothing: %d extensions with it, %d without" % (ext_on, ext_off)
        if kw.get("min_seed_len") == 70:
            assert ext_on == ext_off, (ext_on, ext_off)
    units.close(h); O.close()


def test_units_seed_probe_emu_small(emu_units, oracle, small_genome, monkeypatch):
    _check_small(emu_units, oracle, small_genome, monkeypatch, 20, 70)


@pytest.mark.gpu
def test_units_seed_probe_gpu_small(hip_units, oracle, small_genome, monkeypatch):
    _check_small(hip_units, oracle, small_genome, monkeypatch, 400, 150)


# ------------------------------------------------------------------------------------------ 2. repeat genome
def _n_searches(O, opts, read):
    """bwt_smem1 calls of mem_collect_intv's first two loops.  Pass 1: every search emits at least its longest candidate and returns
    that one's end, which is where the next search starts; no match of another search contains the start (it would reach further
    than the forward walk from there did), so the matches of pass 1 alone, at min_seed_len 1, give the walk back.  Pass 2: one
    search per match that passes the split test (the middle of a match is never ambiguous)."""
    codes = CODE[np.frombuffer(read, dtype=np.uint8)]
    p1 = O.collect(B.set_opt(bytearray(opts), min_seed_len=1, split_width=0, max_mem_intv=0), codes)
    spans = [(info >> 32, info & 0xffffffff) for _, _, info in p1]
    x, n = 0, 0
    while x < len(codes):
        if codes[x] > 3:
            x += 1
            continue
        ends = [e for s, e in spans if s <= x < e]
        assert ends, "no match over position %d" % x
        x = max(ends); n += 1
    return n + _pass2_candidates(O, opts, read)


def _check_repeats(units, oracle, repeat_genome, monkeypatch, n_reads):
    """reads of a young repeat family: short candidates have many occurrences, probes are alive at min_seed_len and fall back to the
    row walk.  What a search can lose to that is the probe that is given up, min_seed_len - 1 extensions at the most."""
    seqs, img, starts = repeat_genome
    O = Oracle(oracle, img); h = units.open(img, 1)
    opts = oracle.default_options()
    reads = _repeat_reads(seqs, starts, n_reads, length=110, seed=9)
    g = seqs[0][1]
    for st in starts[:3]:                                                   # a substitution every 24 bases
        rd = bytearray(g[st + 20:st + 130])
        for p in range(12, len(rd), 24):
            rd[p] = ord("ACGT"[("ACGT".index(chr(rd[p])) + 1) % 4])
        reads.append(bytes(rd))
    ref = _seed_reference(O, opts, reads)
    assert any(size > 100 for iv in ref["intv"] for _, size, _ in iv)
    ext_on, ext_off = _on_off(units, h, monkeypatch, opts, reads, ref, "repeats")
    searches = sum(_n_searches(O, opts, r) for r in reads)
    _record("emu" if units.emu else "gpu", "repeat genome", len(reads), ext_on, ext_off, searches=searches)
    bound = ext_off + (B.get_opt(opts, "min_seed_len") - 1) * searches
    assert ext_on <= bound, "%d extensions with the probe, %d without, %d searches: more than %d" % (ext_on, ext_off, searches, bound)
    units.close(h); O.close()


def test_units_seed_probe_emu_repeats(emu_units, oracle, repeat_genome, monkeypatch):
    _check_repeats(emu_units, oracle, repeat_genome, monkeypatch, 10)


@pytest.mark.gpu
def test_units_seed_probe_gpu_repeats(hip_units, oracle, repeat_genome, monkeypatch):
    _check_repeats(hip_units, oracle, repeat_genome, monkeypatch, 150)


# ------------------------------------------------------------------------------------------ 3. edge reads
def _sub(read, p):
    rd = bytearray(read)
    rd[p] = ord("ACGT"[("ACGT".index(chr(rd[p]).upper()) + 1) % 4])
    return bytes(rd)


def _edge_reads(seqs, min_seed_len):
    g = seqs[0][1]
    assert b"N" not in g[5000:5400].upper() and b"N" not in g[9000:9200].upper()
    a = bytes(g[5000:5100])
    every5 = bytearray(a); every5[4::5] = b"N" * len(every5[4::5])
    every25 = bytearray(g[5200:5350]); every25[24::25] = b"N" * len(every25[24::25])
    reads = [b"N" + a[1:], b"NN" + a[2:60],                                  # the read starts with N: the first search has no base in front of it
             bytes(every5), bytes(every25),                                 # probes and rows that run into N
             a[:min_seed_len], a[:min_seed_len - 1], a[:min_seed_len + 1],  # exactly min_seed_len bases
             _sub(a, 1), _sub(a, 0), _sub(_sub(a, 1), 3),                    # the first mismatch at base 1: searches that start next to the read's start
             _chimera(g, 1, pieces=8, piece=20), _chimera(g, 3, pieces=7, piece=20) + bytes(g[9000:9060])]    # 20-base pieces: short candidates only
    return reads


def _check_edges(units, oracle, small_genome, monkeypatch):
    seqs, img = small_genome
    O = Oracle(oracle, img); h = units.open(img, 1)
    for kw in (dict(), dict(min_seed_len=12), dict(min_seed_len=20, split_factor=1.0)):
        opts = B.set_opt(oracle.default_options(), **kw)
        msl = B.get_opt(opts, "min_seed_len")
        reads = _edge_reads(seqs, msl)
        ref = _seed_reference(O, opts, reads)
        assert ref["intv"][2] == [] and ref["intv"][5] == [] and len(ref["intv"][4]) >= 1 and len(ref["intv"][0]) >= 1
        ext_on, ext_off = _on_off(units, h, monkeypatch, opts, reads, ref, ("edges", kw))
        _record("emu" if units.emu else "gpu", "edge reads %s" % (kw or "default"), len(reads), ext_on, ext_off)
    units.close(h); O.close()


def test_units_seed_probe_emu_edges(emu_units, oracle, small_genome, monkeypatch):
    _check_edges(emu_units, oracle, small_genome, monkeypatch)


@pytest.mark.gpu
def test_units_seed_probe_gpu_edges(hip_units, oracle, small_genome, monkeypatch):
    _check_edges(hip_units, oracle, small_genome, monkeypatch)
