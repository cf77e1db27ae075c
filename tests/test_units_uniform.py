"""The wave-per-read DP kernels keep their wave-uniform state scalar (wave_ops.h: wave_uni and the uniform reductions).  The
unit wrapper of the extension only reaches extend_any; the outer loops of extend_read (which seed, covered test, forced
extension, band retries) and the retry loop of k_gcigar are reached end to end only, so this file drives constructed reads
through jnibwa_createAlignments and compares every record with the oracle, byte for byte.  The emulation flavour runs in the
CPU suite: there every uniform helper is a rendezvous of the wave's 64 fibres, so a call that one lane misses fails here and
not on a GPU.  Each read set runs twice: plain, and with BWAMEM_HIP_DEBUGK=256 (no diagonal certificate: every extension goes
through the DP rows)."""
import ctypes
import os

import numpy as np
import pytest

import bwalib as B

L = 150
NEXT = {65: 67, 67: 71, 71: 84, 84: 65}


def _reference():
    """80 kbp of seeded i.i.d. sequence; bases 50000..52000 are a 3 % diverged copy of bases 10000..12000"""
    rng = np.random.default_rng(0x0D1F)
    g = rng.integers(0, 4, size=80000, dtype=np.uint8)
    seg = g[10000:12000].copy()
    mut = rng.random(2000) < 0.03
    seg[mut] = (seg[mut] + rng.integers(1, 4, size=int(mut.sum()), dtype=np.uint8)) % 4
    g[50000:52000] = seg
    return B.BASES[g].tobytes()


def _mut(rd, positions, n_at=()):
    rd = bytearray(rd)
    for p in positions:
        rd[p] = NEXT[rd[p]]
    for p in n_at:
        rd[p] = 78
    return bytes(rd)


def _edge_read(g, p, q, side, extra, rng, with_n=False):
    """150 bases at p whose longest exact stretch leaves a query of q bases to the left (side 0) or right (side 1) extension:
    a substitution next to the seed, `extra` more in the extended part, and -- where that part is longer than the seed --
    one every 17 bases so that it holds no seed of its own"""
    rd = g[p:p + L]
    ext = list(range(q - 1, -1, -1)) if side == 0 else list(range(L - q, L))      # from the seed outwards
    pos = [ext[0]]
    if q - 1 >= L - q - 1:
        pos += ext[17::17]
    free = [x for x in ext[1:] if x not in pos]
    if extra and free:
        pos += [int(x) for x in rng.choice(free, size=min(extra, len(free)), replace=False)]
    n_at = [free[len(free) // 2]] if with_n and len(free) > 2 else []
    return _mut(rd, pos, n_at)


def _short_reads(g):
    rng = np.random.default_rng(77)
    reads = []
    spots = (3000, 31007)
    for k, p in enumerate(spots):
        for side in (0, 1):
            for q in (1, 62, 63, 64, 65, 126, 127, 128):
                for extra in ((0, 1, 2, 4) if 60 < q < 70 else (0,)):                 # 1, 2, 3 and 5 substitutions in the extended part
                    rd = _edge_read(g, p + 13 * q, q, side, extra, rng)
                    reads.append(rd if (q + extra + k) % 2 else B.revcomp(rd))
            for q in (64, 126):
                reads.append(_edge_read(g, p + 501, q, side, 1, rng, with_n=True))
        reads.append(g[p + 900:p + 900 + L])                                           # the seed spans the read: no extension at all
        reads.append(B.revcomp(g[p + 1100:p + 1100 + L]))
    # a deletion and an insertion of 20 .. 40 bases about 90 bases from the seed (the region's global alignment then needs a wide band)
    for k, n in enumerate((20, 30, 40)):
        p = 20000 + 400 * k
        rd = g[p:p + 25] + g[p + 25 + n:p + 25 + n + 125]                                  # deletion; the seed is the right end
        reads.append(_mut(rd, [25 + 17 * x for x in range(1, 6)]))
        ins = B.BASES[rng.integers(0, 4, size=n)].tobytes()
        rd = g[p + 200:p + 225] + ins + g[p + 225:p + 225 + (125 - n)]                   # insertion
        reads.append(_mut(rd, [25 + n + 17 * x for x in range(1, 4)]))
    # the duplicated segment: two chains; the second seed of the better chain is already covered, and forced-extension candidates exist
    for off in (300, 900, 1500):
        reads.append(g[10000 + off:10000 + off + L])
        reads.append(_mut(B.revcomp(g[50000 + off:50000 + off + L]), [40, 41, 100]))
    reads.append(B.BASES[np.random.default_rng(5).integers(0, 4, size=L)].tobytes())   # no chain
    reads.append(b"N" * 40)
    # global-alignment jobs: 3, 4, 5 and 8 substitutions (lane form and its limits), indels of 1, 5, 17 and 30 bases (one- and
    # two-chunk wave forms, a band-doubling retry)
    for k, ns in enumerate((3, 4, 5, 8)):
        p = 40000 + 300 * k
        reads.append(_mut(g[p:p + L], [int(x) for x in np.linspace(20, 130, ns).astype(int)]))
    for k, n in enumerate((1, 5, 17, 30)):
        p = 60000 + 500 * k
        reads.append(g[p:p + 70] + g[p + 70 + n:p + 70 + n + 80])
        reads.append(B.revcomp(g[p + 200:p + 270] + B.BASES[rng.integers(0, 4, size=n)].tobytes() + g[p + 270:p + 270 + 80 - n]))
        reads.append(_mut(g[p + 300:p + 360] + g[p + 360 + n:p + 360 + n + 90], [10, 100, 140]))
    return reads


RETRY_AT, RETRY_A, RETRY_DEL, RETRY_B = 70000, 100, 80, 150


def _retry_read(g):
    """100 bases, an 80-base deletion, 150 bases: the left extension of the right part (the longer seed) crosses the deletion --
    its 150 pay for the gap and the 100 matches behind it win that back -- so its best cell lies 80 columns off the diagonal.
    That is >= 3/4 of the band of 100, and the second band try (200) runs.  (With the default scores this needs more than 81
    bases on either side of the gap: no 150-base read gets there, which is why _run also aligns the short reads with w = 40.)"""
    p = RETRY_AT
    return g[p:p + RETRY_A] + g[p + RETRY_A + RETRY_DEL:p + RETRY_A + RETRY_DEL + RETRY_B]


def _long_reads(g):
    rng = np.random.default_rng(78)
    reads = []
    for k, n in enumerate((191, 192, 250, 250)):
        p = 5000 + 700 * k
        reads.append(_mut(g[p:p + n], [int(x) for x in rng.choice(n, size=3 + k, replace=False)]))
        reads.append(B.revcomp(_mut(g[p + 300:p + 300 + n], [n // 2])))
    reads.append(_retry_read(g))
    p = 72000                                                                           # the same with an 80-base insertion between two 100-base parts
    reads.append(g[p:p + 100] + B.BASES[rng.integers(0, 4, size=80)].tobytes() + g[p + 100:p + 200])
    reads.append(g[p + 400:p + 500] + g[p + 530:p + 680])                                 # a 30-base deletion in a 250-base read
    return reads


def _code(s):
    return bytes(b"ACGT".index(c) if c in b"ACGT" else 4 for c in s)


def _check_retry_case(oracle, g):
    """the oracle's ksw_extend2 on the left extension of the retry read at the first band: max_off >= 3/4 w, i.e. mem_chain2aln
    runs the second try and the region's w is 200"""
    oext = oracle.dll.o_ksw_extend2
    oext.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p] + [ctypes.c_int] * 8 + [ctypes.c_void_p] * 5
    opts = oracle.default_options()
    w = B.get_opt(opts, "w")
    assert w == 100
    q = _code(g[RETRY_AT:RETRY_AT + RETRY_A][::-1])
    tgt = _code(g[RETRY_AT - 60:RETRY_AT + RETRY_A + RETRY_DEL][::-1])
    out = (ctypes.c_int * 5)()
    sc = oext(len(q), q, len(tgt), tgt, 5, bytes(opts[140:165]), 6, 1, 6, 1, w, 5, 100, RETRY_B,
              ctypes.byref(out, 0), ctypes.byref(out, 4), ctypes.byref(out, 8), ctypes.byref(out, 12), ctypes.byref(out, 16))
    assert sc > RETRY_B and out[4] >= (w >> 1) + (w >> 2), (sc, list(out))


def _index(lib, workdir, name, g):
    fa = os.path.join(workdir, name + ".fa")
    img = fa + ".img"
    if not os.path.exists(img):
        B.write_fasta(fa, [("chrU", g)])
        build = lib.dll.jnibwa_createReferenceIndex
        build.argtypes = [ctypes.c_char_p] * 3
        assert build(fa.encode(), fa.encode(), b"auto") == 0
        assert lib.create_index_file(fa, img) == 0
    return img


def _run(lib, oracle, workdir, name, monkeypatch):
    g = _reference()
    _check_retry_case(oracle, g)
    img = _index(lib, workdir, name, g)
    h, ho = lib.open_index(img), oracle.open_index(img)
    opts = lib.default_options()
    try:
        short, long_ = _short_reads(g), _long_reads(g)
        assert max(len(r) for r in short) == L and max(len(r) for r in long_) > 191
        # separate calls: the tile of the long reads takes k_extend, not k_extend_short.  w = 40: the 30- and 40-base gaps of the short
        # reads lie >= 3/4 w off the diagonal, so k_extend_short's band retries run as well
        for reads, w in ((short, 100), (long_, 100), (short[-60:], 40)):
            opts = B.set_opt(lib.default_options(), w=w)
            req = B.pack_request(reads)
            want = oracle.align_raw(ho, opts, req)
            recs = B.decode_response(want, len(reads))
            assert sum(1 for r in recs if r and not r[0]["flag"] & 4) >= len(reads) - 3    # (all but the random reads are placed)
            for debugk in (None, "256"):
                if debugk:
                    monkeypatch.setenv("BWAMEM_HIP_DEBUGK", debugk)
                else:
                    monkeypatch.delenv("BWAMEM_HIP_DEBUGK", raising=False)
                got = lib.align_raw(h, opts, req)
                assert got is not None
                if got != want:
                    a, b = B.split_response(got, len(reads)), B.split_response(want, len(reads))
                    bad = [i for i in range(len(reads)) if a[i] != b[i]]
                    raise AssertionError("reads %s differ from the oracle (DEBUGK=%s)" % (bad[:10], debugk))
    finally:
        monkeypatch.delenv("BWAMEM_HIP_DEBUGK", raising=False)
        lib.destroy_index(h); oracle.destroy_index(ho)


def test_uniform_emu(oracle, workdir, monkeypatch):
    B.build_emu()
    _run(B.product_lib(emu=True), oracle, workdir, "uni_emu", monkeypatch)


@pytest.mark.gpu
def test_uniform_gpu(hip_lib, oracle, workdir, monkeypatch):
    _run(hip_lib, oracle, workdir, "uni_hip", monkeypatch)
