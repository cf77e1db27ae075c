"""Function-level parity of the seeding front end: k_seed.hip and the rank / LF / suffix-array helpers of dev_common.h
(wrapped by tests/gpu_units/units_seed.hip) against the oracle's FM-index, which tests/test_oracle_fmindex.py pins by
brute force.  Every comparison is exact integer equality.  The emulation flavour runs in the CPU suite; the hipcc
flavour is the GPU twin, at larger sizes."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bwalib as B

UNITS = os.path.join(B.ROOT, "tests", "gpu_units")
P = ctypes.c_void_p
I32, I64, U64 = ctypes.c_int, ctypes.c_int64, ctypes.c_uint64
ERR_INTV_CAP = 1
SEED_EL_CAP = 4                      # k_seed.hip: pass-2 candidates a lane remembers in LDS
CODE = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    CODE[_c] = _i
    CODE[_c + 32] = _i


def _u64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint64))


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int32))


def _p(a):
    return a.ctypes.data_as(P)


# ------------------------------------------------------------------------------------------ the two libraries
class Units:
    def __init__(self, flavour):
        subprocess.run(["make", "-s", "-C", UNITS] + (["emu"] if flavour == "emu" else []), check=True)
        self.emu = flavour == "emu"
        self.dll = ctypes.CDLL(os.path.join(UNITS, "_build", "libunits_seed_%s.so" % flavour))
        d = self.dll
        d.useed_index_open.restype = P; d.useed_index_open.argtypes = [ctypes.c_char_p, I32]
        d.useed_index_close.restype = None; d.useed_index_close.argtypes = [P]
        d.useed_index_info.restype = None; d.useed_index_info.argtypes = [P, P]
        d.useed_index_sa_raw.argtypes = [P, P, P]
        d.useed_sa_lookup.argtypes = [P, I64, P, P, P]
        d.useed_lf.argtypes = [P, I64, P, P]
        d.useed_extend.argtypes = [P, I64] + [P] * 6
        d.useed_window.argtypes = [P, U64, U64, U64, P, U64, I64] + [P] * 6 + [I64, P, P]
        d.useed_sa_synth.argtypes = [I64, P, P, I64, P, P, P]
        d.useed_candstack.argtypes = [I32, I32, I32] + [P] * 8
        d.useed_seed.argtypes = [P, P, I32, P, P] + [I32] * 7 + [P] * 6 + [I64] + [P] * 6
        d.useed_scan.argtypes = [P, I32, P]
        d.useed_order.argtypes = [P, I32, P]
        d.useed_nul_offsets.argtypes = [P, I64, I64, I64, P, P]
        d.useed_encode.argtypes = [P, I64]

    def open(self, img, sa_intv=1):
        h = self.dll.useed_index_open(img.encode(), sa_intv)
        assert h, "the wrapper could not put %s on the device" % img
        return h

    def close(self, h):
        self.dll.useed_index_close(h)

    def info(self, h):
        o = np.zeros(12, dtype=np.uint64)
        self.dll.useed_index_info(h, _p(o))
        v = [int(x) for x in o]
        return dict(primary=v[0], L2=v[1:6], seq_len=v[6], n_kept=v[7], sa_intv=v[8], densify_err=int(o[9:10].view(np.int64)[0]), l_pac=v[10], n_seqs=v[11])

    def sa_table(self, h):
        """the kept suffix-array entries, decoded from their two planes as 40-bit two's complement"""
        n = self.info(h)["n_kept"]
        lo, hi = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint8)
        assert self.dll.useed_index_sa_raw(h, _p(lo), _p(hi)) == 0
        v = lo.astype(np.int64) | hi.astype(np.int64) << 32
        return np.where(v >= 1 << 39, v - (1 << 40), v)

    def sa_lookup(self, h, ks):
        ks = _u64(ks); out = np.zeros(len(ks), dtype=np.int64); n_lf = np.zeros(1, dtype=np.uint64)
        assert self.dll.useed_sa_lookup(h, len(ks), _p(ks), _p(out), _p(n_lf)) == 0
        return out, int(n_lf[0])

    def lf(self, h, ks):
        ks = _u64(ks); out = np.zeros(len(ks), dtype=np.uint64)
        assert self.dll.useed_lf(h, len(ks), _p(ks), _p(out)) == 0
        return out

    def extend(self, h, x0, x1, size, c, back):
        x0, x1, size, c, back = _u64(x0), _u64(x1), _u64(size), _i32(c), _i32(back)
        out = np.zeros((len(x0), 3), dtype=np.uint64)
        assert self.dll.useed_extend(h, len(x0), _p(x0), _p(x1), _p(size), _p(c), _p(back), _p(out)) == 0
        return out


class Oracle:
    """an index opened by the oracle, and its FM-index primitives over arrays"""

    def __init__(self, lib, img):
        self.lib, d = lib, lib.dll
        d.oracle_test_extend.restype = None; d.oracle_test_extend.argtypes = [P, ctypes.c_size_t] + [P] * 6
        d.oracle_test_sa.restype = None; d.oracle_test_sa.argtypes = [P, ctypes.c_size_t, P, P]
        d.oracle_test_contigs.argtypes = [P, P, I32]
        d.oracle_test_bwt_info.restype = None; d.oracle_test_bwt_info.argtypes = [P, P]
        d.oracle_collect_intv.argtypes = [P, P, I32, ctypes.c_char_p, P, I32]
        self.h = lib.open_index(img)
        o = np.zeros(9, dtype=np.uint64)
        d.oracle_test_bwt_info(self.h, _p(o))
        v = [int(x) for x in o]
        self.primary, self.L2, self.seq_len, self.sa_intv, self.l_pac = v[0], v[1:6], v[6], v[7], v[8]
        c = np.zeros((4096, 2), dtype=np.int64)
        n = d.oracle_test_contigs(self.h, _p(c), 4096)
        self.ctg_off, self.ctg_len = c[:n, 0].copy(), c[:n, 1].copy()
        self._sa = None

    def close(self):
        self.lib.destroy_index(self.h)

    def sa(self, ks):
        ks = _u64(ks); out = np.zeros(len(ks), dtype=np.int64)
        self.lib.dll.oracle_test_sa(self.h, len(ks), _p(ks), _p(out))
        return out

    def extend(self, x0, x1, size, c, back):
        x0, x1, size, c, back = _u64(x0), _u64(x1), _u64(size), _i32(c), _i32(back)
        out = np.zeros((len(x0), 3), dtype=np.uint64)
        self.lib.dll.oracle_test_extend(self.h, len(x0), _p(x0), _p(x1), _p(size), _p(c), _p(back), _p(out))
        return out

    def full(self):
        """-> (SA of every rank 0..seq_len with SA[0] = -1, rank of every text position 0..seq_len, LF of every rank, the text)"""
        if self._sa is None:
            n = self.seq_len
            sa = self.sa(np.arange(n + 1))
            assert sa[0] == -1 and sa[self.primary] == 0
            pos = sa.copy(); pos[0] = n                                 # rank 0: the empty suffix
            rank_of = np.empty(n + 1, dtype=np.int64); rank_of[pos] = np.arange(n + 1)
            assert (np.sort(pos) == np.arange(n + 1)).all()
            lf = np.where(pos > 0, rank_of[np.maximum(pos - 1, 0)], 0)  # rank of SA[k] - 1; k == primary -> 0
            first = np.searchsorted(np.asarray(self.L2[1:5], dtype=np.int64), np.arange(n + 1), side="left")   # first symbol of the suffix of rank k >= 1
            text = first[rank_of[:n]].astype(np.uint8)
            self._sa = (sa, rank_of, lf, text)
        return self._sa

    def collect(self, opts, codes):
        """mem_collect_intv of one read (codes 0..4) -> list of (x0, size, info), sorted by info"""
        ob = ctypes.create_string_buffer(bytes(opts), 168)
        cap = 4 * len(codes) + 64
        out = np.zeros((cap, 4), dtype=np.uint64)
        n = self.lib.dll.oracle_collect_intv(self.h, ob, len(codes), bytes(codes), _p(out), cap)
        assert n <= cap
        return sorted(((int(a[0]), int(a[2]), int(a[3])) for a in out[:n]), key=lambda t: t[2])


@pytest.fixture(scope="module")
def emu_units():
    return Units("emu")


@pytest.fixture(scope="module")
def hip_units():
    return Units("hip")


# ------------------------------------------------------------------------------------------ 1. the index on the device
def _walks(lf, ks, spacing, primary):
    """LF-walks of sa_lookup from the ranks ks to the next kept rank -> (total steps, ranks whose walk steps from primary to rank 0)"""
    cur = np.asarray(ks, dtype=np.int64).copy()
    total, through = 0, np.zeros(len(cur), dtype=bool)
    while True:
        m = (cur & (spacing - 1)) != 0
        if not m.any():
            return total, through
        total += int(m.sum())
        through |= m & (cur == primary)
        cur[m] = lf[cur[m]]


def _check_index(units, oracle, img, spacings, sample=None):
    O = Oracle(oracle, img)
    sa, rank_of, lf, _ = O.full()
    n, primary = O.seq_len, O.primary
    ranks = np.arange(1, n + 1)
    edge = np.concatenate([rank_of[:70], [primary - 1, primary, primary + 1, 1, 2, n - 1, n], (n // 64) * 64 + np.arange(-2, 3)])
    edge = np.unique(edge[(edge >= 1) & (edge <= n)])
    if sample is not None:
        ranks = np.unique(np.concatenate([ranks[::sample], edge]))
    any_through = False
    for spacing in spacings:
        h = units.open(img, spacing)
        info = units.info(h)
        assert info["densify_err"] == 0 and info["sa_intv"] == spacing and info["n_kept"] == (n >> (spacing.bit_length() - 1)) + 1
        assert (info["primary"], info["L2"], info["seq_len"]) == (primary, O.L2, n)
        tab = units.sa_table(h)
        assert tab[0] == -1
        assert (tab == sa[::spacing]).all(), "densified suffix array differs at spacing %d" % spacing
        got, n_lf = units.sa_lookup(h, ranks)
        assert (got == sa[ranks]).all(), "sa_lookup differs at spacing %d" % spacing
        want_lf, through = _walks(lf, ranks, spacing, primary)
        assert n_lf == want_lf and (n_lf == 0) == (spacing == 1)
        any_through |= bool(through.any())
        if spacing == spacings[0]:
            ks = np.arange(0, n + 1) if sample is None else np.unique(np.concatenate([[0], ranks]))
            assert (units.lf(h, ks).astype(np.int64) == lf[ks]).all(), "lf_step differs"
            assert lf[primary] == 0
        units.close(h)
    if max(spacings) > 1:
        assert any_through, "no sampled rank walks through primary to rank 0"
    O.close()


def test_units_seed_emu_index(emu_units, oracle, rota_img, small_genome):
    _check_index(emu_units, oracle, rota_img, (1, 2, 8, 32))
    _check_index(emu_units, oracle, small_genome[1], (1, 2, 8, 32), sample=41)


@pytest.mark.gpu
def test_units_seed_gpu_index(hip_units, oracle, rota_img, small_genome, medium_genome):
    for img in (rota_img, small_genome[1], medium_genome[1]):
        _check_index(hip_units, oracle, img, (1, 2, 8, 32))


# ------------------------------------------------------------------------------------------ 2. the rank step
def _base_intv(O, c):
    return (O.L2[c] + 1, O.L2[3 - c] + 1, O.L2[c + 1] - O.L2[c])


def _kmer_intervals(O, kmax):
    """every bi-interval of a text k-mer, k <= kmax, reached by extending the one-base intervals in both directions"""
    seen = {_base_intv(O, c) for c in range(4) if O.L2[c + 1] > O.L2[c]}
    level = set(seen)
    for _ in range(kmax - 1):
        iv = np.array(sorted(level), dtype=np.uint64)
        nxt = set()
        for back in (0, 1):
            for c in range(4):
                r = O.extend(iv[:, 0], iv[:, 1], iv[:, 2], np.full(len(iv), c), np.full(len(iv), back))
                nxt |= {tuple(int(v) for v in t) for t in r if t[2] > 0}
        level = nxt - seen
        seen |= nxt
    return sorted(seen)


def _single_rank_pairs(O, ranks):
    """(x, y): the bi-interval (x, y, 1) of a string that occurs once and starts at SA[x], found by extending the first base of
    that suffix forward along the text with the oracle until the interval has size 1"""
    sa, _, _, text = O.full()
    n = O.seq_len
    ranks = np.asarray(ranks, dtype=np.int64)
    pos = sa[ranks].copy()
    c0 = text[pos]
    L2 = np.asarray(O.L2, dtype=np.int64)
    x0, x1, size = L2[c0] + 1, L2[3 - c0] + 1, L2[c0 + 1] - L2[c0]
    depth = np.ones(len(ranks), dtype=np.int64)
    while True:
        act = np.flatnonzero((size > 1) & (pos + depth < n))
        if not len(act):
            break
        r = O.extend(x0[act], x1[act], size[act], 3 - text[pos[act] + depth[act]], np.zeros(len(act))).astype(np.int64)
        x0[act], x1[act], size[act] = r[:, 0], r[:, 1], r[:, 2]
        depth[act] += 1
    ok = size == 1
    assert (x0[ok] == ranks[ok]).all()
    return np.stack([x0[ok], x1[ok]], axis=1)


def _all_extensions(intervals):
    iv = np.asarray(intervals, dtype=np.uint64).reshape(-1, 3)
    x0, x1, sz = (np.repeat(iv[:, j], 8) for j in range(3))
    c = np.tile(np.repeat(np.arange(4), 2), len(iv)); back = np.tile(np.arange(2), 4 * len(iv))
    return x0, x1, sz, c, back


def _classes(O, x0, x1, sz, back):
    """which edges of the rank arithmetic a list of extension cases touches"""
    xa = np.where(back != 0, x0, x1).astype(np.int64)
    k, l = xa - 1, xa - 1 + sz.astype(np.int64)
    kk, ll = k - (k >= O.primary), l - (l >= O.primary)
    last = (O.seq_len - 1) >> 6
    return dict(k_off=set((kk & 63).tolist()), l_off=set((ll & 63).tolist()), xa_minus_primary=set((xa - O.primary)[np.abs(xa - O.primary) <= 1].tolist()),
                contains=int(((xa <= O.primary) & (xa + sz.astype(np.int64) - 1 >= O.primary) & (sz > 1)).sum()),
                last_block=int(((kk >> 6 == last) | (ll >> 6 == last)).sum()), split=int((kk >> 6 != ll >> 6).sum()))


def _compare_extend(units, O, h, cases, what):
    x0, x1, sz, c, back = cases
    want = O.extend(x0, x1, sz, c, back)
    got = units.extend(h, x0, x1, sz, c, back)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), "%s: extend_sm differs from o_bwt_extend in %d of %d cases, first (x0, x1, size, c, is_back) = %s: got %s, want %s" % (
        what, len(bad), len(x0), (int(x0[bad[0]]), int(x1[bad[0]]), int(sz[bad[0]]), int(c[bad[0]]), int(back[bad[0]])), got[bad[0]].tolist(), want[bad[0]].tolist())


MASK16_EDGES = {0, 15, 16, 31, 32, 47, 48, 63}


def _check_extend_exhaustive(units, oracle, img):
    O = Oracle(oracle, img); h = units.open(img)
    kmers = _kmer_intervals(O, 3)
    pairs = _single_rank_pairs(O, np.arange(1, O.seq_len + 1))
    assert len(pairs) > 0.9 * O.seq_len
    singles = [(x, y, 1) for x, y in pairs.tolist()]
    cases = _all_extensions(kmers + singles)
    cl = _classes(O, cases[0], cases[1], cases[2], cases[4])
    assert cl["k_off"] == set(range(64)) and cl["l_off"] == set(range(64)) and cl["xa_minus_primary"] == {-1, 0, 1}
    assert cl["contains"] > 0 and cl["last_block"] > 0 and cl["split"] > 0
    _compare_extend(units, O, h, cases, "exhaustive")
    units.close(h); O.close()


def _harvest(O, reads, rng, per_read=2):
    """real bi-intervals: walk reads with the oracle as bwt_smem1 does, forward from a start until nothing matches, then backward
    from one of the intervals met on the way -> the extension cases asked on the way"""
    q = [CODE[np.frombuffer(r, dtype=np.uint8)] for r in reads if len(r) >= 20]
    q = [np.where(a > 3, rng.integers(0, 4, size=len(a), dtype=np.uint8), a) for a in q] * per_read
    nl = len(q)
    L = np.array([len(a) for a in q]); mat = np.zeros((nl, L.max()), dtype=np.int64)
    for i, a in enumerate(q):
        mat[i, :len(a)] = a
    start = (rng.random(nl) * (L - 10)).astype(np.int64)
    L2 = np.asarray(O.L2, dtype=np.int64)
    c0 = mat[np.arange(nl), start]
    st = np.stack([L2[c0] + 1, L2[3 - c0] + 1, L2[c0 + 1] - L2[c0]], axis=1)
    pos = start + 1
    keep_at = start + 1 + (rng.random(nl) * 25).astype(np.int64)        # the forward depth whose interval the backward walk starts from
    kept = st.copy()
    out = []
    while True:
        act = np.flatnonzero((st[:, 2] > 0) & (pos < L))
        if not len(act):
            break
        c = 3 - mat[act, pos[act]]
        out.append((st[act, 0], st[act, 1], st[act, 2], c, np.zeros(len(act), dtype=np.int64)))
        r = O.extend(st[act, 0], st[act, 1], st[act, 2], c, np.zeros(len(act))).astype(np.int64)
        st[act] = r
        pos[act] += 1
        upd = act[(r[:, 2] > 0) & (pos[act] <= keep_at[act])]
        kept[upd] = st[upd]
    st, pos = kept, start - 1
    while True:
        act = np.flatnonzero((st[:, 2] > 0) & (pos >= 0))
        if not len(act):
            break
        c = mat[act, pos[act]]
        out.append((st[act, 0], st[act, 1], st[act, 2], c, np.ones(len(act), dtype=np.int64)))
        st[act] = O.extend(st[act, 0], st[act, 1], st[act, 2], c, np.ones(len(act))).astype(np.int64)
        pos[act] -= 1
    return tuple(np.concatenate([o[j] for o in out]) for j in range(5))


def _directed_ranks(O, per_class=6):
    """ranks x whose single-rank interval puts k = x - 1 or l = x on each of mask16's boundaries, and the ranks around primary"""
    n, primary = O.seq_len, O.primary
    x = np.arange(1, n + 1)
    k, l = x - 1, x
    kk, ll = k - (k >= primary), l - (l >= primary)
    out = [np.array([primary - 1, primary, primary + 1, 1, n])]
    for off in sorted(MASK16_EDGES):
        for v in (kk, ll):
            hit = x[(v & 63) == off]
            out.append(hit[np.linspace(0, len(hit) - 1, per_class).astype(np.int64)])
    r = np.unique(np.concatenate(out))
    return r[(r >= 1) & (r <= n)]


def _check_extend_genome(units, oracle, img, reads, seed):
    O = Oracle(oracle, img); h = units.open(img)
    rng = np.random.default_rng(seed)
    harvested = _harvest(O, reads, rng)
    assert len(harvested[0]) > 20 * len(reads)
    hc = _classes(O, harvested[0], harvested[1], harvested[2], harvested[4])
    assert hc["split"] > 0 and (harvested[2] > 1000).any() and (harvested[2] == 1).any()
    _compare_extend(units, O, h, harvested, "harvested")
    pairs = _single_rank_pairs(O, _directed_ranks(O))
    both = [(x, y, 1) for x, y in pairs.tolist()] + [(y, x, 1) for x, y in pairs.tolist()]      # the interval of a string and of its reverse complement
    directed = _all_extensions(both + _kmer_intervals(O, 2))
    dc = _classes(O, directed[0], directed[1], directed[2], directed[4])
    for back in (0, 1):                                                     # every directed class, in each direction
        m = directed[4] == back
        d1 = _classes(O, directed[0][m], directed[1][m], directed[2][m], directed[4][m])
        assert MASK16_EDGES <= d1["k_off"] and MASK16_EDGES <= d1["l_off"] and d1["xa_minus_primary"] == {-1, 0, 1}, (back, d1)
    assert dc["contains"] > 0 and dc["last_block"] > 0
    _compare_extend(units, O, h, directed, "directed")
    units.close(h); O.close()


def _repeat_reads(seqs, starts, n, length=120, seed=2):
    rng = np.random.default_rng(seed)
    g = seqs[0][1]
    return [bytes(g[s + o:s + o + length]) for s, o in zip(rng.choice(starts, n).tolist(), rng.integers(-40, 200, n).tolist())]


def test_units_seed_emu_extend(emu_units, oracle, rota_img, small_genome, repeat_genome):
    _check_extend_exhaustive(emu_units, oracle, rota_img)
    seqs, img = small_genome
    _check_extend_genome(emu_units, oracle, img, B.simulate_reads(seqs, 150, length=100, seed=31, sub=0.02, indel=0.002), 1)
    rs, rimg, starts = repeat_genome
    _check_extend_genome(emu_units, oracle, rimg, _repeat_reads(rs, starts, 100), 2)


@pytest.mark.gpu
def test_units_seed_gpu_extend(hip_units, oracle, rota_img, small_genome, medium_genome, repeat_genome):
    _check_extend_exhaustive(hip_units, oracle, rota_img)
    for k, (seqs, img) in enumerate((small_genome, medium_genome)):
        _check_extend_genome(hip_units, oracle, img, B.simulate_reads(seqs, 1500, length=150, seed=31 + k, sub=0.02, indel=0.002), 1 + k)
    rs, rimg, starts = repeat_genome
    _check_extend_genome(hip_units, oracle, rimg, _repeat_reads(rs, starts, 800), 5)


# ------------------------------------------------------------------------------------------ 3. beyond 2^32 on a window
class Window:
    """a Python-integer model of n_blocks occ blocks that stand for blocks B0.. of an index whose counts are beyond 2^32"""

    def __init__(self, rng, n_blocks, primary_at):
        self.nb = n_blocks
        self.sym = rng.integers(0, 4, size=64 * n_blocks, dtype=np.int64)
        self.sym[64 * 7:64 * 9] = 3                                          # runs of one symbol: whole words and blocks of it
        self.sym[64 * 11:64 * 12] = 0
        # counts before the window: T crosses 2^39 inside it (all eight high bits), G crosses 2^33 (its low word wraps), C is just beyond 2^32
        C, G, T = (1 << 32) + 12345, (1 << 33) - 1500, (1 << 39) - 2000
        A = (1 << 36) + 77
        A += -(A + C + G + T) % 64
        self.base = [A, C, G, T]
        assert min(C, G, T) >= 1 << 32 and T >= (1 << 39) - (1 << 20)
        self.B0 = (A + C + G + T) // 64
        self.lo, self.hi = 64 * self.B0, 64 * (self.B0 + n_blocks)           # stored positions of the window
        self.primary = {"inside": self.lo + 64 * (n_blocks // 2) + 17, "below": 1000, "above": self.hi + 5000}[primary_at]
        self.seq_len = self.hi + 100000
        self.L2 = [0, (1 << 38) + 5, (1 << 38) + (1 << 37) + 11, (1 << 39) + 3, self.seq_len]
        onehot = self.sym[:, None] == np.arange(4)[None, :]
        self.cum = np.cumsum(onehot, axis=0)                                 # cum[j][c] = # of c among stored symbols lo .. lo + j
        assert self.base[3] + int(self.cum[-1, 3]) > 1 << 39 and self.base[2] + int(self.cum[-1, 2]) > 1 << 33

    def table(self):
        t = np.zeros((self.nb, 8), dtype=np.uint32)
        for b in range(self.nb):
            cnt = [self.base[c] + (int(self.cum[64 * b - 1, c]) if b else 0) for c in range(4)]
            assert sum(cnt) == 64 * (self.B0 + b)
            t[b, 0:3] = [cnt[1] & 0xffffffff, cnt[2] & 0xffffffff, cnt[3] & 0xffffffff]
            t[b, 3] = (cnt[1] >> 32 & 0xff) | (cnt[2] >> 32 & 0xff) << 8 | (cnt[3] >> 32 & 0xff) << 16
            for w in range(4):
                s = self.sym[64 * b + 16 * w:64 * b + 16 * w + 16]
                t[b, 4 + w] = sum(int(v) << (2 * (15 - i)) for i, v in enumerate(s))
        return t

    def occ(self, k):
        """# of each symbol in BWT$[0..k], k in sentinel-inclusive coordinates"""
        kk = k - (k >= self.primary)
        assert self.lo <= kk < self.hi
        return [self.base[c] + int(self.cum[kk - self.lo, c]) for c in range(4)]

    def extend(self, x0, x1, size, c, back):
        xa, xb = (x0, x1) if back else (x1, x0)
        tk, tl = self.occ(xa - 1), self.occ(xa - 1 + size)
        s = [tl[i] - tk[i] for i in range(4)]
        other = xb + (1 if xa <= self.primary <= xa + size - 1 else 0) + sum(s[c + 1:])
        na = self.L2[c] + 1 + tk[c]
        return (na, other, s[c]) if back else (other, na, s[c])

    def lf(self, k):
        if k == self.primary:
            return 0
        x = k - (k > self.primary)
        c = int(self.sym[x - self.lo])
        return self.L2[c] + self.base[c] + int(self.cum[x - self.lo, c])


def _check_window(units, n_blocks, n_cases):
    rng = np.random.default_rng(17)
    for at in ("inside", "below", "above"):
        W = Window(rng, n_blocks, at)
        lo, hi = W.lo + 2, W.hi - 2                                           # ranks whose stored positions the model keeps inside the window
        k = rng.integers(lo, hi, size=n_cases)
        size = np.minimum(rng.choice([1, 2, 5, 63, 64, 65, 700, 64 * n_blocks], size=n_cases) * rng.random(n_cases) + 1, hi - k).astype(np.int64)
        xa = k + 1
        edge = [W.lo + 64 * 7 + o for o in (0, 15, 16, 31, 32, 47, 48, 63, 64)]
        if at == "inside":
            p = W.primary
            xa = np.concatenate([xa, [p - 1, p, p + 1, p - 5, p - 70, p, p - 1, lo + 1]])
            size = np.concatenate([size, [1, 1, 1, 10, 141, 200, 2, hi - lo - 2]])
            assert ((xa <= p) & (xa + size - 1 >= p) & (size > 1)).sum() >= 4     # intervals that contain primary
        xa = np.concatenate([xa, np.array(edge) + 1, np.array(edge) - 20]); size = np.concatenate([size, [1] * len(edge), [21] * len(edge)])
        n = len(xa)
        xb = rng.integers(1, 1 << 39, size=n)
        c, back = rng.integers(0, 4, size=n), rng.integers(0, 2, size=n)
        x0, x1 = np.where(back == 1, xa, xb), np.where(back == 1, xb, xa)
        want = np.array([W.extend(int(x0[i]), int(x1[i]), int(size[i]), int(c[i]), int(back[i])) for i in range(n)], dtype=np.uint64)
        ks = np.concatenate([rng.integers(lo, hi, size=n_cases), np.array(edge), [W.primary] if at == "inside" else [], [W.primary - 1, W.primary + 1] if at == "inside" else []]).astype(np.int64)
        want_lf = np.array([W.lf(int(v)) for v in ks], dtype=np.uint64)
        assert want.max() >= 1 << 39 and want_lf.max() >= 1 << 39
        x0, x1, sz, c32, b32, ksu = _u64(x0), _u64(x1), _u64(size), _i32(c), _i32(back), _u64(ks)
        got, got_lf = np.zeros((n, 3), dtype=np.uint64), np.zeros(len(ks), dtype=np.uint64)
        tab, L2 = W.table(), _u64(W.L2)
        rc = units.dll.useed_window(_p(tab), W.nb, W.B0, W.primary, _p(L2), W.seq_len, n, _p(x0), _p(x1), _p(sz), _p(c32), _p(b32), _p(got), len(ks), _p(ksu), _p(got_lf))
        assert rc != -2, "the wrapper refused a case: a rank outside the window"
        assert rc == 0
        bad = np.flatnonzero((got != want).any(axis=1))
        assert not len(bad), (at, len(bad), [int(v) for v in (x0[bad[0]], x1[bad[0]], sz[bad[0]], c[bad[0]], back[bad[0]])], got[bad[0]].tolist(), want[bad[0]].tolist())
        assert (got_lf == want_lf).all(), (at, "lf_step")
    # the refusal itself: a rank one block beyond the window launches nothing
    far = _u64([W.hi + 64])
    assert units.dll.useed_window(_p(tab), W.nb, W.B0, W.primary, _p(L2), W.seq_len, 0, None, None, None, None, None, None, 1, _p(far), _p(got_lf)) == -2


def _check_sa_synth(units):
    rng = np.random.default_rng(4)
    ent = np.concatenate([[-1, 0, (1 << 32) - 1, 1 << 32, (1 << 39) - 1, 1, (1 << 32) + 1, (1 << 39) - 2, 255 << 31], rng.integers(0, 1 << 39, size=300)]).astype(np.int64)
    lo, hi = (ent & 0xffffffff).astype(np.uint32), (ent >> 32 & 0xff).astype(np.uint8)
    assert lo[0] == 0xffffffff and hi[0] == 0xff
    ks = _u64(np.arange(len(ent))); out = np.zeros(len(ent), dtype=np.int64); n_lf = np.ones(1, dtype=np.uint64)
    assert units.dll.useed_sa_synth(len(ent), _p(lo), _p(hi), len(ks), _p(ks), _p(out), _p(n_lf)) == 0
    assert (out == ent).all() and n_lf[0] == 0


def _check_candstack(units):
    rng = np.random.default_rng(6)
    for K in (2, 4, 16):
        for narrow in (0, 1):
            n = K + 9
            vmax, emax = ((1 << 35) - 1, 1022) if narrow else ((1 << 37) - 1, (1 << 17) - 1)

            def vals():
                x, s = rng.integers(0, vmax + 1, size=(n, 64)), rng.integers(0, vmax + 1, size=(n, 64))
                e = rng.integers(0, emax + 1, size=(n, 64))
                x[0, :8], s[0, 8:16], e[0, 16:24] = vmax, vmax, emax          # the largest value of each field, alone and together
                x[n - 1, :8], s[n - 1, :8], e[n - 1, :8] = vmax, vmax, emax
                x[1, :4], s[1, 4:8], e[1, 8:12] = 0, 0, 0
                x[2], s[2], e[2] = np.arange(64) << 29, np.arange(64) << 28, np.arange(64) * (emax // 64)
                return _u64(x), _u64(s), _i32(e)
            a, b = vals(), vals()
            assert len({tuple(v) for v in np.stack([a[0], a[1], a[2].astype(np.uint64)], axis=2).reshape(n, 64, 3)[3].tolist()}) == 64   # the lanes differ
            out = np.zeros((2, n, 64, 3), dtype=np.uint64); ok = np.zeros((n + 2, 64), dtype=np.int32)
            assert units.dll.useed_candstack(K, narrow, n, _p(a[0]), _p(a[1]), _p(a[2]), _p(b[0]), _p(b[1]), _p(b[2]), _p(out), _p(ok)) == 0
            assert (ok[:n] == 1).all() and (ok[n:] == 0).all(), (K, narrow, "push beyond spill_cap must fail, and only that")
            for ph, v in enumerate((a, b)):
                for j in range(3):
                    assert (out[ph, :, :, j] == v[j].astype(np.uint64)).all(), (K, narrow, ph, "x0 size end".split()[j])


def test_units_seed_emu_window(emu_units):
    _check_window(emu_units, 200, 600)
    _check_sa_synth(emu_units)
    _check_candstack(emu_units)


@pytest.mark.gpu
def test_units_seed_gpu_window(hip_units):
    _check_window(hip_units, 400, 4000)
    _check_sa_synth(hip_units)
    _check_candstack(hip_units)


# ------------------------------------------------------------------------------------------ 4. k_seed + k_seed_fin + k_sa
def _intv2rid(O, rb, re):
    """bns_intv2rid restated: the contig of [rb, re) in the doubled coordinate system; -2 across the strand boundary, -1 across contigs"""
    rb, re = np.asarray(rb, dtype=np.int64), np.asarray(re, dtype=np.int64)
    l_pac = O.l_pac

    def rid(p):
        p = np.where(p >= l_pac, 2 * l_pac - 1 - p, p)
        return np.searchsorted(O.ctg_off, p, side="right") - 1
    a, b = rid(rb), rid(np.where(rb < re, re - 1, rb))
    return np.where((rb < l_pac) & (re > l_pac), -2, np.where(a == b, a, -1))


def _seed_reference(O, opts, reads):
    """what k_seed + k_seed_fin + the scan + k_sa must produce, from the oracle's interval lists and mem_chain's occurrence rule"""
    max_occ, min_len, split_len = B.get_opt(opts, "max_occ"), B.get_opt(opts, "min_seed_len"), int(B.get_opt(opts, "min_seed_len") * B.get_opt(opts, "split_factor") + .499)
    ref = dict(intv=[], iso=[], n_seeds=[], l_rep=[], ranks=[], qbeg=[], slen=[])
    for rd in reads:
        codes = CODE[np.frombuffer(rd, dtype=np.uint8)]
        iv = O.collect(opts, codes) if len(codes) else []
        iso, n_seeds, l_rep, b, e = [], 0, 0, 0, 0
        for x0, size, info in iv:
            sb, se = info >> 32, info & 0xffffffff
            assert se - sb >= min_len
            step = size // max_occ if size > max_occ else 1
            count = min(-(-size // step), max_occ)
            iso.append(n_seeds); n_seeds += count
            ref["ranks"] += [x0 + k * step for k in range(count)]; ref["qbeg"] += [sb] * count; ref["slen"] += [se - sb] * count
            if size > max_occ:                                         # the union length of the repetitive spans
                if sb > e:
                    l_rep += e - b; b, e = sb, se
                else:
                    e = max(e, se)
        l_rep += e - b
        ref["intv"].append(iv); ref["iso"].append(iso); ref["n_seeds"].append(n_seeds); ref["l_rep"].append(l_rep)
    ref["rbeg"] = O.sa(ref["ranks"]) if ref["ranks"] else np.zeros(0, dtype=np.int64)
    ref["rid"] = _intv2rid(O, ref["rbeg"], ref["rbeg"] + np.asarray(ref["slen"], dtype=np.int64))
    ref["split_len"] = split_len
    return ref


def _pass2_candidates(O, opts, read):
    """matches of pass 1 that pass 2 re-seeds: counted on pass 1 alone (the list of split_width 0 without pass 3)"""
    p1 = O.collect(B.set_opt(bytearray(opts), split_width=0, max_mem_intv=0), CODE[np.frombuffer(read, dtype=np.uint8)])
    split_len = int(B.get_opt(opts, "min_seed_len") * B.get_opt(opts, "split_factor") + .499)
    return sum(1 for x0, size, info in p1 if (info & 0xffffffff) - (info >> 32) >= split_len and size <= B.get_opt(opts, "split_width"))


def _run_seed(units, h, opts, reads, mode=0, K=16, refill_min=4, narrow=1, grid=None, intv_cap=None, smem_cap=None, seeds_cap=1 << 21):
    n = len(reads)
    off = np.zeros(n + 1, dtype=np.int64); off[1:] = np.cumsum([len(r) + 1 for r in reads])
    req = b"".join(r + b"\0" for r in reads)
    max_len = max(len(r) for r in reads)
    intv_cap = intv_cap or max(64, max_len + 8); smem_cap = smem_cap or max_len + 2; grid = grid or (n + 63) // 64
    ob = ctypes.create_string_buffer(bytes(opts), 168)
    n_intv, n_seeds, l_rep = (np.zeros(n, dtype=np.int32) for _ in range(3))
    intv = np.zeros((n, intv_cap, 3), dtype=np.uint64); iso = np.zeros((n, intv_cap), dtype=np.int32)
    seed_off = np.zeros(n + 1, dtype=np.int64)
    rbeg = np.zeros(seeds_cap, dtype=np.int64); qbeg, slen, rid = (np.zeros(seeds_cap, dtype=np.int32) for _ in range(3))
    err = np.zeros(1, dtype=np.int32); cnt = np.zeros(3, dtype=np.uint64)
    rc = units.dll.useed_seed(h, ob, n, req, _p(off), mode, K, refill_min, narrow, grid, intv_cap, smem_cap, _p(n_intv), _p(intv), _p(iso), _p(n_seeds), _p(l_rep), _p(seed_off),
                              seeds_cap, _p(rbeg), _p(qbeg), _p(slen), _p(rid), _p(err), _p(cnt))
    assert rc == 0, "useed_seed returned %d" % rc
    n_occ = int(seed_off[n])
    return dict(n_intv=n_intv, intv=intv, iso=iso, n_seeds=n_seeds, l_rep=l_rep, seed_off=seed_off, rbeg=rbeg[:n_occ], qbeg=qbeg[:n_occ], slen=slen[:n_occ], rid=rid[:n_occ],
                err=int(err[0]), n_lf=int(cnt[1]), n_sa=int(cnt[2]))


def _compare_seed(got, ref, what, overflowed=()):
    """every array of a k_seed run against the reference; reads in `overflowed` must come back empty with ERR_INTV_CAP set"""
    n = len(ref["intv"])
    assert got["err"] == (ERR_INTV_CAP if overflowed else 0), (what, got["err"])
    want_off, ranks_at = [0], [0]
    sel = []
    for r in range(n):
        iv = [] if r in overflowed else ref["intv"][r]
        assert got["n_intv"][r] == len(iv), (what, r, int(got["n_intv"][r]), len(iv))
        assert [tuple(int(v) for v in t) for t in got["intv"][r, :len(iv)]] == iv, (what, "interval list of read %d" % r)
        if r in overflowed:
            assert got["n_seeds"][r] == 0 and got["l_rep"][r] == 0
        else:
            assert got["iso"][r, :len(iv)].tolist() == ref["iso"][r], (what, "intv_seed_off of read %d" % r)
            assert (got["n_seeds"][r], got["l_rep"][r]) == (ref["n_seeds"][r], ref["l_rep"][r]), (what, r)
            sel += range(ranks_at[-1], ranks_at[-1] + ref["n_seeds"][r])
        ranks_at.append(ranks_at[-1] + ref["n_seeds"][r])
        want_off.append(want_off[-1] + int(got["n_seeds"][r]))
    assert got["seed_off"].tolist() == want_off, (what, "seed_off")
    sel = np.asarray(sel, dtype=np.int64)
    for key in ("rbeg", "qbeg", "slen", "rid"):
        assert (got[key] == np.asarray(ref[key])[sel]).all(), (what, key)
    assert got["n_sa"] == len(sel)


def _chimera(g, k, pieces=8, piece=40):
    return b"".join(bytes(g[1000 * (4 * j + k + 1):1000 * (4 * j + k + 1) + piece]) for j in range(pieces))


def _small_reads(seqs, n_sim, length):
    g = seqs[0][1]
    reads = B.simulate_reads(seqs, n_sim, length=length, seed=77, sub=0.03, indel=0.004, n_rate=0.01, random_frac=0.1)
    reads += [b"N" * 30, b"", b"ACGTACGTACGTACGTAC", b"ACGTN" * 12, b"acgtacgtacgtNNacgtacgtgggttcatgca"]
    reads += [_chimera(g, 0), _chimera(g, 2, pieces=6)]
    last = seqs[-1][1]
    reads.append(last[-35:] + B.revcomp(last[-35:]))                       # matches across the end of the forward strand
    reads.append(seqs[0][1][-40:] + seqs[1][1][:40])                         # matches across two contigs
    return reads


def _check_seed_small(units, oracle, small_genome, n_sim, length, n_queue):
    seqs, img = small_genome
    O = Oracle(oracle, img)
    reads = _small_reads(seqs, n_sim, length)
    base = oracle.default_options()
    h1, h32 = units.open(img, 1), units.open(img, 32)
    ref0 = _seed_reference(O, base, reads)
    # the cases hold what they are here for
    assert any(_pass2_candidates(O, base, r) > SEED_EL_CAP for r in reads if r), "no read with more pass-2 candidates than the LDS list holds"
    assert (ref0["rid"] == -1).any() and (ref0["rid"] == -2).any() and (ref0["rid"] >= 0).any()
    assert ref0["intv"][n_sim] == [] and ref0["intv"][n_sim + 1] == [] and ref0["intv"][n_sim + 2] == []
    # geometry: ring sizes, both stack layouts, refill thresholds, one workgroup for the whole tile, more workgroups than reads
    for K in (2, 4, 16):
        for narrow in (0, 1):
            _compare_seed(_run_seed(units, h1, base, reads, K=K, narrow=narrow, refill_min=1 if K == 4 else 64 if K == 2 else 4, grid=1 if K != 16 else 5), ref0, ("K", K, narrow))
    got = _run_seed(units, h32, base, reads, K=16, narrow=1, grid=64)        # many workgroups, sampled SA
    _compare_seed(got, ref0, "spacing 32")
    assert got["n_lf"] > 0
    _compare_seed(_run_seed(units, h1, base, reads, mode=1), ref0, "launch_seed")
    # one workgroup pulling several hundred short reads from the queue
    queue = B.simulate_reads(seqs, n_queue, length=36, seed=5, sub=0.02, n_rate=0.01) + [b"", b"N" * 40]
    _compare_seed(_run_seed(units, h1, base, queue, K=4, narrow=1, refill_min=1, grid=1), _seed_reference(O, base, queue), "queue")
    # options
    for kw in (dict(min_seed_len=12), dict(min_seed_len=30), dict(split_width=0), dict(max_mem_intv=0), dict(max_mem_intv=5), dict(max_occ=3), dict(split_factor=1.0)):
        opts = B.set_opt(oracle.default_options(), **kw)
        ref = _seed_reference(O, opts, reads)
        _compare_seed(_run_seed(units, h1, opts, reads, K=4, narrow=1, grid=2), ref, kw)
    # overflow of the interval list: the read with the most intervals alone
    counts = sorted(len(iv) for iv in ref0["intv"])
    assert counts[-1] > counts[-2]
    heavy = [r for r in range(len(reads)) if len(ref0["intv"][r]) == counts[-1]]
    _compare_seed(_run_seed(units, h1, base, reads, K=16, narrow=1, grid=2, intv_cap=counts[-2]), ref0, "intv_cap", overflowed=set(heavy))
    units.close(h1); units.close(h32); O.close()


def _forward_pushes(O, codes):
    """candidates the forward phase of bwt_smem1 stacks up from position 0 (restated with the oracle's extension)"""
    ik, n = _base_intv(O, int(codes[0])), 0
    for i in range(1, len(codes)):
        if codes[i] > 3:
            break
        ok = tuple(int(v) for v in O.extend([ik[0]], [ik[1]], [ik[2]], [3 - int(codes[i])], [0])[0])
        if ok[2] != ik[2]:
            n += 1
            if ok[2] < 1:
                return n
        ik = ok
    return n + 1


def _forward_sizes(O, codes, x):
    """interval size of codes[x .. i] for every i > x the forward walk reaches (what bwt_seed_strategy1 looks at)"""
    ik, out = _base_intv(O, int(codes[x])), {}
    for i in range(x + 1, len(codes)):
        if codes[i] > 3 or ik[2] == 0:
            break
        ik = tuple(int(v) for v in O.extend([ik[0]], [ik[1]], [ik[2]], [3 - int(codes[i])], [0])[0])
        out[i] = ik[2]
    return out


def _check_seed_repeats(units, oracle, repeat_genome, n_reads):
    """a young repeat family: interval sizes beyond max_occ (occurrences sampled with step > 1, l_rep > 0), deep candidate stacks"""
    seqs, img, starts = repeat_genome
    O = Oracle(oracle, img); h = units.open(img, 1)
    base = oracle.default_options()
    reads = _repeat_reads(seqs, starts, n_reads, length=110, seed=9)
    g = seqs[0][1]
    for st in starts[:3]:                                                   # a substitution every 24 bases: matches short enough to be shared by most copies
        rd = bytearray(g[st + 20:st + 130])
        for p in range(12, len(rd), 24):
            rd[p] = ord("ACGT"[("ACGT".index(chr(rd[p])) + 1) % 4])
        reads.append(bytes(rd))
    ref = _seed_reference(O, base, reads)
    # (600 copies at 2 % divergence share no 19-mer more than about 400 times: the default max_occ of 500 is out of this fixture's
    # reach, so the sampling rule and l_rep are exercised with max_occ 3 and 50 below)
    assert any(size > 100 for iv in ref["intv"] for _, size, _ in iv)
    _compare_seed(_run_seed(units, h, base, reads, K=4, narrow=1, grid=1, refill_min=1), ref, "repeats, spill")
    _compare_seed(_run_seed(units, h, base, reads, K=16, narrow=0, grid=2), ref, "repeats, wide")
    o1 = B.set_opt(oracle.default_options(), max_occ=3)
    r1 = _seed_reference(O, o1, reads)
    assert any(size > 6 for iv in r1["intv"] for _, size, _ in iv)
    _compare_seed(_run_seed(units, h, o1, reads, K=16, narrow=1, grid=2), r1, "repeats, max_occ 3")
    o2 = B.set_opt(oracle.default_options(), max_occ=50)
    r2 = _seed_reference(O, o2, reads)
    assert any(size >= 100 for iv in r2["intv"] for _, size, _ in iv) and max(r2["l_rep"]) > 0        # step >= 2
    _compare_seed(_run_seed(units, h, o2, reads, K=16, narrow=1, grid=2), r2, "repeats, max_occ 50")
    # directed case "pass3_size_equals_max_mem_intv": the greedy seed of pass 3 stops at the first size BELOW max_mem_intv; here the first
    # size it may stop at (min_seed_len bases after the start) equals max_mem_intv, so it has to go on
    codes0 = CODE[np.frombuffer(reads[0], dtype=np.uint8)]
    sizes = _forward_sizes(O, codes0, 0)
    at = B.get_opt(base, "min_seed_len")
    assert sizes[at] > 1 and any(v < sizes[at] for i, v in sizes.items() if i > at)
    o4 = B.set_opt(oracle.default_options(), max_mem_intv=sizes[at])
    r4 = _seed_reference(O, o4, reads)
    assert not any(info == at + 1 and size == sizes[at] for _, size, info in r4["intv"][0])      # (start 0, end at + 1) is not a seed
    _compare_seed(_run_seed(units, h, o4, reads, K=16, narrow=1, grid=2), r4, "pass3_size_equals_max_mem_intv")
    # overflow of the candidate stack: short reads cannot stack more candidates than they have bases; the family read does
    o3 = B.set_opt(oracle.default_options(), min_seed_len=12)
    short = [r[:18] for r in reads[:6]] + [reads[0]]
    K, smem_cap = 4, 16
    assert _forward_pushes(O, CODE[np.frombuffer(reads[0], dtype=np.uint8)]) > K + smem_cap
    r3 = _seed_reference(O, o3, short)
    assert len(r3["intv"][-1]) > 0 and sum(len(iv) for iv in r3["intv"][:-1]) > 0
    _compare_seed(_run_seed(units, h, o3, short, K=K, narrow=1, grid=1, smem_cap=smem_cap), r3, "smem_cap", overflowed={len(short) - 1})
    units.close(h); O.close()


def _check_seed_long(units, oracle, small_genome, n_each):
    """reads beyond 768 bases walk their bases in global memory (LDSQ == false); from 1023 bases on the stack is wide"""
    seqs, img = small_genome
    O = Oracle(oracle, img); h = units.open(img, 1)
    base = oracle.default_options()
    for length, narrow in ((800, 1), (1100, 0)):
        reads = B.simulate_reads(seqs, n_each, length=length, seed=length, sub=0.04, indel=0.01, n_rate=0.002) + [b"ACGT" * 5]
        ref = _seed_reference(O, base, reads)
        _compare_seed(_run_seed(units, h, base, reads, K=4, narrow=narrow, grid=1, intv_cap=length), ref, ("long", length))
        _compare_seed(_run_seed(units, h, base, reads, mode=1, intv_cap=length), ref, ("long, launch_seed", length))
    units.close(h); O.close()


def _check_seed_split_width(units, oracle, hip_lib, workdir):
    """split_width 40000: pass-1 matches with 32768 occurrences or more do not fit the 15-bit size of the LDS candidate word and
    must take the fall-back walk of pass 2.  No fixture has such a match, so one is built: a 40 kbp contig of one base."""
    import conftest
    rng = np.random.default_rng(99)
    seqs = [("r%d" % i, B.BASES[rng.integers(0, 4, size=30000, dtype=np.uint8)].tobytes()) for i in range(2)]
    lowc = bytearray(b"A" * 40000)
    for p in rng.integers(100, 39900, size=12).tolist():                       # a few interruptions, so that reads have several long matches
        lowc[p] = ord("G")
    seqs.insert(1, ("lowc", bytes(lowc)))
    _, img = conftest._build_genome(hip_lib, workdir, "glowc", 0, seqs=seqs)
    O = Oracle(oracle, img); h = units.open(img, 1)
    opts = B.set_opt(oracle.default_options(), split_width=40000)
    reads = [bytes(lowc[s:s + 80]) for s in (5000, 12001, 30000)] + [seqs[0][1][100:170] + bytes(lowc[700:760]), seqs[2][1][500:600]]
    ref = _seed_reference(O, opts, reads)
    big = [(size, (info & 0xffffffff) - (info >> 32)) for iv in ref["intv"] for _, size, info in iv if size >= 32768]
    assert any(ln >= ref["split_len"] for _, ln in big), "no match of 28 bases or more with 32768 occurrences or more"
    _compare_seed(_run_seed(units, h, opts, reads, K=4, narrow=1, grid=1), ref, "split_width 40000")
    _compare_seed(_run_seed(units, h, opts, reads, mode=1), ref, "split_width 40000, launch_seed")
    units.close(h); O.close()


def test_units_seed_emu_kernel(emu_units, oracle, small_genome):
    _check_seed_small(emu_units, oracle, small_genome, 20, 70, 200)


def test_units_seed_emu_kernel_repeats_long(emu_units, oracle, hip_lib, workdir, small_genome, repeat_genome):
    _check_seed_repeats(emu_units, oracle, repeat_genome, 10)
    _check_seed_long(emu_units, oracle, small_genome, 1)
    _check_seed_split_width(emu_units, oracle, hip_lib, workdir)


@pytest.mark.gpu
def test_units_seed_gpu_kernel(hip_units, oracle, hip_lib, workdir, small_genome, repeat_genome):
    _check_seed_small(hip_units, oracle, small_genome, 400, 150, 600)
    _check_seed_repeats(hip_units, oracle, repeat_genome, 150)
    _check_seed_long(hip_units, oracle, small_genome, 12)
    _check_seed_split_width(hip_units, oracle, hip_lib, workdir)


# ------------------------------------------------------------------------------------------ 5. the small kernels
def check_scan_forms(scan, monkeypatch):
    """launch_scan: the one-workgroup form, the two-launch form whose blocks add up the block sums before them, and the three-launch
    form with a one-wave scan of the sums must all be numpy's exclusive cumsum.  scan(x) -> out[n + 1]"""
    rng = np.random.default_rng(5)
    for single_max, fused_max, sizes in (("8192", "2048", (0, 1, 63, 4097)), ("1", "2048", (1, 4095, 4096, 3 * 4096 + 17)), ("1", "1", (4097, 70 * 4096 + 5))):
        monkeypatch.setenv("BWAMEM_HIP_SCAN_SINGLE_MAX", single_max)
        monkeypatch.setenv("BWAMEM_HIP_SCAN_FUSED_MAX", fused_max)
        for n in sizes:
            x = rng.integers(0, 1 << 20, size=max(n, 1), dtype=np.int32)[:n]
            x[: n // 2] = rng.integers(0, 2 ** 31 - 1, size=n // 2, dtype=np.int32)       # totals beyond 32 bits
            out = scan(x)
            want = np.concatenate([[0], np.cumsum(x.astype(np.int64))])
            assert (out == want).all(), (single_max, fused_max, n)


def unit_scan(units):
    def scan(x):
        x = _i32(x); out = np.full(len(x) + 1, -1, dtype=np.int64)
        assert units.dll.useed_scan(_p(x), len(x), _p(out)) == 0
        return out
    return scan


def _check_order(units):
    rng = np.random.default_rng(12)
    for n in (0, 1, 255, 256, 257, 100000):
        ns = rng.choice([0, 0, 1, 1, 2, 3, 7, 8, 500, 1 << 20, 1 << 30, (1 << 30) - 1], size=n).astype(np.int32)
        ns[n // 3:n // 2] = rng.integers(0, (1 << 30) + 1, size=n // 2 - n // 3)
        order = np.full(n, -1, dtype=np.int32)
        assert units.dll.useed_order(_p(_i32(ns)), n, _p(order)) == 0
        assert (np.sort(order) == np.arange(n)).all(), (n, "not a permutation")
        v = ns[order].astype(np.int64)
        bins = np.where(v <= 0, 31, 31 - np.floor(np.log2(np.maximum(v, 1))).astype(np.int64))   # order_bin: __clz of a positive 32-bit int
        assert (np.diff(bins) >= 0).all(), (n, "bins not in order")


def _check_nul(units):
    rng = np.random.default_rng(13)
    bufs = []
    for n in (1, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 8191, 8192, 8193, 3 * 4096 + 16, 50001):
        a = rng.integers(1, 256, size=n, dtype=np.uint8)
        bufs.append(a.copy())                                               # no NUL at all
        b = a.copy(); b[rng.integers(0, n, size=max(1, n // 9))] = 0; b[0] = 0; b[-1] = 0
        if n > 40:
            b[20:24] = 0; b[14:18] = 0; b[n - 3:] = 0                       # adjacent NULs, across a 16-byte boundary, at the end
        bufs.append(b)
        bufs.append(np.zeros(n, dtype=np.uint8))
    for b in bufs:
        want = np.flatnonzero(b == 0) + 1
        for cut in (None, len(want) // 2) if len(want) > 1 else (None,):
            nmax = len(want) + 3 if cut is None else cut
            off = np.zeros(len(want) + 8, dtype=np.int64); found = np.full(1, -7, dtype=np.int64)
            assert units.dll.useed_nul_offsets(_p(b), len(b), nmax, len(off), _p(off), _p(found)) == 0
            assert found[0] == len(want), (len(b), cut)
            k = min(nmax, len(want))
            assert off[0] == 0 and (off[1:k + 1] == want[:k]).all(), (len(b), cut)
            assert (off[k + 1:] == -1).all(), (len(b), cut, "written past n_reads_max or past the NULs found")


def _check_encode(units):
    table = np.full(256, 4, dtype=np.uint8)                                  # nst_nt4_table
    for i, ch in enumerate("ACGT"):
        table[ord(ch)] = table[ord(ch.lower())] = i
    table[0:4] = [0, 1, 2, 3]
    for n in (256, 255, 257, 1000003, 8192 * 256 + 77):
        a = np.resize(np.arange(256, dtype=np.uint8), n).copy()
        np.random.default_rng(n).shuffle(a[256:])
        want = table[a]
        assert units.dll.useed_encode(_p(a), n) == 0
        assert (a == want).all(), n


def test_units_seed_emu_small_kernels(emu_units):
    """(launch_scan on the emulation: tests/test_emu_parity.py::test_emu_scan_forms, through the same helper)"""
    _check_order(emu_units)
    _check_nul(emu_units)
    _check_encode(emu_units)


@pytest.mark.gpu
def test_units_seed_gpu_small_kernels(hip_units, monkeypatch):
    check_scan_forms(unit_scan(hip_units), monkeypatch)
    _check_order(hip_units)
    _check_nul(hip_units)
    _check_encode(hip_units)
