"""The seeding grid's LDS reserve changes only how many k_seed workgroups share a CU with the tiles' kernels, never a byte of
the response: small tiles, small seeding chunks and four tile streams, so that tiles really run beside seeding chunks, under
every plan -- no reserve, the default, one workgroup's worth, a reserve that leaves one seeding workgroup per CU, and
BWAMEM_HIP_SEED_WPC=1."""
import pytest

import bwalib as B

pytestmark = pytest.mark.gpu

BESIDE = {"BWAMEM_HIP_TILE": "97", "BWAMEM_HIP_SEED_CHUNK": "500", "BWAMEM_HIP_STREAMS": "4"}
SETTINGS = [("no reserve", {"BWAMEM_HIP_SEED_RESERVE": "0"}),
            ("default", {}),
            ("one workgroup's worth", {"BWAMEM_HIP_SEED_RESERVE": "16640"}),        # eight workgroups of 150-base reads per CU
            ("one workgroup per CU", {"BWAMEM_HIP_SEED_RESERVE": "1000000"}),      # cut to what one workgroup leaves
            ("wpc 1", {"BWAMEM_HIP_SEED_WPC": "1"})]


def _oracle_bytes(hip_lib, oracle, img, reads, flag=0):
    ho = oracle.open_index(img)
    try:
        return oracle.align_raw(ho, B.set_opt(hip_lib.default_options(), flag=flag), B.pack_request(reads))
    finally:
        oracle.destroy_index(ho)


@pytest.fixture(scope="module")
def cases(hip_lib, oracle, small_genome):
    """name -> (reads, option flag, the oracle's response): computed once, shared by every setting"""
    seqs, img = small_genome
    se = B.simulate_reads(seqs, 3000, length=150, seed=1, sub=0.02, indel=0.003, n_rate=0.002, random_frac=0.02)
    pe = B.simulate_pairs(seqs, 150, length=150, seed=31, ins_mean=350, ins_sd=30, sub=0.01)
    long251 = B.simulate_reads(seqs, 300, length=251, seed=3, sub=0.05, indel=0.01)
    return {"se150": (se, 0, _oracle_bytes(hip_lib, oracle, img, se)),
            "pe150": (pe, B.MEM_F_PE, _oracle_bytes(hip_lib, oracle, img, pe, B.MEM_F_PE)),
            "se251": (long251, 0, _oracle_bytes(hip_lib, oracle, img, long251))}


@pytest.mark.parametrize("case", ["se150", "pe150", "se251"])
def test_every_plan_gives_the_oracles_bytes(hip_lib, small_genome, cases, monkeypatch, case):
    _, img = small_genome
    reads, flag, want = cases[case]
    assert len(reads) == (3000 if case == "se150" else 300)
    for k, v in BESIDE.items():
        monkeypatch.setenv(k, v)
    opts = B.set_opt(hip_lib.default_options(), flag=flag)
    req = B.pack_request(reads)
    got = {}
    for name, env in SETTINGS:
        for k in ("BWAMEM_HIP_SEED_RESERVE", "BWAMEM_HIP_SEED_WPC"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        h = hip_lib.open_index(img)
        try:
            got[name] = hip_lib.align_raw(h, opts, req)
        finally:
            hip_lib.destroy_index(h)
        assert got[name] is not None, name
        if got[name] != want:
            sa, sb = B.split_response(got[name], len(reads)), B.split_response(want, len(reads))
            bad = [i for i in range(len(reads)) if sa[i] != sb[i]]
            pytest.fail("%s: %d/%d reads differ from the oracle; first: read %d" % (name, len(bad), len(reads), bad[0]))
    assert len(set(got.values())) == 1
