"""The LDS plan of the persistent seeding grid (csrc/kernels.h: seed_lds_plan), through bwamem_hip_seed_lds_plan: pure host
arithmetic, no GPU.  The plan must never book more than a CU has -- a seeding workgroup that does not fit stays pending in
the high-priority queue for a whole chunk -- and must leave the reserve it was asked for."""
import ctypes

import pytest

LDS_CU = 160 * 1024
K = 16
EL = 4 * 64 * 4                      # SEED_EL_CAP rows of 64 words
STAGE_LIMIT = 24576                  # reads are staged in LDS while 64 lanes x 4 bytes x ceil(len / 8) words fit here
# 36 .. 5 000 as the seeding kernel meets them; 768 / 769: the last length that is staged and the first that is not
LENGTHS = [(36, 1), (150, 1), (191, 1), (250, 1), (768, 1), (769, 1), (1022, 1), (1023, 0), (5000, 0)]
GRANULES = [1280, 1024, 512, 256]


@pytest.fixture(scope="module")
def plan(hip_lib):
    f = hip_lib.dll.bwamem_hip_seed_lds_plan
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int)]

    def call(lds_cu, granule, max_len, narrow, k, reserve):
        lds, wpc = ctypes.c_int64(-1), ctypes.c_int(-1)
        rc = f(lds_cu, granule, max_len, narrow, k, reserve, ctypes.byref(lds), ctypes.byref(wpc))
        return rc, lds.value, wpc.value
    return call


def _expected_lds(max_len, narrow):
    q = 64 * 4 * ((max_len + 7) // 8)
    return (5 * K * 32 if narrow else 3 * K * 64) * 4 + EL + (q if q <= STAGE_LIMIT else 0) + 16


def _round_up(x, g):
    return (x + g - 1) // g * g


@pytest.mark.parametrize("granule", GRANULES)
@pytest.mark.parametrize("max_len,narrow", LENGTHS)
def test_plan_fits_the_cu_and_leaves_the_reserve(plan, max_len, narrow, granule):
    lds = _expected_lds(max_len, narrow)
    alloc = _round_up(lds, granule)
    for n_res in (0, 1, 2):
        reserve = n_res * alloc
        rc, got_lds, wpc = plan(LDS_CU, granule, max_len, narrow, K, reserve)
        assert rc == 0 and got_lds == lds
        assert 1 <= wpc <= 16
        assert wpc * alloc + reserve <= LDS_CU
        assert wpc == 16 or (wpc + 1) * alloc + reserve > LDS_CU          # and no workgroup less than fits


@pytest.mark.parametrize("max_len,narrow", LENGTHS)
def test_reserve_zero_at_a_1024_byte_granule_is_the_former_formula(plan, max_len, narrow):
    lds = _expected_lds(max_len, narrow)
    former = max(1, min(16, LDS_CU // _round_up(lds, 1024)))
    assert plan(LDS_CU, 1024, max_len, narrow, K, 0) == (0, lds, former)


def test_150_bases(plan):
    assert _expected_lds(150, 1) == 16144
    assert plan(LDS_CU, 1024, 150, 1, K, 0) == (0, 16144, 10)
    # blocks of 1 280 bytes, as the device hands them out: 13 blocks per workgroup, nine workgroups -- ten do not fit
    assert plan(LDS_CU, 1280, 150, 1, K, 0) == (0, 16144, 9)
    assert plan(LDS_CU, 1280, 150, 1, K, 16640) == (0, 16144, 8)
    assert plan(LDS_CU, 1280, 150, 1, K, 2 * 16640) == (0, 16144, 7)


def test_a_reserve_one_workgroup_does_not_leave_is_cut(plan):
    rc, lds, wpc = plan(LDS_CU, 1280, 150, 1, K, 10 ** 6)
    assert (rc, lds, wpc) == (1, 16144, 1)
    rc, lds, wpc = plan(LDS_CU, 1280, 150, 1, K, LDS_CU - 16640)
    assert (rc, wpc) == (0, 1)
    rc, lds, wpc = plan(LDS_CU, 1280, 150, 1, K, LDS_CU - 2 * 16640)
    assert (rc, wpc) == (0, 2)


def test_bad_arguments(plan):
    assert plan(0, 1280, 150, 1, K, 0)[0] == -1
    assert plan(LDS_CU, 0, 150, 1, K, 0)[0] == -1
    assert plan(LDS_CU, 1280, -1, 1, K, 0)[0] == -1
    assert plan(LDS_CU, 1280, 150, 1, 12, 0)[0] == -1
    assert plan(LDS_CU, 1280, 150, 1, K, -1)[0] == -1
