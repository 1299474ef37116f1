"""CPU checks of gamdp_task_live_columns (include/gamdp.h): the library and the stand-in library of integration/ export it, the
Python mirror lists it, and its value is the brute force over rows and columns."""
import ctypes
import os
import subprocess

import numpy as np

import _carrywmodel as W
import _cases
from gam_ngs_amd import api, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_function_is_exported_and_listed():
    l = lib.load_library()
    assert "gamdp_task_live_columns" in lib.SYMBOLS and hasattr(l, "gamdp_task_live_columns") and hasattr(api, "task_live_columns")
    assert "uint64_t gamdp_task_live_columns(" in open(os.path.join(ROOT, "include", "gamdp.h")).read()


def test_the_stand_in_library_has_the_real_one(tmp_path):
    so = tmp_path / "stub.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-o", str(so),
                           os.path.join(ROOT, "integration", "gamdp_stub.c")])
    stub = ctypes.CDLL(str(so))
    # (the live width needs no device: the stand-in's is the real one)
    u64 = ctypes.c_uint64
    stub.gamdp_task_live_columns.argtypes = [u64, u64, ctypes.c_uint32, u64, u64, u64, u64, ctypes.c_int, ctypes.c_int]
    stub.gamdp_task_live_columns.restype = u64
    m64 = (1 << 64) - 1
    for args in _numbers():
        alen, blen, band, ba, ea, bb, eb, fs, fe = args
        assert stub.gamdp_task_live_columns(alen, blen, band, ba & m64, ea & m64, bb & m64, eb & m64, int(fs), int(fe)) == api.task_live_columns(*args), args


EDGE = [   # (alen, blen, band, begin_a, end_a, begin_b, end_b, fs, fe): begin_a far below and far above the band, a shorter than the band
    (50, 60, 1000, 0, 49, 0, 59, False, False), (50, 60, 1000, 49, 49, 0, 59, False, False), (50, 60, 1000, 1049, 2000, 0, 59, False, False),
    (50, 60, 1000, 1050, 2000, 0, 59, False, False), (50, 60, 1000, 1051, 2000, 0, 59, False, False), (50, 900, 1000, 700, 2000, 0, 899, False, False),
    (5000, 300, 3, 4000, 4999, 0, 299, False, False), (5000, 300, 3, 4998, 4999, 0, 299, False, False), (5000, 300, 3, 5002, 5010, 0, 299, False, True),
    (5000, 300, 3, 5003, 5010, 0, 299, False, False), (3000, 3000, 600, 0, 2999, 0, 2999, True, False), (3000, 3000, 600, 599, 2999, 0, 2999, False, False),
    (3000, 3000, 600, 600, 2999, 0, 2999, False, False), (3000, 3000, 600, 601, 2999, 0, 2999, False, True), (3000, 200, 600, 2900, 2999, 10, 150, False, False),
    (1, 1, 0, 0, 0, 0, 0, False, False), (1, 5, 2, 0, 0, 0, 4, False, False), (0, 5, 2, 0, 0, 0, 4, False, False), (7, 5, 2048, 3, 6, 1, 4, True, False),
    (4, 40, 2048, 0, 3, 0, 39, True, False), (40, 40, 150, 0, 39, 40, 45, False, False), (40, 40, 150, 0, 39, 5, 4, False, False),
    (40, 40, 150, (1 << 31) - 65536, 39, 0, 39, False, False), (1200, 1300, 544, 17, 1199, 3, 1299, False, True)]


def _numbers():
    out = []
    for cs in _cases.cases(20261021, 320, max_len=400, bands=(0, 1, 2, 63, 150, 543, 544, 600, 2048)):
        out.append((len(cs["a"]), len(cs["b"]), cs["band"], cs["begin_a"], cs["end_a"], cs["begin_b"], cs["end_b"], cs["fs"], cs["fe"]))
    return out + EDGE


def brute(alen, band, begin_a, X):
    """the definition: the largest number of cells with 0 <= begin_a + i + j - band < alen in one row i < X, 0 <= j <= 2 band -- a loop
    over the rows and, in numpy, over the columns of each"""
    best = 0
    j = np.arange(2 * band + 1, dtype=np.int64)
    for i in range(X):
        pos = begin_a + i + j - band
        best = max(best, int(np.count_nonzero((pos >= 0) & (pos < alen))))
    return best


def brute_py(alen, band, begin_a, X):
    return max(sum(1 for j in range(2 * band + 1) if 0 <= begin_a + i + j - band < alen) for i in range(X))


def test_the_live_width_is_the_brute_force_over_rows_and_columns():
    nums = _numbers()
    assert len(nums) > 300
    n_ok = n_settled = n_clamped = 0
    for args in nums:
        alen, blen, band, ba, ea, bb, eb, fs, fe = args
        got = api.task_live_columns(*args)
        st, _ = api.task_preflight(*args)
        st_model, X = W.preflight(alen, blen, band, ba, ea, bb, eb, fs, fe)
        if st != lib.ST_OK:
            assert got == 0, args
            n_settled += 1
            continue
        if ba > alen + band:   # (the model leaves these to its fill; the library settles them, above)
            continue
        assert st_model == W.OK
        want = brute(alen, band, ba, X)
        assert got == want == W.live_columns(alen, band, ba, X), (args, got, want)
        if band <= 150:
            assert brute_py(alen, band, ba, X) == got, args
        assert got <= min(2 * band + 1, alen), args
        assert (got == 0) == (alen == 0), args   # 0 exactly where the pre-checks settle the call (or a is empty: no cell at all)
        n_ok += 1
        n_clamped += got < 2 * band + 1
    assert n_ok > 150 and n_settled > 10 and n_clamped > 50, (n_ok, n_settled, n_clamped)


def test_the_two_widest_calls_by_closed_form():
    """the two widest calls of tests/test_gpu_l0_parity.py::test_the_limits_that_remain_for_wide_bands: the band exceeds |a| plus the rows on either side, so every row sees
    all of a and nothing else"""
    assert api.task_live_columns(40, 40, 1 << 20, 0, 39, 0, 4) == 40 == W.live_columns(40, 1 << 20, 0, 5)
    assert api.task_live_columns(300, 300, 100003, 7, 299, 2, 290, False, True) == 300 == W.live_columns(300, 100003, 7, 289)
    # and a long thin one: the whole band is live
    assert api.task_live_columns(9000, 9000, 2048, 0, 8999, 0, 8999) == 4097
    assert api.task_live_columns(6000, 6000, 544, 0, 5999, 0, 5999) == 1089
