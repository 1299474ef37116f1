"""CPU checks of the device-side edit-string fingerprints' C ABI (gamdp_task_ops_cap, gamdp_align_batch_fp,
gamdp_ctx_set_ops_chunk_bytes, gamdp_ops_fingerprint_batch, gamdp_ctx_ops_fp_info of include/gamdp.h): the library and the stand-in
library of integration/ export the five, the argument checks that need no GPU, and the bound gamdp_task_ops_cap states -- at least the
reference's edit-string length on the golden vectors, at least the oracle's on a few thousand random and edge calls, 0 exactly where
gamdp_task_preflight settles the call and a multiple of 16 otherwise, the stand-in's equal to the library's."""
import ctypes
import functools
import os
import random
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import _cases
import _golden as G
import _oracle as O
from gam_ngs_amd import api, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gamdp_task_ops_cap", "gamdp_align_batch_fp", "gamdp_ctx_set_ops_chunk_bytes", "gamdp_ops_fingerprint_batch", "gamdp_ctx_ops_fp_info")
U64 = ctypes.c_uint64
CAP_ARGS = [U64, U64, ctypes.c_uint32, U64, U64, U64, U64, ctypes.c_int, ctypes.c_int]
M64 = (1 << 64) - 1


def test_the_five_functions_are_exported_and_listed():
    l = lib.load_library()
    header = open(os.path.join(ROOT, "include", "gamdp.h")).read()
    for name in NAMES:
        assert name in lib.SYMBOLS and hasattr(l, name) and name + "(" in header
    assert hasattr(api.Context, "set_ops_chunk_bytes") and hasattr(api.Context, "ops_fp_info")
    assert hasattr(api.BandedSmithWaterman, "find_alignments_with_ops_fingerprints") and hasattr(api, "ops_fingerprint_many") and hasattr(api, "task_ops_cap")
    assert ctypes.sizeof(lib.OpsFpInfo) == 72


@functools.lru_cache(maxsize=1)
def stub():
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "stub.so")
        subprocess.check_call(["gcc", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-o", so, os.path.join(ROOT, "integration", "gamdp_stub.c")])
        s = ctypes.CDLL(so)   # (stays mapped after the file is gone)
    s.gamdp_task_ops_cap.argtypes = CAP_ARGS
    s.gamdp_task_ops_cap.restype = U64
    return s


def test_the_stand_in_library_exports_them():
    s = stub()
    fake = ctypes.cast(ctypes.create_string_buffer(8), ctypes.c_void_p)
    tasks, out, fp, info = (lib.Task * 1)(), (lib.Result * 1)(), (ctypes.c_uint32 * 1)(), lib.OpsFpInfo()
    off, ln = (U64 * 1)(), (U64 * 1)()
    assert s.gamdp_align_batch_fp(None, None, None, None, 0, None, None) == lib.EINVAL
    assert s.gamdp_align_batch_fp(fake, fake, fake, tasks, 1, out, fp) == lib.ENODEV
    assert s.gamdp_ctx_set_ops_chunk_bytes(None, U64(0)) == lib.EINVAL and s.gamdp_ctx_set_ops_chunk_bytes(fake, U64(4096)) == lib.ENODEV
    assert s.gamdp_ops_fingerprint_batch(None, None, None, None, 0, None) == lib.EINVAL
    assert s.gamdp_ops_fingerprint_batch(fake, b"\x02", off, ln, 1, fp) == lib.ENODEV
    assert s.gamdp_ctx_ops_fp_info(None, None) == lib.EINVAL and s.gamdp_ctx_ops_fp_info(fake, ctypes.byref(info)) == lib.ENODEV


def test_null_arguments_are_einval_before_anything_is_touched():
    l = lib.load_library()
    fake = ctypes.cast(ctypes.create_string_buffer(8), ctypes.c_void_p)   # (never read: every call below is refused on its NULLs)
    tasks, out, fp = (lib.Task * 1)(), (lib.Result * 1)(), (ctypes.c_uint32 * 1)()
    for args in ((None, fake, fake, tasks, 1, out, fp), (fake, None, fake, tasks, 1, out, fp), (fake, fake, None, tasks, 1, out, fp),
                 (fake, fake, fake, None, 1, out, fp), (fake, fake, fake, tasks, 1, None, fp), (fake, fake, fake, tasks, 1, out, None),
                 (fake, fake, fake, tasks, 0, out, None), (fake, fake, fake, None, 0, out, None), (None, None, None, None, 0, None, None)):
        assert l.gamdp_align_batch_fp(*args) == lib.EINVAL, args
    off, ln = (U64 * 1)(), (U64 * 1)()
    for args in ((None, b"\x02", off, ln, 1, fp), (fake, b"\x02", off, ln, 1, None), (fake, b"\x02", None, ln, 1, fp), (fake, b"\x02", off, None, 1, fp),
                 (fake, None, None, None, 0, None), (None, None, None, None, 0, fp)):
        assert l.gamdp_ops_fingerprint_batch(*args) == lib.EINVAL, args
    assert l.gamdp_ctx_set_ops_chunk_bytes(None, 0) == lib.EINVAL and l.gamdp_ctx_set_ops_chunk_bytes(None, 1 << 20) == lib.EINVAL
    info = lib.OpsFpInfo()
    assert l.gamdp_ctx_ops_fp_info(None, ctypes.byref(info)) == lib.EINVAL and l.gamdp_ctx_ops_fp_info(fake, None) == lib.EINVAL


def numbers(cs):
    return (len(cs["a"]), len(cs["b"]), cs["band"], cs["begin_a"] & M64, cs["end_a"] & M64, cs["begin_b"] & M64, cs["end_b"] & M64, int(cs["fs"]), int(cs["fe"]))


def check_cap(cs, status, length, what):
    """the bound on one call: the library's function, the Python binding and the stand-in's agree; 0 exactly where the pre-checks
    settle the call, otherwise a multiple of 16 that is at least `length` (of a call whose status is OK)"""
    cap = api.task_ops_cap(*numbers(cs))
    assert cap == stub().gamdp_task_ops_cap(*numbers(cs)), (what, numbers(cs))
    pre, _ = api.task_preflight(*numbers(cs))
    if pre != lib.ST_OK:
        assert cap == 0, (what, numbers(cs), pre, cap)
        assert status != lib.ST_OK, (what, numbers(cs), pre, status)
        return cap
    assert cap >= 16 and cap % 16 == 0, (what, numbers(cs), cap)
    if status == lib.ST_OK:
        assert length <= cap, (what, numbers(cs), length, cap)
        x = min(len(cs["b"]) - 1, cs["end_b"]) - cs["begin_b"] + 1
        assert cap <= 2 * x + 2 * cs["band"] + 15, (what, numbers(cs), cap)   # (the issue's starting point: 2 X + 2 band, before the view clips it)
    return cap


def test_the_bound_holds_on_the_golden_l0_cases():
    cases = G.l0_cases()
    assert len(cases) == 673
    n_ok = 0
    for name, cs, e in cases:
        check_cap(cs, e["status"], e["length"], name)
        n_ok += e["status"] == lib.ST_OK
        if e["status"] == lib.ST_OK:
            assert e["length"] == len(e["ops"])
    assert n_ok > 500


def edge_cases():
    """windows at the contig ends, forced starts and ends, bands 1 to 600 against short and long pairs"""
    rng = random.Random(600)
    out = []
    for band in (1, 2, 7, 31, 64, 150, 300, 512, 544, 600):
        for _ in range(40):
            n = rng.randint(20, 900)
            a, b = _cases.related_pair(rng, n, 0.0, div=rng.choice((0.0, 1.0, 3.0)))
            kind = rng.randrange(6)
            begin_a, end_a, begin_b, end_b = 0, len(a) - 1, 0, len(b) - 1
            if kind == 0:      # the window starts at the very end of a
                begin_a = max(0, len(a) - rng.randint(1, 12))
            elif kind == 1:    # ... of b
                begin_b = max(0, len(b) - rng.randint(1, 12))
            elif kind == 2:    # b outlasts a by more than the band: rows bounded by |a| + band - begin_a
                b = b + _cases.rand_seq(rng, band + rng.randint(1, 200))
                end_b = len(b) - 1
            elif kind == 3:    # a outlasts b: GAP_B runs along the last rows
                a = a + _cases.rand_seq(rng, 2 * band + rng.randint(1, 100))
                end_a = len(a) - 1
            elif kind == 4:    # begin_a inside the band's left triangle, unrelated prefix on b: GAP_A runs down column pos == 0
                begin_a = rng.randint(0, min(band, len(a) - 1))
                b = _cases.rand_seq(rng, rng.randint(1, 2 * band + 10)) + b
                end_b = len(b) - 1
            else:              # end_a short of the window: the anti-diagonal end cells
                end_a = rng.randint(0, len(a) - 1)
            out.append(dict(a=a.encode(), b=b.encode(), band=band, begin_a=begin_a, end_a=end_a, begin_b=begin_b, end_b=end_b,
                            fs=rng.random() < 0.3, fe=rng.random() < 0.3))
    return out


def test_the_bound_holds_on_random_and_edge_cases_against_the_oracle():
    cases = (_cases.cases(20261020, 2200, max_len=400, bands=(1, 2, 5, 8, 20, 63, 150, 288, 543, 600)) + _cases.beyond_cases(77, 400) + edge_cases())
    assert len(cases) >= 3000

    def one(cs):
        a, b = O.encode(cs["a"]), O.encode(cs["b"])
        o, _ = O.oracle_align(a, b, cs["band"], cs["begin_a"], cs["end_a"], cs["begin_b"], cs["end_b"], cs["fs"], cs["fe"], want_ops=False)
        return o.key()[0], o.key()[5]
    with ThreadPoolExecutor(16) as ex:   # (the oracle's C code runs outside the GIL)
        want = list(ex.map(one, cases))
    n_ok = n_settled = 0
    for cs, (status, length) in zip(cases, want):
        cap = check_cap(cs, status, length, "random")
        n_ok += status == lib.ST_OK
        n_settled += cap == 0
    assert n_ok >= 1800 and n_settled >= 300, (n_ok, n_settled)
