"""The two-task band-512 kernel (k_align_p<17,4>) keeps the halves of its plain and END ranges as integer bit patterns of f16 numbers
(gam_ngs_amd/csrc/kernel_pair.inc, "the pattern format"): the diag candidate is one 32-bit integer add for both tasks, the maximum is
v_pk_maximum3_f16 on the patterns, and what the strips read back from the slot is the same patterns.  Where the f16 form leaned on
-inf / NaN being absorbing, the integer form says so outright; this file goes for those places.

Every batch is band 512 and N-free through gamdp_align_batch; gamdp_ctx_launch_info must name k_align_p<17,4> with units_dirfree ==
units; every field and the edit string are compared with the CPU oracle (tests/_oracle.py).  The same batch goes through
gamdp_carry_batch, a kernel that shares no code with it, with all fields equal.  Every case has status OK in the oracle (asserted).
The shapes are the smallest that still reach every range: a 2 kb call at begin_a = 0 has top blocks, eight or more plain blocks and
the END range.  Nothing here is built to fault: every input is a valid call."""
import functools
import os
import random
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

import _cases
import _oracle as O
import _fillonly as F       # run / got_of: every field of gamdp_carry_batch's results
from _gpu import ctx, oracle_for, run_cases
from gam_ngs_amd import lib as L

pytestmark = pytest.mark.gpu

BAND = 512
DIAG_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gam_ngs_amd", "libgamdp_diag.so")


def case(a, b, begin_a=0, begin_b=0, end_a=None, end_b=None, fs=False, fe=False):
    return dict(a=a.encode(), b=b.encode(), band=BAND, begin_a=begin_a, end_a=len(a) - 1 if end_a is None else end_a,
                begin_b=begin_b, end_b=len(b) - 1 if end_b is None else end_b, fs=fs, fe=fe)


def light(rng, s):
    return _cases.mutate(rng, s, 0.02, 0.0, 0.0)   # substitutions only: the path stays on its column


def related(rng, n, begin_a=0, **kw):
    a = _cases.rand_seq(rng, begin_a + n)
    return case(a, _cases.mutate(rng, a[begin_a:]), begin_a=begin_a, **kw)


# ---- the batches: each is ONE gamdp_align_batch call, so the tasks named together share wavefronts ---------------------------------

@functools.lru_cache(maxsize=None)
def batches():
    rng = random.Random(51290)
    out = {}
    # all three ranges: 2 kb (top blocks, >= 8 plain blocks, END), 3 kb (one materialise() call spans groups of all three), 6.5 kb
    out["three_ranges"] = [related(rng, n) for n in (2000, 2000, 3000, 3000, 6500, 6500)]
    # extremes of growth
    ident = _cases.rand_seq(rng, 2600)
    tail = _cases.rand_seq(rng, 60)
    out["identical"] = [case(ident, ident), case(ident[::-1], ident[::-1])]                 # + 21 per row and column: the largest patterns
    out["no_match"] = [case("A" * 2600 + tail, "C" * 2600 + tail), case("G" * 2600 + tail, "T" * 2600 + tail)]   # + 12 per row (the tail makes it an alignment)
    # one 400-base insertion / deletion behind a displacement of 112: the path runs along band column 1 024 (lane LE, column CE: no
    # `up` source) / column 0 (lane 0: no `left` source); 1 500 bases behind the step, or the aligner would not pay for it
    s1, s2 = _cases.rand_seq(rng, 700), _cases.rand_seq(rng, 1500)
    p, ins = _cases.rand_seq(rng, 112), _cases.rand_seq(rng, 400)
    out["band_edges"] = [case(p + s1 + ins + s2, light(rng, s1) + light(rng, s2)), case(s1 + s2 + tail, p + light(rng, s1) + ins + light(rng, s2))]
    # tie-rich repeats
    unit17 = _cases.rand_seq(rng, 17)
    out["ties"] = [case("A" * 2600, "A" * 2590), case("AC" * 1300, "CA" * 1300), case(unit17 * 150, unit17 * 150), case("ACGT" * 650, "ACGT" * 640)]
    # both halves: an all-match task beside a no-match task; the lengths differ by a few rows, so whichever way the host sorts a
    # unit's tasks, the all-match task sits once in the low and once in the high halves
    out["halves_1"] = [case(ident[:2400], ident[:2400]), case("A" * 2403 + tail, "C" * 2403 + tail)]
    out["halves_2"] = [case(ident[:2470], ident[:2470]), case("A" * 2400 + tail, "C" * 2400 + tail)]
    # unequal ends: the two tasks of a unit end 50 blocks apart (the END range runs on past the shorter one's last row)
    out["unequal_ends"] = [related(rng, 2400), related(rng, 3200)]
    # windows
    out["no_top_blocks"] = [related(rng, 2600, begin_a=BAND + 64 + 100), related(rng, 2600, begin_a=BAND + 64 + 100)]
    out["inside_triangle"] = [related(rng, 2600, begin_a=200), related(rng, 2600, begin_a=200)]
    out["force_start"] = [related(rng, 2600, fs=True), related(rng, 2600, begin_a=300, fs=True)]
    out["force_end"] = [related(rng, 2600, fe=True), related(rng, 2600, fe=True)]
    out["mixed_begin_a"] = [related(rng, 2600, begin_a=0), related(rng, 2600, begin_a=330)]
    return out


@functools.lru_cache(maxsize=None)
def wants():
    """{name: [(oracle result, edit string)]}: computed once, every case OK"""
    flat = [(name, cs) for name, cases in batches().items() for cs in cases]
    with ThreadPoolExecutor(16) as ex:   # (the oracle's C code runs outside the GIL)
        res = list(ex.map(lambda nc: oracle_for(nc[1]), flat))
    out = {}
    for (name, cs), r in zip(flat, res):
        assert r[0].status == O.OK, (name, len(cs["a"]), len(cs["b"]), r[0].status)
        out.setdefault(name, []).append(r)
    return out


def path_columns(cs, o, ops):
    """the band columns the oracle's path visits"""
    x, pos = o.begin_b - cs["begin_b"], o.begin_a
    cols = set()
    for op in ops:
        cols.add(pos - cs["begin_a"] - x + BAND)
        x += op != "B"
        pos += op != "A"
    return cols


def test_the_cases_are_what_they_claim_to_be():
    w = wants()
    hi, lo = (path_columns(cs, *r) for cs, r in zip(batches()["band_edges"], w["band_edges"]))
    assert 2 * BAND in hi and 0 in lo, (max(hi), min(lo))
    for (o, ops), cs in zip(w["identical"], batches()["identical"]):
        assert set(ops) == {"M"} and o.length == len(cs["a"])
    for cs in batches()["no_match"]:
        assert not set(cs["a"][:2600]) & set(cs["b"][:2600])     # no match in any row before the tail
    rows = [len(cs["b"]) for cs in batches()["unequal_ends"]]
    assert 45 * 16 <= abs(rows[0] - rows[1]) <= 64 * 16


@pytest.mark.parametrize("name", sorted(batches()))
def test_batch_against_the_oracle_and_the_carry_kernel(name):
    cases, want = batches()[name], wants()[name]
    for want_ops in (True, False):
        res = run_cases(cases, want_ops=want_ops)
        info = ctx().launch_info()
        assert {r["kernel"] for r in info} == {"k_align_p<17,4>"}, info
        assert all(r["units_dirfree"] == r["units"] and r["units"] > 0 for r in info), info
        for k, (cs, r, (o, ops)) in enumerate(zip(cases, res, want)):
            assert r.status != L.ST_DIAG_RANGE, (name, k)
            assert r.key() == o.key(), (name, k, want_ops, r.key(), o.key())
            assert r.cells == o.cells, (name, k)
            assert r.ops == (ops if want_ops else None), (name, k, "edit string")
    carry = F.run("carry", ctx(), cases, ascii=True)
    assert carry == [F.got_of(o) for o, _ in want], name
    assert carry == [F.got_of(r) for r in res], name
    print(name, len(cases), "calls,", sum(r["units_packed_top"] for r in info), "units with packed top blocks,", sum(r["strips"] for r in info), "strip calls")


def test_the_diagnostics_build_sees_every_live_pattern_inside_its_range():
    """The same batches on libgamdp_diag.so in a fresh process (the library is chosen once per process): it compares every live pattern
    with both bounds before each re-centring and reports a violation as GAMDP_ST_DIAG_RANGE -- no result may carry it (asserted above)."""
    if os.environ.get("GAMDP_PATTERN_CELL_CHILD"):
        assert L.load_library().gamdp_build_info() & 1, "the child asked for the diagnostics build"
        return
    assert os.path.exists(DIAG_LIB), "libgamdp_diag.so is built with the product library"
    env = dict(os.environ, GAMDP_LIB=DIAG_LIB, GAMDP_PATTERN_CELL_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2500:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-1500:]
