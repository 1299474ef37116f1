"""Tie-rich windowed and forced long pairs (tests/_ties.py) through every alignment kernel and through k_score.

The two rules of find_alignment that a kernel restates and can get subtly wrong are tie rules: the end-cell scan takes the FIRST maximum
(last row left to right, then the pos == end_a anti-diagonal downwards, strict '>': banded_smith_waterman.cc:174-212) and the traceback
prefers the diagonal, then GAP_A or GAP_B by column position (:217-311).  Random ACGT hardly ever ties; homopolymers, dinucleotide and
tandem repeats, complements do all the time, and with windows, force flags and N on them the end blocks, the strips re-created from
values, the run-skipping summary walk, k_align_w's reduction and k_score's (value, scan key) pair all get to decide.

Expected values come from the CPU oracle, which tests/test_oracle_vs_ref.py pins to the reference's own code on the whole `tie_windows`
group.  What ran is taken from gamdp_ctx_launch_info / gamdp_ctx_score_info.  Nothing here is built to fault: every input is a valid call.
"""
import os
import subprocess
import sys

import pytest

import _fillonly as F                 # want_of, run, cols_for: one statement of the end-cell rule
import _oracle as O
import _views as V
from _gpu import ctx, run_cases
from _ties import ALIGN_BANDS, LONG_BANDS, SCORE_BANDS, band_cases, long_cases, wants, what
import gam_ngs_amd as gam
from gam_ngs_amd import lib as L

pytestmark = pytest.mark.gpu

DIAG_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gam_ngs_amd", "libgamdp_diag.so")

assert {F.cols_for(b) for b in SCORE_BANDS} == {2, 3, 5, 9, 17}    # all five k_score<C> over the file


def check_align(cases, want, want_ops):
    """One gamdp_align_batch call: key and edit string of every call equal the oracle's -> the launches of the call.
    want_ops: one flag, or one per call."""
    res = run_cases(cases, want_ops=want_ops)
    info = ctx().launch_info()
    flags = list(want_ops) if isinstance(want_ops, (list, tuple)) else [bool(want_ops)] * len(cases)
    assert len(res) == len(cases) == len(want)
    for cs, r, (o, ops), f in zip(cases, res, want, flags):
        assert r.status != L.ST_DIAG_RANGE, what(cs)
        assert r.key() == o.key(), (what(cs), r.key(), o.key())
        assert r.ops == (ops if f else None), (what(cs), "edit string")
    return info


def surely_direction_free(cs):
    """A call that has a direction-free range whatever the rounding to blocks of 16 rows and groups of 4 blocks: between the row where
    the top blocks end (every cell has pos >= 1 and every lane is inside: at most max(64, band - begin_a + 1)) and the row where the
    end blocks begin (the last row, or the pos == end_a anti-diagonal entering the band at row end_a - begin_a - band) lie 18 blocks
    or more -- one block lost at either end, one tagged block in front, up to 3 + 3 for whole groups, 8 for the range to be worth it."""
    top = max(64, cs["band"] - cs["begin_a"] + 1)
    end = min(V.rows_of(cs) - 1, cs["end_a"] - cs["begin_a"] - cs["band"])
    return end - top >= 18 * 16


# ---- (a) every instantiation by band --------------------------------------------------------------------------------------------

GENERIC = {20: "k_align<2,-1,true>", 129: "k_align<5,-1,true>", 200: "k_align<9,-1,true>", 400: "k_align<17,-1,true>", 600: "k_align_w"}


@pytest.mark.parametrize("band", ALIGN_BANDS)
def test_every_instantiation_by_band(band):
    cases, want = band_cases(band), wants("band", band)
    n_ok = sum(1 for o, _ in want if o.status == O.OK)
    assert 2 * n_ok >= len(cases), (band, n_ok)
    infos = []
    for want_ops in (False, True):
        info = check_align(cases, want, want_ops)
        infos += info
        if band in (200, 400):   # direction-free ranges: at least the calls that have one by the rule above, and that ran (status OK)
            sure = sum(1 for cs, (o, _) in zip(cases, want) if o.status == O.OK and surely_direction_free(cs))
            assert sure >= 10, (band, sure)
            assert sum(r["units_dirfree"] for r in info) >= sure, (band, sure, info)
    if band == 150:
        # (a small band-150 batch with N in some windows goes to the N-aware kernel as a whole, gamdp_host.cpp route_merge_n:
        # the calls on sequences without N once more on their own)
        free = [k for k, cs in enumerate(cases) if b"N" not in cs["a"] + cs["b"]]
        assert 0 < len(free) < len(cases)
        for want_ops in (False, True):
            infos += check_align([cases[k] for k in free], [want[k] for k in free], want_ops)
    names = {r["kernel"] for r in infos}
    print("band %d: %d cases, %d OK, ran %s" % (band, len(cases), n_ok, sorted(names)))
    if band in GENERIC:
        assert names == {GENERIC[band]}, (band, infos)
    else:   # the tuned bands: the planner's choice, an N-aware and an N-free instantiation
        assert {bool(r["n_aware"]) for r in infos} == {False, True}, (band, infos)
        assert all(("<5,0," in n or "<19,15" in n) if band == 150 else "<17,4" in n for n in names), (band, names)


# ---- (b) long tuned shapes ------------------------------------------------------------------------------------------------------

def expected_cells():
    """The cells of tests/_views.py CELLS this process must run: the tuned kernels of the default environment, or what the parent of a
    child process names."""
    cells = os.environ.get("GAMDP_TIE_CELLS", "p17,c17n").split(",")
    for cell in cells:   # the environment CELLS gives for them is the one we are in
        assert all(os.environ.get(k) == v for k, v in V.CELLS[cell][3].items()), (cell, V.CELLS[cell][3])
    return cells


@pytest.mark.parametrize("band", LONG_BANDS)
def test_long_tuned_shapes(band):
    if os.environ.get("GAMDP_LIB"):
        assert gam.load_library().gamdp_build_info() & 1, "the child asked for the diagnostics build"
    cases, want = long_cases(band), wants("long", band)
    n_ok = sum(1 for (o, _), cs in zip(want, cases) if o.status == O.OK and cs["tag"][0] != "partner of")
    assert 4 * n_ok >= len(cases), (band, n_ok)     # (half of the tie-rich half)
    infos = []
    for want_ops in (False, True, [k % 3 == 0 for k in range(len(cases))]):
        infos += check_align(cases, want, want_ops)
    names = {r["kernel"] for r in infos}
    print("band %d: %d cases, %d tie-rich OK, ran %s, packed top units %d" % (band, len(cases), n_ok, sorted(names), sum(r["units_packed_top"] for r in infos)))
    for cell in expected_cells():
        kernel, bands = V.CELLS[cell][:2]
        if bands == (band,):
            assert kernel in names, (cell, kernel, names)
    if "k_align_p<17,4>" in names:
        assert sum(r["units_packed_top"] for r in infos) > 0, infos


# ---- (c) gamdp_score_batch ------------------------------------------------------------------------------------------------------

def check_scores(cases, want, band):
    got = F.run("score", ctx(), cases, ascii=True)
    assert len(got) == len(cases)
    for cs, g, (o, ops) in zip(cases, got, want):
        assert tuple(g) == F.want_of(o, ops), (what(cs), tuple(g), F.want_of(o, ops))
    info = ctx().score_info()
    assert [r["kernel"] for r in info] == ["k_score<%d>" % F.cols_for(band)], info
    print("band %d: %d scores, ran %s" % (band, len(cases), info[0]["kernel"]))


@pytest.mark.parametrize("band", SCORE_BANDS)
def test_scores_and_end_cells(band):
    check_scores(band_cases(band), wants("band", band), band)
    if band in LONG_BANDS:
        check_scores(long_cases(band), wants("long", band), band)


# ---- (d) the other ways through: (b) once more in a child process each -----------------------------------------------------------

OTHER_WAYS = {   # environment of the child -> the cells of tests/_views.py CELLS it must run
    "eight_and_four_tasks": (dict(GAMDP_QUAD_MIN="1"), "o19,q19n"),
    "four_tasks_int32": (dict(GAMDP_QUAD_MIN="1", GAMDP_NO_PAIR="1"), "q19"),
    "one_task_band512": (dict(GAMDP_NO_PAIR="1"), "c17"),
    "diagnostics_build": (dict(GAMDP_LIB=DIAG_LIB), "p17"),
    "diagnostics_build_eight_tasks": (dict(GAMDP_LIB=DIAG_LIB, GAMDP_QUAD_MIN="1"), "o19"),
}


@pytest.mark.parametrize("way", sorted(OTHER_WAYS))
def test_long_tuned_shapes_the_other_ways_through_in_a_fresh_process(way):
    """The switches are read once per process.  The two children on libgamdp_diag.so check, before every re-centring of a packed-f16
    block, that each live value lies inside the exact range, and report a violation as GAMDP_ST_DIAG_RANGE: no result may carry it."""
    if os.environ.get("GAMDP_TIE_CELLS"):
        pytest.skip("already inside the child")
    extra, cells = OTHER_WAYS[way]
    env = dict(os.environ, GAMDP_TIE_CELLS=cells, **extra)
    for k in ("GAMDP_QUAD_MIN", "GAMDP_NO_PAIR", "GAMDP_LIB"):
        if k not in extra:
            env.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-s", "-m", "gpu", os.path.abspath(__file__), "-k", "test_long_tuned_shapes"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (way, r.stdout[-2500:] + r.stderr[-2000:])
    print(way, [ln.lstrip(".") for ln in r.stdout.splitlines() if ln.lstrip(".").startswith("band ")])
    assert "2 passed" in r.stdout and "5 skipped" in r.stdout, r.stdout[-1500:]
