"""gamdp_carry_ops_batch (k_carry_f, gam_ngs_amd/csrc/gamdp_carry_ops.hip): gamdp_carry_batch's result with the fingerprint of the
edit string the reference would return, from a fill alone.

In every test the results equal the CPU oracle's (or the golden key) and ops_fp[i] equals the fingerprint -- the three-line
definition (tests/_fpmodel.py: fp_def), not the library's function -- of the oracle's edit string where the status is OK and is 0
everywhere else (tests/_fillonly.py, kind "carry_ops").  The sections the call shares with the other fill-only calls -- views,
refusals, the other calls' records, few rows, all edge bands -- come from tests/_fillonly_sections.py.  The shapes are the smallest
that reach each piece of the kernel: every column count, the slow path and short fast ranges, the fast path of every instantiation,
fast ranges cut by the pos == end_a anti-diagonal, paths that cross many lane boundaries, the tie rule, N, views, and
gamdp_align_batch's own strings from every kernel that takes a band up to 543.  The counts asserted beside the results are the
oracle's alone.

Nothing here is built to fault: every input is a valid call, or one the library documents that it refuses on the host before any launch.
"""
import json
import os
import random
import subprocess
import sys

import pytest

import _cases
import _fillonly_sections as SEC
import _fillonly as S      # coded, cols_for, golden_l0, check_against_oracle, fp_of, got_of
import _oracle as O
import _views as V
from _gpu import ctx
import gam_ngs_amd as gam
from gam_ngs_amd import lib as L

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GAP_A, GAP_B = "A", "B"     # of O.OPS
fp_of, got_of = S.fp_of, S.got_of


def ok_strings(answers):
    return [ops for o, ops in answers if o.status == O.OK]


def check_against_oracle(cases, what):
    """-> [(oracle result, edit string)]"""
    return S.check_against_oracle("carry_ops", cases, what)


def launched_cols(c):
    return [r["cols"] for r in c.carry_ops_info()]


# ---- 1. the reference's golden vectors, against the reference's own edit strings -----------------------------------------------

def test_golden_l0_cases():
    cases, want = S.golden_l0("carry_ops")   # (673 of them)
    ok_by_cols = {}
    for cs, ((key, _), _) in zip(cases, want):
        if key[0] == O.OK:
            ok_by_cols[S.cols_for(cs["band"])] = ok_by_cols.get(S.cols_for(cs["band"]), 0) + 1
    assert ok_by_cols == {2: 426, 5: 82, 17: 1}, ok_by_cols
    S.check(cases, S.run("carry_ops", ctx(), cases), want, "golden l0")


# ---- 2. every column count: the slow path and short fast ranges ---------------------------------------------------------------

def test_random_cases_of_every_column_count():
    cases = [S.coded(cs) for cs in _cases.cases(20261020, 1300, max_len=700, bands=(1, 31, 63, 64, 95, 96, 150, 159, 160, 287, 288, 512, 543))]
    want = check_against_oracle(cases, "random")
    assert launched_cols(ctx()) == [2, 3, 5, 9, 17]
    assert len(ok_strings(want)) >= 0.8 * len(cases), len(ok_strings(want))
    for cols in (2, 3, 5, 9, 17):
        strings = [ops for cs, (o, ops) in zip(cases, want) if o.status == O.OK and S.cols_for(cs["band"]) == cols]
        counts = (len(strings), sum(1 for s in strings if GAP_A in s), sum(1 for s in strings if GAP_B in s))
        assert counts[0] >= 150 and counts[1] >= 80 and counts[2] >= 80, (cols, counts)
    distinct = set(ok_strings(want))
    assert len({fp_of(s) for s in distinct}) == len(distinct) > 1000   # (no collision among them: a wrong op anywhere would show)


# ---- 3. the fast path in every instantiation ----------------------------------------------------------------------------------

FAST_BANDS = (20, 80, 150, 250, 512)
assert [S.cols_for(b) for b in FAST_BANDS] == [2, 3, 5, 9, 17]


def whole_pair(a, b, band):
    return S.coded(dict(a=a.encode(), b=b.encode(), band=band, begin_a=0, end_a=len(a) - 1, begin_b=0, end_b=len(b) - 1, fs=False, fe=False))


def test_whole_pairs_long_enough_for_fast_blocks():
    """X and |a| beyond 2 band + 100 rows: FastRange (gamdp_score_common.inc) lets blocks of 32 row-times through fast_step"""
    rng = random.Random(20261020)
    cases = []
    for band in FAST_BANDS:
        for _ in range(8):
            a = _cases.rand_seq(rng, 2 * band + 400)
            cases.append(whole_pair(a, _cases.mutate(rng, a, 0.03, 0.01, 0.01), band))
    n_mut = len(cases)
    for band in FAST_BANDS:
        a = _cases.rand_seq(rng, 2 * band + 400)
        cases.append(whole_pair(a, a, band))
    want = check_against_oracle(cases, "fast")
    assert launched_cols(ctx()) == [2, 3, 5, 9, 17]
    assert all(o.status == O.OK for o, _ in want)
    mut = [ops for _, ops in want[:n_mut]]
    assert sum(1 for s in mut if GAP_A in s) >= 39 and sum(1 for s in mut if GAP_B in s) == 40, "gaps of both kinds inside the fast blocks"
    assert all(set(ops) == {"M"} for _, ops in want[n_mut:]), "the identical pairs"


# ---- 4. fast ranges cut by the pos == end_a anti-diagonal; paths that cross many lane boundaries -----------------------------

@pytest.mark.parametrize("band", [150, 512])
def test_window_cases_on_long_pairs(band):
    want = check_against_oracle([S.coded(cs) for cs in _cases.window_cases(3, band, count=40)], "windows")
    assert len(ok_strings(want)) >= 30


@pytest.mark.parametrize("band", [150, 512])
def test_paths_displaced_across_the_band(band):
    cases = [S.coded(cs) for cs in _cases.displaced_path_cases(band)]
    want = check_against_oracle(cases, "displaced")
    assert len(cases) == 32 and all(o.status == O.OK and GAP_A in ops and GAP_B in ops for o, ops in want)


# ---- 5. the tie rule --------------------------------------------------------------------------------------------------------------

def test_tie_rich_windows():
    cases = [S.coded(cs) for cs in _cases.tie_window_cases(5, FAST_BANDS, (300,), 4)]
    assert len(cases) == 240
    want = check_against_oracle(cases, "ties")
    for band in FAST_BANDS:
        assert sum(1 for cs, (o, _) in zip(cases, want) if cs["band"] == band and o.status == O.OK) >= 25, band


# ---- 6. N ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("band", [150, 512, 20])
def test_one_n_around_every_edge_of_the_window(band):
    cases = [dict(a=O.encode(a), b=O.encode(b), band=band, begin_a=ba, end_a=ea, begin_b=bb, end_b=eb, fs=False, fe=False)
             for a, b, ba, ea, bb, eb, _ in _cases.n_edge_cases(band)]
    want = check_against_oracle(cases, "n edges")
    assert all(o.status == O.OK for o, _ in want)


def test_n_runs_in_random_pairs():
    """an N on the diagonal is a MATCH (banded_smith_waterman.cc:239, :274): the flag that feeds n_match feeds the fingerprint"""
    rng = random.Random(20261021)
    cases = []
    for band in FAST_BANDS:
        for _ in range(6):
            a = _cases.rand_seq(rng, 2 * band + 300, 0.02)
            cases.append(whole_pair(a, _cases.sprinkle_n(rng, _cases.mutate(rng, a, 0.03, 0.01, 0.01), 0.01), band))
    want = check_against_oracle(cases, "n runs")
    assert all(o.status == O.OK and o.n_match == ops.count("M") for o, ops in want)
    assert all(4 in cs["a"] and 4 in cs["b"] for cs in cases)   # (code 4: N)


# ---- 7. the sections shared with the other fill-only calls: views, few rows, refusals, the other calls' records, all edge bands ----

globals().update(SEC.tests_for("carry_ops"))


# ---- 8. against gamdp_align_batch's own strings, from every kernel that takes a band up to 543 -------------------------------

ALIGN_CELLS = {k: v for k, v in V.CELLS.items() if max(v[1]) <= 543}
SWITCHES = ("GAMDP_QUAD_MIN", "GAMDP_NO_PAIR", "GAMDP_NO_MERGE_N", "GAMDP_WALK_SKIP", "GAMDP_OCTO_MIN_ROWS")
assert {v[0] for v in V.CELLS.values()} - {v[0] for v in ALIGN_CELLS.values()} == {"k_align_w"}


def _env_key(env):
    return tuple(sorted(env.items()))


def cells_for(env):
    return [k for k, v in ALIGN_CELLS.items() if _env_key(v[3]) == _env_key(env)]


def cell_pairs(cell):
    """two whole-sequence pairs of 3 to 6 kb at the cell's widest band, with runs of N where the cell is an N-aware kernel's"""
    name, bands, n_mode, _ = ALIGN_CELLS[cell]
    rng = random.Random("carry-ops/" + cell)
    out = []
    for n in (rng.randint(3000, 4200), rng.randint(4800, 6000)):
        a = _cases.rand_seq(rng, n, 0.002 if n_mode else 0.0)
        b = _cases.mutate(rng, a, 0.03, 0.01, 0.01)
        if n_mode:
            a, b = a[:n // 2] + "NNN" + a[n // 2 + 3:], b[:700] + "N" + b[701:]
        out.append(dict(a=a.encode(), b=b.encode(), band=max(bands), begin_a=0, end_a=len(a) - 1, begin_b=0, end_b=len(b) - 1, fs=False, fe=False))
    return out


def check_cell(c, cell, walk_skip=False):
    """gamdp_align_batch with edit strings on the cell's kernel, then gamdp_carry_ops_batch on the same tasks: every field and the
    fingerprint of the bytes the alignment kernel wrote"""
    name = ALIGN_CELLS[cell][0]
    cases = cell_pairs(cell)
    n = len(cases)
    sset = gam.SequenceSet(c, [s for cs in cases for s in (cs["a"], cs["b"])], ascii=True)
    calls = [(sset.contig(2 * i), cs["begin_a"], cs["end_a"], sset.contig(2 * i + 1), cs["begin_b"], cs["end_b"]) for i, cs in enumerate(cases)]
    bsw = gam.BandedSmithWaterman(c, cases[0]["band"])
    if walk_skip:
        c.set_walk_skip(L.WALK_SKIP_DIAG)
    try:
        al = bsw.find_alignments(calls, want_ops=True)
    finally:
        if walk_skip:
            c.set_walk_skip(L.WALK_STRIPS)
    info = c.launch_info()
    assert {r["kernel"] for r in info} == {name}, (cell, info)
    res, fps = bsw.find_results_with_ops_fingerprints(calls)
    sset.close()
    assert launched_cols(c) == [S.cols_for(cases[0]["band"])]
    for i in range(n):
        assert al[i].status == O.OK and 3000 <= len(al[i].ops) and ("A" in al[i].ops or "B" in al[i].ops), (cell, i)
        assert got_of(res[i]) == got_of(al[i]), (cell, i, got_of(res[i]), got_of(al[i]))
        assert fps[i] == fp_of(al[i].ops) == gam.ops_fingerprint(al[i].ops), (cell, i, fps[i], fp_of(al[i].ops))
    return name


def child_main():
    """Inside a fresh child process: the cells that need this process's planner switches."""
    env = {k: os.environ[k] for k in ("GAMDP_QUAD_MIN", "GAMDP_NO_PAIR") if k in os.environ}
    c = ctx()
    seen = {cell: check_cell(c, cell) for cell in cells_for(env)}
    if "o19" in seen:   # the eight-task kernel's opt-in walks that skip strips
        check_cell(c, "o19", walk_skip=True)
    print("CARRY_OPS_KERNELS " + json.dumps(seen))


DEFAULT_CELLS = cells_for({})
CHILD_ENVS = sorted({_env_key(v[3]) for v in ALIGN_CELLS.values() if v[3]})
SEEN = {}


@pytest.mark.parametrize("cell", DEFAULT_CELLS)
def test_fingerprints_of_the_strings_align_batch_wrote(cell):
    SEEN[cell] = check_cell(ctx(), cell)


def run_child(env):
    """A fresh child (never exec) with the planner switches the cells' kernels need, under its own timeout."""
    if all(cell in SEEN for cell in cells_for(dict(env))):
        return
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_carry_ops as T\nT.child_main()\n") % (os.path.dirname(HERE), HERE)
    full = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    full.update(dict(env))
    r = subprocess.run([sys.executable, "-c", code], env=full, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (env, r.stdout[-3000:] + r.stderr[-3000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("CARRY_OPS_KERNELS ")]
    assert line, r.stdout[-2000:]
    seen = json.loads(line[-1][len("CARRY_OPS_KERNELS "):])
    assert sorted(seen) == sorted(cells_for(dict(env))), seen
    SEEN.update(seen)


@pytest.mark.parametrize("env", CHILD_ENVS, ids=lambda e: "+".join("%s=%s" % kv for kv in e))
def test_fingerprints_of_the_strings_align_batch_wrote_in_a_fresh_process(env):
    run_child(env)


def test_zz_every_kernel_that_takes_bands_up_to_543_was_compared():
    """After the whole module (run alone, it runs what is missing): the kernels compared are those of kernel_info but k_align_w."""
    for cell in DEFAULT_CELLS:
        if cell not in SEEN:
            SEEN[cell] = check_cell(ctx(), cell)
    for env in CHILD_ENVS:
        run_child(env)
    assert set(SEEN) == set(ALIGN_CELLS)
    assert set(SEEN.values()) == V.kernel_names_in_source() - {"k_align_w"}
