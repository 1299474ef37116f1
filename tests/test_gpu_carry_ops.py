"""gamdp_carry_ops_batch (k_carry_f, gam_ngs_amd/csrc/gamdp_carry_ops.hip): gamdp_carry_batch's result with the fingerprint of the
edit string the reference would return, from a fill alone.

In every test the results equal the CPU oracle's (or the golden key), as in tests/test_gpu_carry_batch.py, and ops_fp[i] equals the
fingerprint -- the three-line definition below, not the library's function -- of the oracle's edit string where the status is OK and is
0 everywhere else.  The shapes are the smallest that reach each piece of the kernel: every column count, the slow path and short
fast ranges, the fast path of every instantiation, fast ranges cut by the pos == end_a anti-diagonal, paths that cross many lane
boundaries, the tie rule, N, views, and gamdp_align_batch's own strings from every kernel that takes a band up to 543.  The counts
asserted beside the results are the oracle's alone.

Nothing here is built to fault: every input is a valid call, or one the library documents that it refuses on the host before any launch.
"""
import ctypes
import json
import os
import random
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

import _cases
import _golden
import _oracle as O
import _views as V
import test_gpu_score_batch as S      # coded, cols_for, edge_cases, view_cases, small_set, plain_tasks
from _gpu import ctx
import gam_ngs_amd as gam
from gam_ngs_amd import lib as L

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MULT = 0x9E3779B1
GAP_A, GAP_B = "A", "B"     # of O.OPS
FIELDS = tuple(f for f, _ in L.Result._fields_ if f != "pad_")


def fp_of(ops):
    """F(empty) = 0, F(s . e) = F(s) * M + (e + 1) mod 2^32 of an edit string over O.OPS"""
    f = 0
    for ch in ops:
        f = (f * MULT + O.OPS.index(ch) + 1) & 0xFFFFFFFF
    return f


def whole(r):
    """every field of a gamdp_result"""
    return tuple(getattr(r, f) for f in FIELDS)


def got_of(r):
    """(key, cells) of a MyAlignment / gamdp_result / oracle result"""
    return (tuple(r.key()), r.cells)


def oracle_wants(cases):
    """cases on code bytes -> [((key, cells), edit string)] of the oracle"""
    def one(cs):
        o, ops = O.oracle_align(cs["a"], cs["b"], cs["band"], cs["begin_a"], cs["end_a"], cs["begin_b"], cs["end_b"], cs["fs"], cs["fe"], want_ops=True)
        return got_of(o), ops
    with ThreadPoolExecutor(16) as ex:   # (the oracle's C code runs outside the GIL)
        return list(ex.map(one, cases))


def run_results(c, cases):
    """One gamdp_carry_ops_batch call over cases (on code bytes) that each bring their own pair of sequences -> [(key, cells)], [fingerprint]"""
    seqs = []
    for cs in cases:
        seqs += [cs["a"], cs["b"]]
    sset = gam.SequenceSet(c, seqs, ascii=False)
    calls = [(sset.contig(2 * i), cs["begin_a"], cs["end_a"], sset.contig(2 * i + 1), cs["begin_b"], cs["end_b"], cs["fs"], cs["fe"])
             for i, cs in enumerate(cases)]
    res, fps = gam.BandedSmithWaterman(c).find_results_with_ops_fingerprints(calls, bands=[cs["band"] for cs in cases])
    sset.close()
    assert all(r.ops is None for r in res) and len(fps) == len(res)
    return [got_of(r) for r in res], fps


def check(cases, got, fps, want, what):
    """want: [((key, cells), edit string)]; the fingerprint of a call whose status is not OK is 0"""
    assert len(got) == len(fps) == len(want) == len(cases)
    want_fp = [fp_of(ops) if w[0][0] == O.OK else 0 for w, ops in want]
    bad = [(i, got[i], fps[i], want[i][0], want_fp[i]) for i in range(len(cases)) if got[i] != want[i][0] or fps[i] != want_fp[i]]
    assert not bad, (what, len(bad), [(dict(cases[i], a=len(cases[i]["a"]), b=len(cases[i]["b"])), g, f, w, wf) for i, g, f, w, wf in bad[:3]])


def ok_strings(want):
    return [ops for w, ops in want if w[0][0] == O.OK]


def check_against_oracle(cases, what):
    got, fps = run_results(ctx(), cases)
    want = oracle_wants(cases)
    check(cases, got, fps, want, what)
    return want


def launched_cols(c):
    return [r["cols"] for r in c.carry_ops_info()]


# ---- 1. the reference's golden vectors, against the reference's own edit strings -----------------------------------------------

def test_golden_l0_cases():
    cases, want = [], []
    for name, cs, e in _golden.l0_cases():
        cc = S.coded(cs)
        o, _ = O.oracle_align(cc["a"], cc["b"], cs["band"], cs["begin_a"], cs["end_a"], cs["begin_b"], cs["end_b"], cs["fs"], cs["fe"], want_ops=False)
        cases.append(cc)
        want.append(((_golden.expect_key(e), o.cells), e["ops"]))   # (the golden vectors record no cell count)
    assert len(cases) == 673
    ok_by_cols = {}
    for cs, (w, _) in zip(cases, want):
        if w[0][0] == O.OK:
            ok_by_cols[S.cols_for(cs["band"])] = ok_by_cols.get(S.cols_for(cs["band"]), 0) + 1
    assert ok_by_cols == {2: 426, 5: 82, 17: 1}, ok_by_cols
    got, fps = run_results(ctx(), cases)
    check(cases, got, fps, want, "golden l0")


# ---- 2. every column count: the slow path and short fast ranges ---------------------------------------------------------------

def test_random_cases_of_every_column_count():
    cases = [S.coded(cs) for cs in _cases.cases(20261020, 1300, max_len=700, bands=(1, 31, 63, 64, 95, 96, 150, 159, 160, 287, 288, 512, 543))]
    want = check_against_oracle(cases, "random")
    assert launched_cols(ctx()) == [2, 3, 5, 9, 17]
    assert len(ok_strings(want)) >= 0.8 * len(cases), len(ok_strings(want))
    for cols in (2, 3, 5, 9, 17):
        strings = [ops for cs, (w, ops) in zip(cases, want) if w[0][0] == O.OK and S.cols_for(cs["band"]) == cols]
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
    assert all(w[0][0] == O.OK for w, _ in want)
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
    assert len(cases) == 32 and all(w[0][0] == O.OK and GAP_A in ops and GAP_B in ops for w, ops in want)


# ---- 5. the tie rule --------------------------------------------------------------------------------------------------------------

def test_tie_rich_windows():
    cases = [S.coded(cs) for cs in _cases.tie_window_cases(5, FAST_BANDS, (300,), 4)]
    assert len(cases) == 240
    want = check_against_oracle(cases, "ties")
    for band in FAST_BANDS:
        assert sum(1 for cs, (w, _) in zip(cases, want) if cs["band"] == band and w[0][0] == O.OK) >= 25, band


# ---- 6. N and views -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("band", [150, 512, 20])
def test_one_n_around_every_edge_of_the_window(band):
    cases = [dict(a=O.encode(a), b=O.encode(b), band=band, begin_a=ba, end_a=ea, begin_b=bb, end_b=eb, fs=False, fe=False)
             for a, b, ba, ea, bb, eb, _ in _cases.n_edge_cases(band)]
    want = check_against_oracle(cases, "n edges")
    assert all(w[0][0] == O.OK for w, _ in want)


def test_n_runs_in_random_pairs():
    """an N on the diagonal is a MATCH (banded_smith_waterman.cc:239, :274): the flag that feeds n_match feeds the fingerprint"""
    rng = random.Random(20261021)
    cases = []
    for band in FAST_BANDS:
        for _ in range(6):
            a = _cases.rand_seq(rng, 2 * band + 300, 0.02)
            cases.append(whole_pair(a, _cases.sprinkle_n(rng, _cases.mutate(rng, a, 0.03, 0.01, 0.01), 0.01), band))
    want = check_against_oracle(cases, "n runs")
    assert all(w[0][0] == O.OK and w[0][4] == ops.count("M") for w, ops in want)
    assert all(4 in cs["a"] and 4 in cs["b"] for cs in cases)   # (code 4: N)


@pytest.mark.parametrize("cell,band", S.VIEW_CELLS)
def test_views_equal_explicit_copies_equal_the_oracle(cell, band):
    c = ctx()
    cases = [cs for cs in S.view_cases() if cs["cell"] == cell]
    assert {tuple(cs["tag"]["kinds"]) for cs in cases} == set(V.KIND_PAIRS)   # the 16 rc / suffix combinations
    seqs = []
    for cs in cases:
        seqs += [cs["stored_a"], cs["stored_b"], cs["a"], cs["b"]]
    sset = gam.SequenceSet(c, seqs, ascii=False)
    calls = []
    for i, cs in enumerate(cases):
        calls.append((sset.contig(4 * i, *cs["va"]), cs["begin_a"], cs["end_a"], sset.contig(4 * i + 1, *cs["vb"]), cs["begin_b"], cs["end_b"], cs["fs"], cs["fe"]))
        calls.append((sset.contig(4 * i + 2), cs["begin_a"], cs["end_a"], sset.contig(4 * i + 3), cs["begin_b"], cs["end_b"], cs["fs"], cs["fe"]))
    res, fps = gam.BandedSmithWaterman(c, band).find_results_with_ops_fingerprints(calls)
    sset.close()
    res = [got_of(r) for r in res]
    want = oracle_wants(cases)
    want_fp = [fp_of(ops) if w[0][0] == O.OK else 0 for w, ops in want]
    bad = [(cs["tag"], res[2 * i], res[2 * i + 1], want[i][0], fps[2 * i], fps[2 * i + 1], want_fp[i]) for i, cs in enumerate(cases)
           if not (res[2 * i] == res[2 * i + 1] == want[i][0] and fps[2 * i] == fps[2 * i + 1] == want_fp[i])]
    assert not bad, (len(bad), bad[:3])
    assert len(ok_strings(want)) >= 0.9 * len(cases)
    assert launched_cols(c) == [S.cols_for(band)]


# ---- 7. against gamdp_align_batch's own strings, from every kernel that takes a band up to 543 -------------------------------

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


# ---- 8. refusals, and what the context reports ------------------------------------------------------------------------------------

def test_refusals_leave_the_context_usable():
    c = ctx()
    sset, seqs = S.small_set(c)
    n = 8
    out, fp = (L.Result * n)(), (ctypes.c_uint32 * n)()
    call = lambda tasks, cnt=n, s=sset, f=fp: c.lib.gamdp_carry_ops_batch(c.handle, s.handle, s.handle, tasks, cnt, out, f)  # noqa: E731
    good = S.plain_tasks(seqs, n)
    assert call(good) == 0, c.last_error()
    first, first_fp = [whole(r) for r in out], list(fp)
    assert all(r.status == O.OK and r.length > 0 for r in out) and all(first_fp) and first_fp[:4] == first_fp[4:]
    assert call(good, f=None) == L.EINVAL                        # NULL ops_fp
    assert call(good, 0, f=None) == L.EINVAL
    # a band above GAMDP_MAX_TUNED_BAND anywhere in the batch: the whole call, by name; then the same context again
    wide = S.plain_tasks(seqs, n)
    wide[5].band = 544
    assert call(wide) == L.ENOTSUP
    assert "gamdp_carry_ops_batch" in c.last_error() and "task 5" in c.last_error() and "544" in c.last_error(), c.last_error()
    assert call(good) == 0 and [whole(r) for r in out] == first and list(fp) == first_fp
    assert call(None, 0) == 0                                    # n == 0
    assert call(good, 0) == 0
    bad_id = S.plain_tasks(seqs, n)
    bad_id[3].b_id = 8
    assert call(bad_id) == L.EINVAL
    assert call(None, 1) == L.EINVAL
    synth = gam.SequenceSet.synthetic(c, 1, 2, 500)
    rc_task = (L.Task * 1)()
    rc_task[0].a_id, rc_task[0].b_id, rc_task[0].band, rc_task[0].b_rc = 0, 1, 20, 1
    rc_task[0].end_a, rc_task[0].end_b = 499, synth.lengths[1] - 1
    assert call(rc_task, 1, synth) == L.EINVAL                   # reverse complement of a packed-only set
    rc_task[0].b_rc = 0
    assert call(rc_task, 1, synth) == 0 and out[0].status == O.OK and fp[0] != 0
    # what the pre-checks settle keeps a fingerprint of 0, whatever the array held
    settled = S.plain_tasks(seqs, n)
    settled[2].begin_b = len(seqs[5]) + 7
    for k in range(n):
        fp[k] = 0xDEADBEEF
    assert call(settled) == 0 and out[2].status != O.OK and fp[2] == 0 and [fp[k] for k in range(n) if k != 2] == [first_fp[k] for k in range(n) if k != 2]
    assert call(good) == 0 and [whole(r) for r in out] == first and list(fp) == first_fp
    synth.close()
    sset.close()


def test_the_other_calls_records_stay_and_kernel_time_grows():
    c = ctx()
    sset, seqs = S.small_set(c)
    n = 8
    tasks = S.plain_tasks(seqs, n)
    res = (L.Result * n)()
    assert c.lib.gamdp_align_batch(c.handle, sset.handle, sset.handle, tasks, n, res, None) == 0, c.last_error()
    sc = (L.ScoreResult * n)()
    assert c.lib.gamdp_score_batch(c.handle, sset.handle, sset.handle, tasks, n, sc) == 0, c.last_error()
    ca = (L.Result * n)()
    assert c.lib.gamdp_carry_batch(c.handle, sset.handle, sset.handle, tasks, n, ca) == 0, c.last_error()
    before, before_score, before_carry = c.launch_info(), c.score_info(), c.carry_info()
    ms0, n0 = c.kernel_time()
    out, fp = (L.Result * n)(), (ctypes.c_uint32 * n)()
    assert c.lib.gamdp_carry_ops_batch(c.handle, sset.handle, sset.handle, tasks, n, out, fp) == 0, c.last_error()
    ms1, n1 = c.kernel_time()
    assert c.launch_info() == before and before and before[0]["kernel"].startswith("k_align")
    assert c.score_info() == before_score and [r["kernel"] for r in before_score] == ["k_score<2>"]
    assert c.carry_info() == before_carry and [r["kernel"] for r in before_carry] == ["k_carry<2>"]
    assert n1 == n0 + 1 and ms1 > ms0
    info = c.carry_ops_info()
    assert [(r["kernel"], r["cols"], r["tasks"], r["band_max"]) for r in info] == [("k_carry_f<2>", 2, n, 20)] and 0 < info[0]["slots"] <= n, info
    assert [whole(r) for r in out] == [whole(r) for r in ca] == [whole(r) for r in res]
    sset.close()


def test_a_batch_of_all_edge_bands_takes_five_launches():
    c = ctx()
    cases = [cs for band in S.EDGE_BANDS for cs in S.edge_cases(band)[:6]]
    check_against_oracle(cases, "all bands")
    info = c.carry_ops_info()
    assert [(r["kernel"], r["cols"]) for r in info] == [("k_carry_f<%d>" % k, k) for k in (2, 3, 5, 9, 17)], info
    assert [r["band_max"] for r in info] == [63, 95, 159, 287, 543], info
