"""gamdp_ctx_set_walk_skip_backoff: walks that make the diagonal test (gamdp_ctx_set_walk_skip, _pair, _i32) stop making it for a
while after tests that skipped nothing (kernel_walk.inc walk_many<..., SKIP>, kernel_finish.inc finish_walk<..., SKIP>; the rule is in
include/gamdp.h and, as ten lines of Python, in tests/_backoffmodel.py).

Every case runs on ONE context in three settings -- STRIPS, DIAG, DIAG + backoff: every field of every result equals the oracle's, and
the three runs are equal field by field (edit strings where asked for).  What the walks did is read from the family's
gamdp_ctx_walk_skip*_stats and from gamdp_ctx_walk_skip_backoff_stats.  The kernel families, each reached as its own test file reaches
it (the families and helpers of tests/_walkskip.py):

    o19       k_align_o<19,15>         band 150, GAMDP_QUAD_MIN=1                      test_gpu_walk_skip
    p17_one   k_align_p<17,4>          band 512, one task after the other              test_gpu_walk_skip_pair, GAMDP_SIDE_WALK_ROUNDS=0
    p17_side  k_align_p<17,4>          band 512, its two tasks side by side            ... GAMDP_SIDE_WALK_ROUNDS=1000000
    q19       k_align_q<19,15,false>   band 150                                        test_gpu_walk_skip_i32, cell q19
    gen9      k_align<9,-1,true>       band 200                                        ... cell gen9
    c17n      k_align<17,4,true>       band 512, one N in the pair                     ... cell c17n

The cases run in fresh child processes (never exec), each with a timeout of its own.  The cap of the schedule is not known here: the
expected counts come from tests/_backoffmodel.py driven by the library's own gamdp_walk_skip_backoff_hold."""
import os
import random

import pytest

import _backoffmodel as M
import _cases
import _oracle as O
import _piecewise as P
import _walkskip as W
import gam_ngs_amd as gam
from _walkskip import F, setup
from gam_ngs_amd import lib as L

pytestmark = pytest.mark.gpu

# family of tests/_walkskip.py -> copies of the all-fail pair in its batch
COPIES = {"o19": 16, "p17_one": 8, "p17_side": 8, "q19": 8, "gen9": 8, "c17n": 8}
FAMILIES = {name: W.FAMILIES[name] for name in COPIES}
COUNTERS = ("tests", "groups_tested", "groups_skipped", "rows_skipped", "strips")
SETTINGS = ((L.WALK_STRIPS, L.WALK_BACKOFF_OFF), (L.WALK_SKIP_DIAG, L.WALK_BACKOFF_OFF), (L.WALK_SKIP_DIAG, L.WALK_BACKOFF_ON))
ALL_FAIL_LEN = 11000     # at 32 groups a strip call (16 in the int32 kernels) a walk asks for 5 strips or more
PIECEWISE_LEN = 9000


# ---- in the child ------------------------------------------------------------------------------------------------------------------

def hold_of(f):
    return L.load_library().gamdp_walk_skip_backoff_hold(f)


def three(cases, want_ops=False, want=None):
    """The batch in the three SETTINGS on the family's context.  Every result equals the oracle's and the other settings'.
    -> (oracle answers, [(family stats, backoff stats, launch info)] per setting)"""
    c = W.ctx()
    want = want or W.oracle_all(cases)
    flags = list(want_ops) if isinstance(want_ops, (list, tuple)) else [bool(want_ops)] * len(cases)
    seen, results = [], []
    for skip, backoff in SETTINGS:
        F.set(c, skip)
        c.set_walk_skip_backoff(backoff)
        try:
            res = W.run(cases, want_ops)
        finally:
            F.set(c, L.WALK_STRIPS)
            c.set_walk_skip_backoff(L.WALK_BACKOFF_OFF)
        st, bo, info = F.stats(c), c.walk_skip_backoff_stats(), c.launch_info()
        assert st["mode"] == skip and bo["mode"] == backoff, (st, bo)
        assert F.kernel in {r["kernel"] for r in info}, (F.kernel, info)
        if F.prop == "walk_skip_pair":
            W.check_path(st, info)           # the walk path this child's environment asks for
        assert st["strips"] == W.family_strips(info)
        assert all(v == 0 for k, v in bo.items() if k not in ("mode", F.held)), bo
        if backoff == L.WALK_BACKOFF_OFF:
            assert bo[F.held] == 0, bo
        if skip == L.WALK_STRIPS:
            assert st["tests"] == st["groups_tested"] == st["groups_skipped"] == st["rows_skipped"] == 0, st
        W.check_results(cases, res, want, flags, (skip, backoff))
        seen.append((st, bo, info))
        results.append(res)
    for other in results[1:]:
        W.check_equal(results[0], other)
    print("  %s %d calls: strips %s, tests %s, groups skipped %s, held %d" %
          (F.name, len(cases), [s[0]["strips"] for s in seen], [s[0]["tests"] for s in seen], [s[0]["groups_skipped"] for s in seen], seen[2][1][F.held]))
    return want, seen


def child_gap_free():
    """1. the shapes on which the family's own test asserts strips == 0: nothing is held, and backoff changes no counter"""
    rng = random.Random(1)
    for n in W.sizes():
        a = _cases.rand_seq(rng, W.fit(n))
        cases = [W.case(a, a, same=True), W.case(a, W.substituted(rng, a, 0.02))]
        want = W.oracle_all(cases)
        assert all(o.status == O.OK and W.gap_free(ops) for o, ops in want)
        for want_ops in (False, True):
            _, ((st0, _, _), (st1, bo1, _), (st2, bo2, _)) = three(cases, want_ops, want)
            assert bo2[F.held] == 0, bo2
            assert [st1[k] for k in COUNTERS] == [st2[k] for k in COUNTERS], (st1, st2)
            if not want_ops:
                assert st0["strips"] > 0 and st1["strips"] == 0 and st1["groups_skipped"] > 0, (st0, st1)


def all_fail_pair(rng, n, period=40):
    """a pair whose alignment holds a gap every ~period rows, an insertion and a deletion in turn: the path stays within a column of the
    band's middle, and no 64 rows of it are free of gaps"""
    a = _cases.rand_seq(rng, n)
    b, at, k = [], 0, 0
    while at < n:
        step = period + rng.randint(-3, 3)
        seg = a[at:at + step]
        if at + step < n:
            # a base only b has / a base only a has -- never the neighbour's base, which would let the gap slide along a run of equal bases
            seg = seg + next(ch for ch in "ACGT" if ch != seg[-1] and ch != a[at + step]) if k % 2 == 0 else seg[:-1]
        b.append(seg)
        at += step
        k += 1
    return a, "".join(b)


def diagonal_runs(ops):
    runs, n = [], 0
    for ch in ops:
        if ch in "MX":
            n += 1
        else:
            runs.append(n)
            n = 0
    runs.append(n)
    return runs


def child_all_fail():
    """2. copies of one pair with a gap in every 64 rows of its path: every test below the end cell's first span fails, and the counts
    are those of the model"""
    rng = random.Random(2)
    a, b = all_fail_pair(rng, ALL_FAIL_LEN)
    cs = W.case(a, b)
    (o, ops), = W.oracle_all([cs])
    runs = diagonal_runs(ops)
    # on the CPU: no 64 consecutive diagonal steps anywhere on the path, so every 64-row window of it holds a gap -- the span below the
    # end cell (1 .. 64 rows, down to the next stored row) is the only one that can pass
    assert o.status == O.OK and o.length >= ALL_FAIL_LEN - 200 and max(runs) < 64 and len(runs) > ALL_FAIL_LEN // 50, (o.length, max(runs), len(runs))
    n = COPIES[F.name]
    cases, want = [cs] * n, [(o, ops)] * n
    _, ((st0, _, _), (st1, bo1, _), (st2, bo2, _)) = three(cases, False, want)
    assert st1["strips"] >= 4 * n, st1
    assert st1["strips"] == st2["strips"] and st1["groups_skipped"] == st2["groups_skipped"], (st1, st2)
    held = bo2[F.held]
    assert st2["tests"] + held == st1["tests"] and held > 0, (st1, st2, bo2)
    # one walk's outcomes without backoff, from the DIAG counters: the copies do the same
    assert st1["tests"] % n == 0 and st1["groups_skipped"] % n == 0, st1
    t, g = st1["tests"] // n, st1["groups_skipped"] // n
    assert g in (0, 1), st1                    # (the first span alone: every span of 64 rows holds a gap)
    tests, points_held = M.simulate([True] * g + [False] * (t - g), hold_of)
    print("  one walk: %d tests (%d passing), with backoff %d tests + %d held" % (t, g, tests, points_held))
    assert st2["tests"] == n * tests and held == n * points_held, (st2, bo2, tests, points_held)
    # a task that wants its edit string never tests and never holds
    _, (_, (st1, _, _), (st2, bo2, _)) = three(cases[:2], True, want[:2])
    assert st1["tests"] == st2["tests"] == 0 and bo2[F.held] == 0 and st2["strips"] > 0, (st1, st2, bo2)


def child_piecewise():
    """3. pairs whose divergence changes along the pair (tests/_piecewise.py), both orders: backoff still skips, never more than the
    plain test does, and asks for no more strips than a walk without the test"""
    for reverse in (False, True):
        cases = [W.case(*P.pair(100 + k, PIECEWISE_LEN, reverse=reverse)) for k in range(4)]
        want = W.oracle_all(cases)
        assert all(o.status == O.OK and 10 * o.length >= 9 * PIECEWISE_LEN for o, _ in want), [o.length for o, _ in want]
        _, ((st0, _, _), (st1, _, _), (st2, bo2, _)) = three(cases, False, want)
        assert st2["groups_skipped"] > 0, st2
        assert st2["groups_skipped"] <= st1["groups_skipped"], (st1, st2)
        assert st1["strips"] <= st2["strips"] <= st0["strips"], (st0, st1, st2)
        assert st2["tests"] + bo2[F.held] >= 1, (st2, bo2)
    three(cases, [True, False, False, True], want)


def child_properties():
    """4. refusals, the default and the environment default, backoff without a test to back off from, two contexts in different modes,
    merge blocks"""
    import ctypes
    setup("o19")
    l = L.load_library()
    st = L.WalkSkipBackoffStats()
    assert l.gamdp_ctx_set_walk_skip_backoff(None, L.WALK_BACKOFF_OFF) == L.EINVAL and l.gamdp_ctx_set_walk_skip_backoff(None, L.WALK_BACKOFF_ON) == L.EINVAL
    assert l.gamdp_ctx_walk_skip_backoff_stats(None, ctypes.byref(st)) == L.EINVAL
    c = W.ctx()
    assert l.gamdp_ctx_walk_skip_backoff_stats(c.handle, None) == L.EINVAL
    for mode in (-1, 2, 7):
        assert l.gamdp_ctx_set_walk_skip_backoff(c.handle, mode) == L.EINVAL
        with pytest.raises(gam.GamdpError):
            c.set_walk_skip_backoff(mode)
    assert c.walk_skip_backoff_stats() == dict(held=0, held_pair=0, held_i32=0, mode=0)
    # the mode of a fresh context: what its first call reports
    want_mode = L.WALK_BACKOFF_ON if os.environ.get("GAMDP_WALK_SKIP_BACKOFF") == "1" else L.WALK_BACKOFF_OFF
    rng = random.Random(4)
    a, b = all_fail_pair(rng, ALL_FAIL_LEN)
    fail8 = [W.case(a, b)] * 8
    want8 = W.oracle_all(fail8[:1]) * 8
    c.set_walk_skip(L.WALK_SKIP_DIAG)
    try:
        res = W.run(fail8, False)
    finally:
        c.set_walk_skip(L.WALK_STRIPS)
    bo = c.walk_skip_backoff_stats()
    assert [r.key() for r in res] == [o.key() for o, _ in want8]
    assert bo["mode"] == want_mode and (bo["held"] > 0) == (want_mode == L.WALK_BACKOFF_ON) and bo["held_pair"] == bo["held_i32"] == 0, bo
    print("ENV_MODE %d" % bo["mode"])
    if os.environ.get("GAMDP_WALK_SKIP_BACKOFF_TEST_ENV_ONLY"):
        return
    # backoff ON with the three skip properties OFF: no test, nothing held, every counter and every launch as without it
    x = _cases.rand_seq(rng, 5000)
    y = _cases.mutate(rng, x, 0.01, 0.002, 0.002)
    xn = x[:2500] + "N" + x[2501:]
    mk = lambda p, q, band: dict(a=p.encode(), b=q.encode(), band=band, begin_a=0, end_a=len(p) - 1, begin_b=0, end_b=len(q) - 1, fs=False, fe=False)
    mixed = fail8 + [mk(x, y, 512), mk(x, x, 512), mk(xn, y, 150), mk(x, y, 200)]
    wantm = want8 + W.oracle_all(mixed[8:])
    timeless = lambda info: [{k: v for k, v in r.items() if "ms" not in k} for r in info]
    seen = []
    for backoff in (L.WALK_BACKOFF_OFF, L.WALK_BACKOFF_ON):
        c.set_walk_skip_backoff(backoff)
        try:
            res = W.run(mixed, False)
        finally:
            c.set_walk_skip_backoff(L.WALK_BACKOFF_OFF)
        assert [r.key() for r in res] == [o.key() for o, _ in wantm]
        seen.append((timeless(c.launch_info()), c.walk_skip_stats(), c.walk_skip_pair_stats(), c.walk_skip_i32_stats(), c.walk_skip_backoff_stats()))
    assert seen[0][:4] == seen[1][:4], seen
    assert {r["kernel"] for r in seen[1][0]} >= {"k_align_o<19,15>", "k_align_p<17,4>", "k_align_q<19,15,true>", "k_align<9,-1,true>"}, seen[1][0]
    for s in seen:
        assert all(st["tests"] == st["groups_skipped"] == 0 for st in s[1:4]) and s[1]["strips"] > 0, s
    assert seen[0][4] == dict(held=0, held_pair=0, held_i32=0, mode=0) and seen[1][4] == dict(held=0, held_pair=0, held_i32=0, mode=1), seen
    # ... and with all four on, each family counts its own
    for name in ("walk_skip", "walk_skip_pair", "walk_skip_i32"):
        getattr(c, "set_" + name)(L.WALK_SKIP_DIAG)
    c.set_walk_skip_backoff(L.WALK_BACKOFF_ON)
    try:
        fail512 = [dict(cs, band=512) for cs in fail8[:2]]
        fail200 = [dict(cs, band=200) for cs in fail8[:1]]
        res = W.run(fail8 + fail512 + fail200, False)
        bo = c.walk_skip_backoff_stats()
    finally:
        for name in ("walk_skip", "walk_skip_pair", "walk_skip_i32"):
            getattr(c, "set_" + name)(L.WALK_STRIPS)
        c.set_walk_skip_backoff(L.WALK_BACKOFF_OFF)
    assert [r.key() for r in res] == [o.key() for o, _ in want8 + W.oracle_all(fail512 + fail200)]
    assert bo["held"] > 0 and bo["held_pair"] > 0 and bo["held_i32"] > 0 and bo["mode"] == 1, bo
    # gamdp_multi: two contexts on one device, both with the test, one of them with backoff
    seqs = []
    for k in fail8:
        seqs += [k["a"], k["b"]]
    m = gam.MultiContext([0, 0])
    m.set_walk_skip(L.WALK_SKIP_DIAG)
    m.set_walk_skip_backoff(L.WALK_BACKOFF_ON, which=1)
    ms = gam.MultiSequenceSet(m, seqs, ascii=True)
    calls = [(ms.contig(2 * i), k["begin_a"], k["end_a"], ms.contig(2 * i + 1), k["begin_b"], k["end_b"], False, False) for i, k in enumerate(fail8)]
    res = gam.BandedSmithWaterman(m).find_alignments(calls, bands=[150] * len(fail8))
    sts, bos = m.walk_skip_stats(), m.walk_skip_backoff_stats()
    ms.close()
    m.close()
    assert [r.key() for r in res] == [o.key() for o, _ in want8]
    assert [s["mode"] for s in bos] == [L.WALK_BACKOFF_OFF, L.WALK_BACKOFF_ON] and [s["mode"] for s in sts] == [L.WALK_SKIP_DIAG] * 2, (sts, bos)
    assert bos[0]["held"] == 0 and bos[1]["held"] > 0 and sts[0]["tests"] > 0 and sts[1]["tests"] > 0, (sts, bos)
    # gamdp_align_merge_blocks: gamdp_mb_out and the audit do not depend on it
    import _l1cases
    import test_gpu_l1_chain_carry as TC
    scs = _l1cases.scenarios(900, 24)
    outs = []
    for skip, backoff in SETTINGS:
        c.set_walk_skip(skip)
        c.set_walk_skip_i32(skip)
        c.set_walk_skip_backoff(backoff)
        try:
            stats = TC.check(c, scs)             # against the oracle's driver, audit included
            outs.append([TC.outcome(mb) for mb in TC.run(c, scs)])
        finally:
            c.set_walk_skip(L.WALK_STRIPS)
            c.set_walk_skip_i32(L.WALK_STRIPS)
            c.set_walk_skip_backoff(L.WALK_BACKOFF_OFF)
        assert stats["ok"] >= 3, stats
    assert outs[0] == outs[1] == outs[2]


CHILDREN = {f.__name__[len("child_"):]: f for f in (child_gap_free, child_all_fail, child_piecewise, child_properties)}


# ---- the tests: one fresh child each (never exec) --------------------------------------------------------------------------------

def run_child(name, family=None, diag=False, extra=None):
    return W.run_child("test_gpu_walk_skip_backoff", name, family, diag, extra, timeout=300)


FAMS = pytest.mark.parametrize("family", sorted(FAMILIES))
LIBS = pytest.mark.parametrize("diag", (False, True), ids=("product", "diag"))


@FAMS
@LIBS
def test_gap_free_pairs_hold_nothing(family, diag):
    run_child("gap_free", family, diag)


@FAMS
@LIBS
def test_every_test_fails_and_the_counts_are_the_models(family, diag):
    """Fails without the feature: held > 0, and tests + held is what the plain test counts."""
    run_child("all_fail", family, diag)


@FAMS
@LIBS
def test_piecewise_pairs_in_both_orders(family, diag):
    run_child("piecewise", family, diag)


def test_refusals_default_no_skip_property_two_contexts_and_merge_blocks():
    assert "ENV_MODE 0" in run_child("properties", extra={"GAMDP_QUAD_MIN": "1"})


def test_the_environment_default():
    only = {"GAMDP_QUAD_MIN": "1", "GAMDP_WALK_SKIP_BACKOFF_TEST_ENV_ONLY": "1"}
    assert "ENV_MODE 1" in run_child("properties", extra=dict(only, GAMDP_WALK_SKIP_BACKOFF="1"))
    assert "ENV_MODE 0" in run_child("properties", extra=dict(only, GAMDP_WALK_SKIP_BACKOFF="0"))
