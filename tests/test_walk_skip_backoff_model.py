"""gamdp_ctx_set_walk_skip_backoff without a GPU: the schedule (gamdp_walk_skip_backoff_hold, a host function that needs no context),
the rule as tests/_backoffmodel.py states it, the exported symbols and the layout of gamdp_walk_skip_backoff_stats.  Nothing here knows
the cap: it is whatever value the schedule stops growing at."""
import ctypes
import itertools
import random

import _backoffmodel as M
import _piecewise as P
from gam_ngs_amd import lib as L


def hold(f):
    return L.load_library().gamdp_walk_skip_backoff_hold(f)


def test_symbols_are_exported_and_the_struct_is_32_bytes():
    l = L.load_library()
    for name in ("gamdp_ctx_set_walk_skip_backoff", "gamdp_walk_skip_backoff_hold", "gamdp_ctx_walk_skip_backoff_stats"):
        assert name in L.SYMBOLS and hasattr(l, name), name
    assert ctypes.sizeof(L.WalkSkipBackoffStats) == 32
    S = L.WalkSkipBackoffStats
    assert (S.held.offset, S.held_pair.offset, S.held_i32.offset, S.mode.offset, S.pad_.offset) == (0, 8, 16, 24, 28)
    assert (L.WALK_BACKOFF_OFF, L.WALK_BACKOFF_ON) == (0, 1)
    # refusals that need no context: the mode is checked first, then the handle
    assert l.gamdp_ctx_set_walk_skip_backoff(None, L.WALK_BACKOFF_ON) == L.EINVAL
    assert l.gamdp_ctx_set_walk_skip_backoff(None, 2) == L.EINVAL
    assert l.gamdp_ctx_walk_skip_backoff_stats(None, ctypes.byref(S())) == L.EINVAL


def test_the_schedule():
    assert hold(0) == 0
    vals = [hold(f) for f in range(0, 80)]
    assert all(x <= y for x, y in zip(vals, vals[1:])), vals
    cap = hold(2 ** 32 - 1)              # no overflow at the largest argument: the value the schedule ends on
    assert cap == vals[-1] == hold(31) == hold(32) == hold(33) == hold(2 ** 31) >= 1, (cap, vals)
    for f, v in enumerate(vals):
        assert v == min(2 ** f - 1, cap), (f, v, cap)
    first_capped = next(f for f, v in enumerate(vals) if v == cap)
    assert all(v == cap for v in vals[first_capped:])
    assert all(v == 2 ** f - 1 for f, v in enumerate(vals[:first_capped]))


def test_all_pass_sequences_hold_nothing():
    for n in range(0, 40):
        assert M.simulate([True] * n, hold) == (n, 0)


def test_all_fail_sequences_test_or_hold_every_point():
    cap = hold(2 ** 32 - 1)
    for n in range(0, 200):
        tests, held = M.simulate([False] * n, hold)
        assert tests + held == n
        # by hand: test k (k = 1, 2, ...) is followed by hold(k) held points
        t = h = 0
        while t + h < n:
            t += 1
            h += min(hold(t), n - t - h)
        assert (tests, held) == (t, h), n
        if n >= 2:
            assert held > 0
        assert tests >= n // (cap + 1)


def test_a_pass_resets_the_schedule():
    # after any history that ends on a tested pass, the walk behaves like a fresh one
    rng = random.Random(5)
    seen = 0
    for _ in range(400):
        head = [rng.random() < 0.4 for _ in range(rng.randint(0, 30))]
        tail = [rng.random() < 0.4 for _ in range(rng.randint(0, 30))]
        t0, h0 = M.simulate(head, hold)
        t1, h1 = M.simulate(head + [True], hold)
        if t1 == t0 + 1:                 # the pass was tested, not held
            seen += 1
            tt, th = M.simulate(tail, hold)
            assert M.simulate(head + [True] + tail, hold) == (t1 + tt, h1 + th)
    assert seen >= 100
    # fail, held, pass, then fail, held, fail: the second failure is followed by hold(1) held points again, not by hold(2)
    assert hold(1) == 1
    assert M.simulate([False, False, True, False, False, False], hold) == (4, 2)
    # every sequence: each point is tested or held, and no point is held without a failed test in front of it
    for seq in itertools.product((False, True), repeat=8):
        tests, held = M.simulate(seq, hold)
        assert tests + held == 8 and (held == 0 or False in seq)


def test_piecewise_pairs_are_seeded_and_change_divergence_along_the_pair():
    a, b = P.pair(11, 9000)
    assert (a, b) == P.pair(11, 9000) and (a, b) != P.pair(12, 9000)
    assert len(a) == 9000 and set(a) <= set("ACGT") and set(b) <= set("ACGT")
    assert a[3000:5900] in b                        # the identical third is there as it is
    assert a[:200] not in b and a[6000:8000] not in b
    ra, rb = P.pair(11, 9000, reverse=True)
    assert ra == a and ra[3000:5900] in rb and ra[:2000] not in rb
    same = P.pair(3, 3000, rates=((0.0, 0.0, 0.0),))
    assert same[0] == same[1]
    _, only_sub = P.pair(3, 3000, rates=((0.05, 0.0, 0.0),))
    assert len(only_sub) == 3000 and 100 <= sum(x != y for x, y in zip(same[0], only_sub)) <= 220
