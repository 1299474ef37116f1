"""The walk-skip properties when gamdp_align_batch goes through four pieces on two contexts (GAMDP_CHUNK_MIN=16): the owner hands its
modes to the helper context before the pieces run and adds the helper's counts to its own afterwards (gamdp_host.cpp).

One fresh child process (never exec) per family of tests/_walkskip.py, in the family's own environment plus GAMDP_CHUNK_MIN=16.  The
batch is 64 calls at the family's band -- the smallest in which each of the four pieces (an eighth, then three thirds of the rest: 8,
19, 19, 18 calls) still holds a whole eight-task unit -- of the two shortest lengths of the family's sizes(): a third identical pairs,
a third pairs with substitutions only, a third pairs with one indel at a group boundary.  It runs on ONE context with the family's
property in WALK_SKIP_DIAG and backoff ON, then with both off.  What the walks did is read from the three gamdp_ctx_walk_skip*_stats,
from gamdp_ctx_walk_skip_backoff_stats and from gamdp_ctx_launch_info, whose rows include the helper context's launches."""
import random

import pytest

import _cases
import _oracle as O
import _walkskip as W
from _walkskip import F
from gam_ngs_amd import lib as L

pytestmark = pytest.mark.gpu

FAMILIES = ("o19", "p17_one", "p17_side", "gen9")
N_CALLS = 64
PROPS = ("walk_skip", "walk_skip_pair", "walk_skip_i32")
HELD = ("held", "held_pair", "held_i32")


def batch():
    rng = random.Random(16)
    lengths = W.sizes()[:2]
    cases = []
    for k in range(N_CALLS):
        n = lengths[(k // 3) % 2]
        if k % 3 == 0:
            a = _cases.rand_seq(rng, n)
            cases.append(W.case(a, a, same=True))
        elif k % 3 == 1:
            a = _cases.rand_seq(rng, n)
            cases.append(W.case(a, W.substituted(rng, a, 0.02)))
        else:     # the indel in row 64 g, in the middle of the pair
            cases.append(W.one_indel(rng, n, 64 * max(1, n // 128), ("ins", "del")[(k // 6) % 2]))
    return cases


def child_pieces():
    c = W.ctx()
    cases = batch()
    want = W.oracle_all(cases)
    assert all(o.status == O.OK for o, _ in want)
    # (on the CPU: the identical pairs align without a gap, the pairs with an indel with one)
    assert all(W.gap_free(ops) for _, ops in want[0::3]) and not any(W.gap_free(ops) for _, ops in want[2::3])
    results = []
    for skip, backoff in ((L.WALK_SKIP_DIAG, L.WALK_BACKOFF_ON), (L.WALK_STRIPS, L.WALK_BACKOFF_OFF)):
        F.set(c, skip)
        c.set_walk_skip_backoff(backoff)
        try:
            res = W.run(cases, False)
        finally:
            F.set(c, L.WALK_STRIPS)
            c.set_walk_skip_backoff(L.WALK_BACKOFF_OFF)
        info, st, bo = c.launch_info(), F.stats(c), c.walk_skip_backoff_stats()
        others = {p: getattr(c, p + "_stats")() for p in PROPS if p != F.prop}
        print("  %s skip %d backoff %d: %s %s, %d launches in pieces %s" % (F.name, skip, backoff, st, bo, len(info), sorted({r["piece"] for r in info})))
        W.check_results(cases, res, want, [False] * N_CALLS, (skip, backoff))
        assert {r["piece"] for r in info} == {0, 1, 2, 3}, info
        rows = W.family_rows(info)
        assert st["strips"] == sum(r["strips"] for r in rows), (st, info)
        if F.prop == "walk_skip_i32":
            assert st["launches"] == len(rows), (st, info)
        if F.prop == "walk_skip_pair":
            assert st["launches_side_by_side"] + st["launches_one_by_one"] == len(rows), (st, info)
            W.check_path(st, info)
        assert st["mode"] == skip and bo["mode"] == backoff, (st, bo)
        if skip == L.WALK_SKIP_DIAG:
            assert all(st[k] > 0 for k in W.COUNTERS), st
            K = F.K() if callable(F.K) else F.K
            assert st["groups_skipped"] <= st["groups_tested"] <= K * st["tests"], st
            assert 64 * st["groups_skipped"] - 63 * st["tests"] <= st["rows_skipped"] <= 64 * st["groups_skipped"], st
        else:
            assert all(st[k] == 0 for k in W.COUNTERS) and bo[F.held] == 0, (st, bo)
        assert all(bo[h] == 0 for h in HELD if h != F.held), bo
        for p, other in others.items():
            # (gamdp_walk_skip_stats.mode is set at every call: the eight-task property's own mode)
            assert all(v == 0 for k, v in other.items() if (p, k) != ("walk_skip", "mode")), (p, other)
            assert other["mode"] == L.WALK_STRIPS, (p, other)
        results.append(res)
    W.check_equal(results[0], results[1])


CHILDREN = {"pieces": child_pieces}


@pytest.mark.parametrize("family", FAMILIES)
def test_four_pieces_on_two_contexts_count_as_one_call(family):
    W.run_child("test_gpu_walk_skip_pieces", "pieces", family, extra={"GAMDP_CHUNK_MIN": "16"}, timeout=300)
