"""The merge-block driver with its tail alignments seeded by findHits on the GPU (gamdp_ctx_set_l1_hits(GAMDP_L1_HITS_DEVICE)):
every merge block stored in tests/golden/l1_vs_ref.json.gz must give the reference's outcome, coordinates, n_dp, cells and DP
trail -- and, where the whole trail is stored, each tail call's seed (the window's begin_a) -- whichever way the call goes: the setter, the environment switch,
several cohorts, the round loop, a MultiContext, and an arena so small that a query falls back to the host.  Host mode must
stay byte for byte what it is.  The summary kernel (k_hits_summary: no hit list) is checked on its own against the list path
and the host on the reduction's edge shapes."""
import json
import os
import random
import subprocess
import sys

import pytest

import _cases
import _gage
import _gpu
import _hitsq as Q
import _l1hits as H
import test_l1_oracle_vs_ref as T
import gam_ngs_amd as gam
from gam_ngs_amd import api, lib

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DIAG_LIB = os.path.join(os.path.dirname(lib.library_path()), "libgamdp_diag.so")
SWITCHES = ("GAMDP_L1_ROUNDS", "GAMDP_L1_NO_TWINS", "GAMDP_L1_COHORTS", "GAMDP_L1_COHORT_MIN", "GAMDP_L1_DEVICE_HITS",
            "GAMDP_DIAG_HITS_DROP", "GAMDP_LIB")


@pytest.fixture(scope="module")
def device_ctx():
    c = gam.Context(0)
    c.set_l1_hits(lib.L1_HITS_DEVICE)
    yield c
    c.close()


def test_golden_parity_with_device_hits(device_ctx):
    n, diffs, n_tail, st, _ = H.run_groups(device_ctx, list(T.GROUPS), lambda: [device_ctx.l1_hits_stats()])
    assert n >= 1700 and not diffs, diffs[:5]
    assert st["mode"] == lib.L1_HITS_DEVICE
    assert st["device_queries"] > 0 and st["host_queries"] == 0 and st["host_fallback"] == 0, st
    assert st["tail_queries"] == st["device_queries"] + st["trivial_queries"], st
    assert st["tail_queries"] == n_tail and n_tail > 500, (st, n_tail)
    assert st["seeds"] > 600, st   # tail calls whose seed was compared with the stored window's begin_a
    assert st["hits_launches"] >= 3


def test_host_mode_is_unchanged(device_ctx):
    host = gam.Context(0)
    host.set_l1_hits(lib.L1_HITS_HOST)
    for group in ("edges", "seeded_500", "gage_32"):
        cases = [c for c, a in zip(T.GROUPS[group](), T.stored(group, T.GROUPS[group]())) if a is not None]
        out_h, aud_h, _ = H.raw_call(host, cases)
        st = host.l1_hits_stats()
        assert st["mode"] == lib.L1_HITS_HOST and st["device_queries"] == 0 and st["hits_launches"] == 0, st
        assert st["host_queries"] == st["tail_queries"] > 0 and st["trivial_queries"] == st["host_fallback"] == 0, st
        out_d, aud_d, _ = H.raw_call(device_ctx, cases)
        assert out_d == out_h and aud_d == aud_h, group
        assert device_ctx.l1_hits_stats()["tail_queries"] == st["tail_queries"]
    host.close()


# ---- the summary kernel ------------------------------------------------------------------------------------------------

SIZES = (1, 63, 64, 65, 255, 256, 257, 3000, 5121)   # nf: below / at / above a wavefront and a workgroup, and many rounds of one


def _edge_queries():
    """(seqs, queries): for every nf of SIZES, with word 1 (one b k-mer "C": diagonal i holds a vote iff a[i] is C): the maximum
    on every diagonal, on the first and the last alone, on the first alone, on the last alone, in the middle, nowhere
    (all-zero votes); and, with word 20, a related pair."""
    rng = random.Random(11)
    seqs, queries = [], []

    def add(a, b, word):
        i = len(seqs) // 2
        seqs.extend([api.encode(a), api.encode(b)])
        queries.append((2 * i, False, 0, 0, Q.M64, 2 * i + 1, False, 0, 0, Q.M64, word))

    for nf in SIZES:
        add("C" * nf, "C", 1)
        add("C" + "A" * (nf - 2) + "C" if nf > 1 else "C", "C", 1)
        add("C" + "A" * (nf - 1), "C", 1)
        add("A" * (nf - 1) + "C", "C", 1)
        add("A" * (nf // 2) + "C" + "A" * (nf - nf // 2 - 1), "C", 1)
        add("A" * nf, "C", 1)
        if nf >= 63:
            a = _cases.rand_seq(rng, nf, 0)
            add(a, _cases.mutate(rng, a[nf // 3:], 0.02, 0.005, 0.005), 20)
            # two copies of b in a: a tie between two diagonals far apart
            b = _cases.rand_seq(rng, 25, 0)
            if nf >= 255:
                add(b + _cases.rand_seq(rng, nf - 50, 0) + b, b, 20)
    return seqs, queries


def _check_summaries(seqs, queries):
    ctx = _gpu.ctx()
    sset = gam.SequenceSet(ctx, seqs, ascii=False)
    calls = [(sset.contig(q[0], q[1], q[2]), q[3], q[4], sset.contig(q[5], q[6], q[7]), q[8], q[9]) for q in queries]
    words = [q[10] for q in queries]
    ab = gam.ABlast()
    sums = ab.find_hits_many(ctx, calls, want_hits=False, words=words)          # k_hits_summary
    lists = ab.find_hits_many(ctx, calls, caps=[8] * len(calls), words=words)   # k_hits_collect + k_hits_gather
    sset.close()
    n_hit = 0
    for k, (q, s) in enumerate(zip(queries, sums)):
        a, b = Q.view(seqs[q[0]], q[1], q[2]), Q.view(seqs[q[5]], q[6], q[7])
        want = gam.ABlast(q[10]).findHits(a, q[3], q[4], b, q[8], q[9])
        assert s[:3] == (len(want), want[0] if want else 0, want[-1] if want else 0), (k, q, s)
        assert lists[k] == want[:8], (k, q)
        if len(a) <= 6000:
            assert s[3] == Q.py_find_hits(a, q[3], q[4], b, q[8], q[9], q[10])[1], (k, q, s)
        n_hit += bool(want)
    return sums, n_hit


def test_summary_kernel_on_the_reductions_edge_shapes():
    seqs, queries = _edge_queries()
    sums, _ = _check_summaries(seqs, queries)
    k = 0
    for nf in SIZES:
        # (n_hits, first, last, votes) of the six word-1 shapes
        assert sums[k] == (nf, 0, nf - 1, 1)
        assert sums[k + 1] == (min(nf, 2), 0, nf - 1, 1)
        assert sums[k + 2] == (1, 0, 0, 1)
        assert sums[k + 3] == (1, nf - 1, nf - 1, 1)
        assert sums[k + 4] == (1, nf // 2, nf // 2, 1)
        assert sums[k + 5] == (0, 0, 0, 0)
        k += 6 + (nf >= 63) + (nf >= 255)
        if nf >= 255:
            assert sums[k - 1][:3] == (2, 0, nf - 25)
    assert k == len(queries)


def test_summary_kernel_on_the_with_hit_list_paths_summaries():
    """hits_buf == NULL against the summaries the list path returns, on the tail windows of a GAGE-shaped problem"""
    pb = _gage.problem(3)
    seqs, queries = Q.tail_queries(pb)
    ctx = _gpu.ctx()
    sset = gam.SequenceSet(ctx, seqs, ascii=False)
    n = len(queries)
    tasks = (lib.HitsTask * n)()
    for t, q in zip(tasks, queries):
        t.a_id, t.a_rc, t.a_off, t.a_start, t.a_end = q[0], int(q[1]), q[2], q[3] & Q.M64, q[4] & Q.M64
        t.b_id, t.b_rc, t.b_off, t.b_start, t.b_end, t.word = q[5], int(q[6]), q[7], q[8] & Q.M64, q[9] & Q.M64, q[10]
    import ctypes as C
    out0, out1 = (lib.HitsResult * n)(), (lib.HitsResult * n)()
    buf, zeros = (C.c_uint32 * 1)(), (C.c_uint64 * n)()
    assert ctx.lib.gamdp_find_hits_batch(ctx.handle, sset.handle, sset.handle, tasks, n, out0, None, None, None) == 0
    assert ctx.lib.gamdp_find_hits_batch(ctx.handle, sset.handle, sset.handle, tasks, n, out1, buf, zeros, zeros) == 0
    sset.close()
    assert n > 50 and bytes(out0) == bytes(out1)
    seeded = 0
    for q, o in zip(queries, out0):
        a, b = Q.view(seqs[q[0]], q[1], q[2]), Q.view(seqs[q[5]], q[6], q[7])
        want = gam.ABlast(q[10]).findHits(a, q[3], q[4], b, q[8], q[9])
        assert (o.n_hits, o.first, o.last) == (len(want), want[0] if want else 0, want[-1] if want else 0), q
        seeded += bool(want)
    assert seeded > n // 4


# ---- a query that does not fit the cohort's share of the arena -------------------------------------------------------------

FALLBACK_GROUP = "gage_32"


def test_a_query_too_big_for_the_arena_share_falls_back_to_the_host():
    """gage_32: 36 merge blocks (one cohort), four tail calls whose findHits queries need 3 929, 252 969, 254 271 and 255 657
    words of scratch (words = 3 * cap + 2 + na + nf: the three long ones have na of 28 170 .. 29 514 a k-mers, cap 65 536).  The
    arena is set to 4 * (255 657 - 1) = 1 022 624 bytes: the cohort's share is that while no chain launch runs and half of it
    beside one, so the longest query exceeds it either way, by one word at least; the DP calls of this group fit 700 KB
    (tests/test_gpu_l1_vs_ref.py) and so a share of 1 MB -- and the call says so loudly if one does not."""
    cases = T.GROUPS[FALLBACK_GROUP]()
    answers = T.stored(FALLBACK_GROUP, cases)
    words = sorted(H.golden_tail_words(answers))
    assert len(cases) < 48 and all("trail" in a for a in answers if a)   # one cohort; every tail call is in a stored trail
    assert words[-1] > 200_000 and words[0] < 10_000, words
    arena = 4 * (words[-1] - 1)
    c = gam.Context(0)
    c.set_l1_hits(lib.L1_HITS_DEVICE)
    c.set_arena_bytes(arena)
    try:
        n, diffs, n_tail, st, cohorts = H.run_groups(c, [FALLBACK_GROUP], lambda: [c.l1_hits_stats()])
    finally:
        c.set_arena_bytes(0)
        c.close()
    assert cohorts == 1 and n >= 30 and not diffs, diffs[:5]
    assert st["host_fallback"] >= 1 and st["host_queries"] == 0, st
    assert st["tail_queries"] == n_tail == len(words) == st["device_queries"] + st["trivial_queries"] + st["host_fallback"], (st, words)
    # exactly the queries larger than the share fall back: at least the largest, at most those above half the arena
    assert st["host_fallback"] <= sum(1 for w in words if 4 * w > arena // 2), (st, words)


# ---- other ways through a call, in fresh processes (the switches are read once per process) --------------------------------

def _child(groups, how, env, libpath=None):
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    e.update(env)
    if libpath:
        e["GAMDP_LIB"] = libpath
    r = subprocess.run([sys.executable, os.path.join(HERE, "_l1hits.py"), groups, how], env=e, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-2500:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("how,env,cohorts", [
    ("setter", {"GAMDP_L1_COHORTS": "3", "GAMDP_L1_COHORT_MIN": "8"}, 3),
    ("setter", {"GAMDP_L1_ROUNDS": "1"}, 1),
    ("setter", {"GAMDP_L1_ROUNDS": "1", "GAMDP_L1_COHORTS": "2", "GAMDP_L1_COHORT_MIN": "8"}, 2),
    ("env", {"GAMDP_L1_DEVICE_HITS": "1"}, 1),
], ids=["cohorts3", "rounds", "rounds-cohorts2", "env-switch"])
def test_other_ways_through_a_call_in_a_fresh_process(how, env, cohorts):
    r = _child("gage_33,edges", how, env)
    st = r["stats"]
    assert r["n"] >= 130 and r["n_diffs"] == 0, r
    assert r["cohorts"] >= cohorts, r
    assert st["mode"] == lib.L1_HITS_DEVICE and st["device_queries"] > 50 and st["host_queries"] == st["host_fallback"] == 0, r
    assert st["tail_queries"] == r["tail_calls"] == st["device_queries"] + st["trivial_queries"], r


def test_the_switch_unset_is_host_mode_in_a_fresh_process():
    r = _child("gage_33", "env", {})
    st = r["stats"]
    assert r["n_diffs"] == 0 and st["mode"] == lib.L1_HITS_HOST and st["device_queries"] == 0, r
    assert st["host_queries"] == st["tail_queries"] == r["tail_calls"] > 0, r


def test_multi_context_of_two_on_one_gpu():
    m = gam.MultiContext([0, 0])
    m.set_l1_hits(lib.L1_HITS_DEVICE)
    try:
        n, diffs, n_tail, st, _ = H.run_groups(m, ["gage_33", "edges"], m.l1_hits_stats)
        per_ctx = m.l1_hits_stats()
    finally:
        m.close()
    assert n >= 130 and not diffs, diffs[:5]
    assert all(s["mode"] == lib.L1_HITS_DEVICE and s["device_queries"] > 0 and s["host_queries"] == 0 for s in per_ctx), per_ctx
    assert st["tail_queries"] == n_tail == st["device_queries"] + st["trivial_queries"] and st["host_fallback"] == 0, (st, n_tail)


# ---- mutation: a wrong seed is noticed -------------------------------------------------------------------------------------

def _needs_diag():
    if not os.path.exists(DIAG_LIB):
        pytest.skip("libgamdp_diag.so not built")


def test_dropped_hits_are_noticed_by_the_golden_comparison():
    """GAMDP_DIAG_HITS_DROP=1 on the diagnostics library: the comparison of test_golden_parity_with_device_hits reports differing
    cases.  It is the compared seeds that notice (gamdp_ctx_l1_tail_calls against the begin_a of the stored windows): 231 of the 694
    tail calls stored with their windows were seeded differently from the no-hits default, but by 148 bases at the most, inside the
    band of 150, and the reference's find_alignment returns the same result from either seed for every one of them -- outcome,
    n_dp, cells and the trail of results alone cannot tell a dropped seed from a right one on these merge blocks."""
    _needs_diag()
    r = _child(",".join(T.GROUPS), "setter", {"GAMDP_DIAG_HITS_DROP": "1"}, DIAG_LIB)
    assert r["diag"] and r["stats"]["device_queries"] > 1000, r
    assert r["n_diffs"] >= 1 and all("seeds" in d for d in r["diffs"]), r


def test_dropped_hits_are_noticed_on_a_case_whose_seed_matters():
    """tests/_l1hits.py seed_case(): the device path gives the oracle driver's answer; with every device query reporting no hits
    (diagnostics library) the same comparison reports the case"""
    _needs_diag()
    r = _child("seed-case", "setter", {}, DIAG_LIB)
    assert r["diag"] and r["stats"]["device_queries"] == 2 and r["n_diffs"] == 0 and r["tail_calls"] == 2, r
    r = _child("seed-case", "setter", {"GAMDP_DIAG_HITS_DROP": "1"}, DIAG_LIB)
    assert r["diag"] and r["stats"]["device_queries"] == 2 and r["n_diffs"] == 1, r
    assert "trail_crc" in r["diffs"][0], r


def test_the_product_library_ignores_the_drop_switch():
    r = _child("seed-case", "setter", {"GAMDP_DIAG_HITS_DROP": "1"})
    assert not r["diag"] and r["stats"]["device_queries"] == 2 and r["n_diffs"] == 0, r
    r = _child("gage_33,edges", "setter", {"GAMDP_DIAG_HITS_DROP": "1"})
    assert not r["diag"] and r["stats"]["device_queries"] > 50 and r["n_diffs"] == 0, r
