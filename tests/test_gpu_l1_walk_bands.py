"""GAMDP_L1_WALK_ANY_BAND: the main chains of gamdp_align_merge_blocks on k_chain2g<C> (gam_ngs_amd/csrc/gamdp_kernel.hip) --
k_chain2's workgroup (one filling and two walking wavefronts, scratch slots, twins) around the generic N-aware cell, at every band
up to 543 but 150, which keeps k_chain2.  Every comparison is check()'s of tests/test_gpu_l1_chain_carry.py, against the oracle's
restatement of PctgBuilder::alignMergeBlock: status, align_ok, coords_set, n_dp, cells, the coordinates and every record of the
audit trail.  gamdp_ctx_l1_chain_stats says which kernel ran and how many chains it took."""
import functools
import os
import random
import subprocess
import sys

import pytest

import _cases
import _l1cases
import _oracle as O
import gam_ngs_amd as gam
from gam_ngs_amd import lib
from test_gpu_l1_chain_carry import (BAND_SEED, _empty_frame_scenarios, _oracle, _stopping_scenarios, chained, check, make_mbs, outcome,
                                     run, score_cols, small_shapes)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SWITCHES = ("GAMDP_L1_CHAIN_CARRY", "GAMDP_L1_WALK_ANY_BAND", "GAMDP_L1_COHORTS", "GAMDP_L1_COHORT_MIN", "GAMDP_L1_ROUNDS",
            "GAMDP_L1_NO_TWINS", "GAMDP_LIB", "GAMDP_DIAG_CHAIN_SKEW")


@functools.lru_cache(maxsize=1)
def any_ctx():
    c = gam.Context(0)
    c.set_l1_walk_bands(lib.L1_WALK_ANY_BAND)
    return c


def gen_kernel(band):
    return "k_chain2g<%d>" % score_cols(band)


def assert_generic_launch(st, band):
    assert st["mode"] == lib.L1_CHAIN_WALK and st["kernel"] == gen_kernel(band) and st["cols"] == score_cols(band), st
    assert st["scratch_bytes"] > 0 and st["launches"] >= 1, st


# ---- 1. one band per instantiation and at each edge between two -----------------------------------------------------------------

@pytest.mark.parametrize("band", sorted(BAND_SEED))
def test_every_instantiation_and_edge(band):
    c = any_ctx()
    scs = _l1cases.scenarios(BAND_SEED[band], 20)
    stats = check(c, scs, band)
    assert stats["ok"] - stats["rev"] >= 1 and stats["rev"] >= 1 and stats["bad"] >= 1, stats
    st = c.l1_chain_stats()
    assert_generic_launch(st, band)
    assert st["chains"] == chained(scs) > 0 and st["round_loop_mbs"] == 0, st


# ---- 2. band 150 keeps k_chain2 -------------------------------------------------------------------------------------------------

def test_band_150_keeps_k_chain2_with_the_property_set():
    scs = _l1cases.scenarios(500, 60)
    c = any_ctx()
    check(c, scs, 150)
    st = c.l1_chain_stats()
    assert st["mode"] == lib.L1_CHAIN_WALK and st["kernel"].startswith("k_chain2<") and st["cols"] == 5, st
    assert st["chains"] == chained(scs) == 60, st
    with_property = [outcome(mb) for mb in run(c, scs, 150)]
    plain = gam.Context(0)
    try:
        without = [outcome(mb) for mb in run(plain, scs, 150)]
        st0 = plain.l1_chain_stats()
    finally:
        plain.close()
    assert with_property == without
    assert st0["kernel"] == st["kernel"] and st0["chains"] == st["chains"] and st0["chain_calls"] == st["chain_calls"], (st0, st)


# ---- 3. above GAMDP_MAX_TUNED_BAND ------------------------------------------------------------------------------------------------

def test_band_544_keeps_the_round_loop():
    c = any_ctx()
    rng = random.Random(544)
    scs = [_l1cases.scenario(rng, kind) for kind in ("tiny", "overlap", "overlap_rev", "bad", "wrong_vote")]
    check(c, scs, 544)
    st = c.l1_chain_stats()
    assert st["mode"] == lib.L1_CHAIN_WALK and st["chains"] == 0 and st["launches"] == 0 and st["kernel"] == "", st
    assert st["round_loop_mbs"] == len(scs) and st["cols"] == 0, st


# ---- 4. the smallest shapes -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("band", [5, 100, 200])
def test_smallest_shapes(band):
    c = any_ctx()
    scs = small_shapes(41)
    stats = check(c, scs, band)
    assert stats["ok"] >= 10 and stats["rev"] >= 3, stats
    st = c.l1_chain_stats()
    assert_generic_launch(st, band)
    assert st["chains"] == chained(scs) == len(scs), st


# ---- 5. chains that stop --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("band", [5, 200])
def test_chains_that_stop(band):
    scs = _stopping_scenarios()
    o = [_oracle(sc, band)[0] for sc in scs]
    # (what the scenarios are for, on the oracle alone)
    if band == 5:
        assert o[0].status == O.OUT_OF_RANGE
    assert o[1].status == O.OUT_OF_RANGE and o[1].n_dp == 2 and o[3].status == O.OUT_OF_RANGE and o[3].n_dp == 2
    assert o[4].status == O.INVALID and o[4].n_dp == 2 and o[2].align_ok
    c = any_ctx()
    stats = check(c, scs, band)
    assert stats["thrown"] >= 2
    st = c.l1_chain_stats()
    assert_generic_launch(st, band)
    assert st["chains"] == len(scs), st


# ---- 6. N -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("band", [64, 200])
def test_one_n_around_every_edge_of_a_calls_window(band):
    """tests/_cases.py n_edge_cases(band) as merge blocks of ONE block whose frames are the call's windows"""
    scs = [dict(kind="n-edge %s" % (tag,), master=a.decode(), slave=b.decode(), blocks=[(ba, ea, bb, eb, "+", "+", 10)], tails=(True, True, True, True))
           for a, b, ba, ea, bb, eb, tag in _cases.n_edge_cases(band)]
    c = any_ctx()
    stats = check(c, scs, band)
    assert len(scs) >= 50 and stats["ok"] >= 1 and stats["thrown"] == 0, stats
    st = c.l1_chain_stats()
    assert_generic_launch(st, band)
    assert st["chains"] == len(scs), st


# ---- 7. twins -------------------------------------------------------------------------------------------------------------------
TWIN_SEED = 502   # chosen on the CPU oracle alone (the assertions below, before the GPU is touched)


def _twin_candidates(scs):
    """select_chains (gamdp_l1.cpp) restated: the chains by decreasing rows; those of at least 1 024 rows and an eighth of the longest,
    from the front of that list, get a twin workgroup"""
    rows = sorted(((sum(b[3] - b[2] + 1 for b in sc["blocks"]), -i) for i, sc in enumerate(scs)), reverse=True)
    tw = []
    for r, neg_i in rows:
        if r * 8 >= rows[0][0] and r >= 1024:
            tw.append(-neg_i)
        else:
            break
    return tw


@pytest.mark.parametrize("band", [100, 200])   # (200: C = 9, twins whose walkers re-create strips, cancelled ones among them)
def test_twins_run_the_second_orientation(band):
    scs = _l1cases.scenarios(TWIN_SEED, 60)
    tw = _twin_candidates(scs)
    assert len(tw) >= 4, tw
    # good only in the second orientation: the first attempt made all its calls and failed, the second is good -- the main chain's calls
    # are twice the blocks (the oracle's n_dp counts the tails on top of them)
    second = [i for i in tw if _oracle(scs[i], band)[0].align_ok and _oracle(scs[i], band)[0].n_dp >= 2 * len(scs[i]["blocks"])]
    first = [i for i in tw if _oracle(scs[i], band)[0].align_ok and i not in second]
    failed = [i for i in tw if not _oracle(scs[i], band)[0].align_ok]
    assert second and first and failed, (second, first, failed)
    c = any_ctx()
    stats = check(c, scs, band)
    assert stats["ok"] >= 15 and stats["bad"] >= 5, stats
    st = c.l1_chain_stats()
    assert_generic_launch(st, band)
    assert st["twins"] == len(tw) > 0 and st["launches"] == 1 and st["chains"] == chained(scs) == 60, st


# ---- 8. a small arena -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("arena_kb", [6144, 700])
def test_a_small_arena(arena_kb):
    """half of the arena is the chain launch's: with 3 MB the slots of the 60 chains go in pieces, without twins; with 350 KB the
    longest chain's three slots do not fit and the call takes the round loop"""
    band = 100
    scs = _l1cases.scenarios(503, 60)
    c = gam.Context(0)
    c.set_l1_walk_bands(lib.L1_WALK_ANY_BAND)
    c.set_arena_bytes(arena_kb << 10)
    try:
        stats = check(c, scs, band)
        st = c.l1_chain_stats()
    finally:
        c.set_arena_bytes(0)
        c.close()
    assert stats["ok"] >= 15 and stats["bad"] >= 5, stats
    if st["launches"]:
        assert_generic_launch(st, band)
        assert st["launches"] > 1 and st["twins"] == 0 and st["chains"] == 60, st
        assert st["scratch_bytes"] <= (arena_kb << 10) // 2, st
    else:
        assert st["chains"] == 0 and st["kernel"] == "" and st["round_loop_mbs"] == 60, st


# ---- 9. empty slave frames ------------------------------------------------------------------------------------------------------

def test_empty_slave_frames_stay_with_the_round_loop_beside_chained_ones():
    band = 100
    c = any_ctx()
    scs = _l1cases.scenarios(611, 24)
    odd = _empty_frame_scenarios()
    mixed = scs[:12] + odd + scs[12:]
    stats = check(c, mixed, band)
    assert stats["ok"] >= 5
    st = c.l1_chain_stats()
    assert_generic_launch(st, band)
    assert st["chains"] == chained(mixed) == len(scs) and st["round_loop_mbs"] == len(odd), st
    check(c, odd, band)   # on their own: no chain launch at all
    st = c.l1_chain_stats()
    assert st["chains"] == 0 and st["launches"] == 0 and st["round_loop_mbs"] == len(odd), st


# ---- 10. the property of one context --------------------------------------------------------------------------------------------

def test_switching_the_property_on_one_context():
    band = 100
    scs = _l1cases.scenarios(502, 60)
    c = gam.Context(0)
    try:
        outs, sts = [], []
        for mode, which in ((lib.L1_CHAIN_WALK, lib.L1_WALK_BAND_150), (lib.L1_CHAIN_WALK, lib.L1_WALK_ANY_BAND),
                            (lib.L1_CHAIN_WALK, lib.L1_WALK_BAND_150), (lib.L1_CHAIN_CARRY, lib.L1_WALK_ANY_BAND)):
            c.set_l1_chain(mode)
            c.set_l1_walk_bands(which)
            outs.append([outcome(mb) for mb in run(c, scs, band)])
            sts.append(c.l1_chain_stats())
    finally:
        c.close()
    assert outs[0] == outs[1] == outs[2] == outs[3]
    for st in (sts[0], sts[2]):   # the round loop
        assert st["mode"] == lib.L1_CHAIN_WALK and st["kernel"] == "" and st["chains"] == 0 and st["launches"] == 0, st
        assert st["round_loop_mbs"] == 60 and st["scratch_bytes"] == 0, st
    assert_generic_launch(sts[1], band)
    assert sts[1]["kernel"] == "k_chain2g<5>" and sts[1]["chains"] == 60 and sts[1]["round_loop_mbs"] == 0, sts[1]
    assert sts[3]["mode"] == lib.L1_CHAIN_CARRY and sts[3]["kernel"] == "k_chain_c<5>" and sts[3]["scratch_bytes"] == 0, sts[3]
    assert sts[3]["chains"] == 60 and sts[3]["chain_calls"] == sts[1]["chain_calls"], sts


# ---- 11. several contexts -------------------------------------------------------------------------------------------------------

def test_multi_context_of_two_on_one_gpu():
    band = 100
    scs = _l1cases.scenarios(501, 60)
    m = gam.MultiContext([0, 0])
    try:
        m.set_l1_walk_bands(lib.L1_WALK_ANY_BAND)
        masters = gam.MultiSequenceSet(m, [sc["master"].encode() for sc in scs])
        slaves = gam.MultiSequenceSet(m, [sc["slave"].encode() for sc in scs])
        mbs = make_mbs(scs)
        gam.PctgBuilder(m, masters, slaves, band=band).alignMergeBlocks(mbs, audit=16)
        per_ctx = m.l1_chain_stats()
    finally:
        m.close()
    for sc, mb in zip(scs, mbs):
        o, oaud = _oracle(sc, band)
        assert (mb.status, mb.align_ok, mb.coords_set, mb.n_dp, mb.cells) == (o.status, bool(o.align_ok), bool(o.touched), o.n_dp, o.cells), sc["kind"]
        if o.touched:
            assert (mb.align_rev, mb.m_start, mb.m_end, mb.s_start, mb.s_end) == (bool(o.align_rev), o.m_start, o.m_end, o.s_start, o.s_end)
        assert [a.key() for a in mb.audit] == oaud, sc["kind"]
    assert all(s["mode"] == lib.L1_CHAIN_WALK and s["kernel"] == "k_chain2g<5>" and s["chains"] > 0 for s in per_ctx), per_ctx
    assert sum(s["chains"] for s in per_ctx) == 60, per_ctx


# ---- 12. fresh processes (the switches are read once per process) ---------------------------------------------------------------

def _child(code, env):
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-2500:]
    return r.stdout


def test_the_environment_switch_sets_the_property_of_new_contexts():
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import _l1cases, gam_ngs_amd as gam, test_gpu_l1_chain_carry as T\n"
            "c = gam.Context(0); T.run(c, _l1cases.scenarios(12, 8), 100)\n"
            "print('KERNEL', repr(c.l1_chain_stats()['kernel']))\n") % (os.path.dirname(HERE), HERE)
    for value, kernel in (("1", "k_chain2g<5>"), (None, "")):
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        if value:
            env["GAMDP_L1_WALK_ANY_BAND"] = value
        assert _child(code, env).strip().splitlines()[-1] == "KERNEL %r" % kernel


def test_band_96_with_three_cohorts_in_a_fresh_process():
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import _l1cases, gam_ngs_amd as gam, test_gpu_l1_chain_carry as T\n"
            "c = gam.Context(0); scs = _l1cases.scenarios(T.BAND_SEED[96], 20)\n"
            "stats = T.check(c, scs, 96); st = c.l1_chain_stats()\n"
            "assert stats['ok'] - stats['rev'] >= 1 and stats['rev'] >= 1 and stats['bad'] >= 1, stats\n"
            "assert st['kernel'] == 'k_chain2g<5>' and st['chains'] == T.chained(scs) > 0 and st['round_loop_mbs'] == 0, st\n"
            "print('CHAINS', st['chains'])\n") % (os.path.dirname(HERE), HERE)
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(GAMDP_L1_WALK_ANY_BAND="1", GAMDP_L1_COHORTS="3", GAMDP_L1_COHORT_MIN="8")
    assert _child(code, env).strip().splitlines()[-1].startswith("CHAINS ")


# ---- 13. the replay guards the new kernel ---------------------------------------------------------------------------------------

def test_a_skewed_device_window_is_noticed():
    """Fault injection (diagnostics build, GAMDP_DIAG_CHAIN_SKEW=1): k_chain2g<5> starts call 1 of every first attempt one slave base
    late.  The record it leaves is a plausible alignment; the host's replay derives the window itself and the call must fail with
    GAMDP_EHIP naming the merge block and begin_b.  The error is returned by the host: nothing on the device misbehaves."""
    from test_gpu_l0_parity import DIAG_LIB
    if not os.path.exists(DIAG_LIB):
        pytest.skip("libgamdp_diag.so not built")
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import _l1cases, gam_ngs_amd as gam, test_gpu_l1_chain_carry as T\n"
            "from gam_ngs_amd import lib as L\n"
            "c = gam.Context(0)\n"
            "try:\n"
            "    T.run(c, _l1cases.scenarios(503, 20), 100)\n"
            "    print('NO ERROR', c.l1_chain_stats()['kernel'])\n"
            "except L.GamdpError as e:\n"
            "    print('ERROR:', e)\n") % (os.path.dirname(HERE), HERE)
    base = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env = dict(base, GAMDP_LIB=DIAG_LIB, GAMDP_L1_WALK_ANY_BAND="1", GAMDP_DIAG_CHAIN_SKEW="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert "ERROR:" in r.stdout and "code %d" % lib.EHIP in r.stdout, r.stdout[-2000:] + r.stderr[-1500:]
    assert "merge block" in r.stdout and "begin_b" in r.stdout, r.stdout[-2000:]
    env = dict(base, GAMDP_LIB=DIAG_LIB, GAMDP_L1_WALK_ANY_BAND="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert "NO ERROR k_chain2g<5>" in r.stdout, r.stdout[-2000:] + r.stderr[-1500:]
