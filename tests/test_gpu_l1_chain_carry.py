"""GAMDP_L1_CHAIN_CARRY: the main chains of gamdp_align_merge_blocks on k_chain_c (gam_ngs_amd/csrc/gamdp_chain_carry.hip), one
wavefront per merge block on the carry cell -- no walk, no scratch slot, any band up to 543.  Every comparison is against the oracle's
restatement of PctgBuilder::alignMergeBlock exactly as tests/test_gpu_l1_parity.py compares: status, align_ok, coords_set, n_dp,
cells, the coordinates and every record of the audit trail.  gamdp_ctx_l1_chain_stats says which kernel ran and how many chains
it took."""
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
from _l1oracle import oracle_mb

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SWITCHES = ("GAMDP_L1_CHAIN_CARRY", "GAMDP_L1_COHORTS", "GAMDP_L1_COHORT_MIN", "GAMDP_L1_ROUNDS", "GAMDP_L1_NO_TWINS", "GAMDP_LIB",
            "GAMDP_DIAG_CHAIN_SKEW")


@functools.lru_cache(maxsize=1)
def carry_ctx():
    c = gam.Context(0)
    c.set_l1_chain(lib.L1_CHAIN_CARRY)
    return c


def make_mbs(scs):
    return [gam.MergeBlock(i, i, [gam.Block(*b) for b in sc["blocks"]], *sc["tails"]) for i, sc in enumerate(scs)]


@functools.lru_cache(maxsize=None)
def _oracle_of(key, band):
    """the oracle's answer for a scenario, computed once per (scenario, band) and shared by the tests"""
    return oracle_mb(_SCENARIOS[key], band=band)


_SCENARIOS = {}


def _oracle(sc, band):
    key = (sc["master"], sc["slave"], tuple(sc["blocks"]), tuple(sc["tails"]))
    _SCENARIOS.setdefault(key, sc)
    return _oracle_of(key, band)


def run(c, scs, band=150):
    masters = gam.SequenceSet(c, [sc["master"].encode() for sc in scs])
    slaves = gam.SequenceSet(c, [sc["slave"].encode() for sc in scs])
    mbs = make_mbs(scs)
    gam.PctgBuilder(c, masters, slaves, band=band).alignMergeBlocks(mbs, audit=16)
    return mbs


def outcome(mb):
    return (mb.status, mb.align_ok, mb.coords_set, mb.n_dp, mb.cells,
            (mb.align_rev, mb.m_start, mb.m_end, mb.s_start, mb.s_end) if mb.coords_set else None, [a.key() for a in mb.audit])


def check(c, scs, band=150):
    mbs = run(c, scs, band)
    stats = {"ok": 0, "rev": 0, "bad": 0, "tails": 0, "thrown": 0}
    for sc, mb in zip(scs, mbs):
        o, oaud = _oracle(sc, band)
        got = (mb.status, mb.align_ok, mb.coords_set, mb.n_dp, mb.cells)
        want = (o.status, bool(o.align_ok), bool(o.touched), o.n_dp, o.cells)
        assert got == want, (sc.get("kind"), band, got, want)
        if o.touched:
            assert (mb.align_rev, mb.m_start, mb.m_end, mb.s_start, mb.s_end) == \
                   (bool(o.align_rev), o.m_start, o.m_end, o.s_start, o.s_end), (sc.get("kind"), band)
        assert [a.key() for a in mb.audit] == oaud, (sc.get("kind"), band)
        stats["ok"] += mb.align_ok
        stats["rev"] += mb.align_ok and mb.align_rev
        stats["bad"] += not mb.align_ok
        stats["tails"] += mb.align_ok and mb.n_dp > len(sc["blocks"])
        stats["thrown"] += mb.status != O.OK
    return stats


def chained(scs):
    """merge blocks whose main chain goes to the device: those without an empty slave frame"""
    return sum(1 for sc in scs if all(b[3] >= b[2] for b in sc["blocks"]))


def score_cols(band):
    return next(c for c in (2, 3, 5, 9, 17) if 2 * band + 1 <= 64 * c)


# ---- band 150 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(4))
def test_band_150_matches_oracle(seed):
    c = carry_ctx()
    scs = _l1cases.scenarios(500 + seed, 60)
    stats = check(c, scs)
    assert stats["ok"] >= 15 and stats["rev"] >= 3 and stats["bad"] >= 5 and stats["tails"] >= 5, stats
    st = c.l1_chain_stats()
    assert st["mode"] == lib.L1_CHAIN_CARRY and st["kernel"] == "k_chain_c<5>" and st["scratch_bytes"] == 0, st
    assert st["cols"] == 5 and st["launches"] == 1 and st["twins"] == 0, st
    assert st["chains"] == chained(scs) == 60 and st["round_loop_mbs"] == 0, st
    # every DP call of a main chain is a record the replay used: all calls but the tails'
    assert st["chain_calls"] >= sum(len(sc["blocks"]) for sc in scs), st


# ---- one band per instantiation and at each edge between two -------------------------------------------------------------------
# seeds chosen on the CPU oracle alone: each band has a good forward, a good reversed and a rejected merge block among its 20
BAND_SEED = {5: 706, 63: 763, 64: 764, 95: 795, 96: 796, 159: 860, 160: 860, 287: 987, 288: 988, 543: 1243}


@pytest.mark.parametrize("band", sorted(BAND_SEED))
def test_every_instantiation_and_edge(band):
    c = carry_ctx()
    scs = _l1cases.scenarios(BAND_SEED[band], 20)
    stats = check(c, scs, band)
    assert stats["ok"] - stats["rev"] >= 1 and stats["rev"] >= 1 and stats["bad"] >= 1, stats
    st = c.l1_chain_stats()
    assert st["mode"] == lib.L1_CHAIN_CARRY and st["cols"] == score_cols(band), st
    assert st["kernel"] == "k_chain_c<%d>" % score_cols(band) and st["scratch_bytes"] == 0, st
    assert st["chains"] == chained(scs) > 0 and st["round_loop_mbs"] == 0, st


def test_band_544_keeps_the_round_loop():
    """above GAMDP_MAX_TUNED_BAND there is no carry instantiation: no chain launch, every call through the round loop and k_align_w"""
    c = carry_ctx()
    rng = random.Random(544)
    scs = [_l1cases.scenario(rng, kind) for kind in ("tiny", "overlap", "overlap_rev", "bad", "wrong_vote")]
    check(c, scs, 544)
    st = c.l1_chain_stats()
    assert st["mode"] == lib.L1_CHAIN_CARRY and st["chains"] == 0 and st["launches"] == 0 and st["kernel"] == "", st
    assert st["round_loop_mbs"] == len(scs) and st["cols"] == 0, st


def test_a_small_arena_does_not_matter():
    """700 KB: k_chain2's slots for the longest chain do not fit and the call falls back to the round loop
    (test_gpu_l1_parity.py::test_merge_blocks_with_a_small_scratch_arena); k_chain_c has no slots"""
    scs = _l1cases.scenarios(503, 60)
    c = gam.Context(0)
    c.set_l1_chain(lib.L1_CHAIN_CARRY)
    stats = check(c, scs)
    full = c.l1_chain_stats()
    c.set_arena_bytes(700 << 10)
    try:
        stats = check(c, scs)
        st = c.l1_chain_stats()
    finally:
        c.set_arena_bytes(0)
        c.close()
    assert stats["ok"] >= 15 and stats["bad"] >= 5, stats
    assert st["chains"] == full["chains"] == 60 and st["scratch_bytes"] == 0 and st["chain_calls"] == full["chain_calls"], (st, full)


# ---- the smallest shapes -------------------------------------------------------------------------------------------------------
FRAME_LENS = (1, 2, 31, 32, 33, 63, 64, 65, 97)   # rows below the lane count, at and around the fast block's 32 row-times


def small_shapes(seed):
    """merge blocks of 1, 2 and 9 blocks, blocks in forward and in backward order, slave on either strand; the slave frames' lengths go
    round FRAME_LENS, one block of every merge block of 9 is a few thousand bases long"""
    rng = random.Random(seed)
    scs = []
    for nb in (1, 2, 9):
        for backward in (False, True):
            for rot in range(0, 9, 2):
                for rev in (False, True):
                    lens = [FRAME_LENS[(rot + k) % 9] for k in range(nb)]
                    if nb == 9 or rot == 4:
                        lens[rng.randrange(nb)] = rng.randint(2000, 4000)
                    gaps = [rng.randint(0, 40) for _ in range(nb)]
                    core = _cases.rand_seq(rng, sum(lens) + sum(gaps) + 20)
                    core_s = "".join(ch if rng.random() > 0.02 else rng.choice("ACGT") for ch in core)   # substitutions only: the frames correspond
                    mL, sL = _cases.rand_seq(rng, rng.randint(0, 300)), _cases.rand_seq(rng, rng.randint(0, 300))
                    master = mL + core + _cases.rand_seq(rng, rng.randint(0, 300))
                    slave = sL + core_s + _cases.rand_seq(rng, rng.randint(0, 300))
                    blocks, at = [], 5
                    for k in range(nb):
                        at += gaps[k]
                        blocks.append([len(mL) + at, len(mL) + at + lens[k] - 1, len(sL) + at, len(sL) + at + lens[k] - 1, "+", "+", rng.randint(5, 50)])
                        at += lens[k]
                    if rev:
                        slave = _l1cases.revcomp_str(slave)
                        for b in blocks:
                            b[2], b[3], b[5] = len(slave) - 1 - b[3], len(slave) - 1 - b[2], "-"
                    if backward:
                        blocks.reverse()
                    scs.append(dict(kind="small nb=%d backward=%d rot=%d rev=%d" % (nb, backward, rot, rev), master=master, slave=slave,
                                    blocks=[tuple(b) for b in blocks], tails=tuple(rng.random() < 0.6 for _ in range(4))))
    return scs


@pytest.mark.parametrize("band", [5, 150])
def test_smallest_shapes(band):
    c = carry_ctx()
    scs = small_shapes(41)
    stats = check(c, scs, band)
    assert stats["ok"] >= 10 and stats["rev"] >= 3, stats
    st = c.l1_chain_stats()
    assert st["chains"] == chained(scs) == len(scs) and st["cols"] == score_cols(band), st


def _n_edge_scenarios():
    """tests/_cases.py n_edge_cases as merge blocks of ONE block whose frames are the call's windows (as test_gpu_l1_parity.py builds them)"""
    return [dict(kind="n-edge %s" % (tag,), master=a.decode(), slave=b.decode(), blocks=[(ba, ea, bb, eb, "+", "+", 10)], tails=(True, True, True, True))
            for a, b, ba, ea, bb, eb, tag in _cases.n_edge_cases(150)]


def test_one_n_around_every_edge_of_a_calls_window():
    c = carry_ctx()
    scs = _n_edge_scenarios()
    stats = check(c, scs)
    assert stats["ok"] + stats["bad"] >= 50, stats
    assert c.l1_chain_stats()["chains"] == len(scs)


def _empty_frame_scenarios():
    """the empty-slave-frame merge blocks of test_gpu_l1_parity.py: they stay with the round loop"""
    rng = random.Random(31)
    odd = []
    for variant in range(6):
        core = _cases.rand_seq(rng, 2600)
        core_s = _cases.mutate(rng, core, 0.01, 0.003, 0.003)
        master = _cases.rand_seq(rng, rng.randint(0, 40)) + core + _cases.rand_seq(rng, 200)
        slave = core_s + _cases.rand_seq(rng, 150)
        off = len(master) - 200 - len(core)
        normal = (off + 300, off + 620, 290, 615, "+", "+", 20)
        normal2 = (off + 900, off + 1300, 890, 1290, "+", "+", 12)
        empty = (off + 10, off + 200, 0, -1, "+", "+", 7)
        empty_late = (off + 700, off + 800, 0, -1, "+", "+", 7)
        blocks = [[empty, normal, normal2], [normal, empty_late, normal2], [empty], [empty, normal], [normal, normal2, empty_late],
                  [(off + 10, off + 200, 5, 2, "+", "-", 9), normal]][variant]
        odd.append(dict(kind="empty_frame", master=master, slave=slave, blocks=blocks, tails=(True, True, True, True)))
    return odd


def test_empty_slave_frames_stay_with_the_round_loop_beside_chained_ones():
    c = carry_ctx()
    scs = _l1cases.scenarios(611, 24)
    odd = _empty_frame_scenarios()
    mixed = scs[:12] + odd + scs[12:]
    stats = check(c, mixed)
    assert stats["ok"] >= 5
    st = c.l1_chain_stats()
    assert st["chains"] == chained(mixed) == len(scs) and st["round_loop_mbs"] == len(odd), st
    check(c, odd)   # on their own: no chain launch at all
    st = c.l1_chain_stats()
    assert st["chains"] == 0 and st["launches"] == 0 and st["round_loop_mbs"] == len(odd), st


def _stopping_scenarios():
    """chains that stop: a DP call that ends outside the master (the reference throws: test_reference_exception_is_reported_per_merge_block),
    and second calls that the pre-checks settle -- the slave gap puts begin_b behind the slave, the master gap begin_a beyond |a| + band"""
    rng = random.Random(9)
    m0, s0 = _cases.rand_seq(rng, 300), _cases.rand_seq(rng, 300)
    thrown = dict(kind="thrown", master=m0, slave=s0, blocks=[(250, 400, 10, 160, "+", "+", 9)], tails=(True, True, True, True))
    core = _cases.rand_seq(rng, 900)
    behind_b = dict(kind="precheck-b", master=_cases.rand_seq(rng, 30) + core + _cases.rand_seq(rng, 100), slave=core + _cases.rand_seq(rng, 60),
                    blocks=[(130, 330, 100, 300, "+", "+", 9), (5030, 5300, 5000, 5270, "+", "+", 9), (5400, 5500, 5370, 5470, "+", "+", 9)],
                    tails=(True, True, True, True))
    behind_b_far = dict(behind_b, kind="precheck-b-invalid")   # ... and begin_a far beyond the master too: INVALID, not OUT_OF_RANGE
    behind_b = dict(behind_b, blocks=[behind_b["blocks"][0], (400, 600, 5000, 5270, "+", "+", 9), behind_b["blocks"][2]])
    beyond_a = dict(kind="precheck-a", master=_cases.rand_seq(rng, 30) + core, slave=core + _cases.rand_seq(rng, 600),
                    blocks=[(130, 330, 100, 300, "+", "+", 9), (2400, 2600, 400, 600, "+", "+", 9)], tails=(True, True, True, True))
    good = _l1cases.scenario(random.Random(4), "overlap")
    return [thrown, behind_b, good, beyond_a, behind_b_far]


@pytest.mark.parametrize("band", [5, 150])
def test_chains_that_stop(band):
    scs = _stopping_scenarios()
    o = [_oracle(sc, band)[0] for sc in scs]
    # (what the scenarios are for, on the oracle alone)
    if band == 5:
        assert o[0].status == O.OUT_OF_RANGE
    assert o[1].status == O.OUT_OF_RANGE and o[1].n_dp == 2 and o[3].status == O.OUT_OF_RANGE and o[3].n_dp == 2
    assert o[4].status == O.INVALID and o[4].n_dp == 2 and o[2].align_ok
    c = carry_ctx()
    stats = check(c, scs, band)
    assert stats["thrown"] >= 2
    assert c.l1_chain_stats()["chains"] == len(scs)


# ---- the mode is a property of the context -------------------------------------------------------------------------------------

def test_mode_switching_on_one_context():
    scs = _l1cases.scenarios(502, 60)
    c = gam.Context(0)
    try:
        outs, sts = [], []
        for mode in (lib.L1_CHAIN_WALK, lib.L1_CHAIN_CARRY, lib.L1_CHAIN_WALK):
            c.set_l1_chain(mode)
            outs.append([outcome(mb) for mb in run(c, scs)])
            sts.append(c.l1_chain_stats())
    finally:
        c.close()
    assert outs[0] == outs[1] == outs[2]
    for st in (sts[0], sts[2]):
        assert st["mode"] == lib.L1_CHAIN_WALK and st["kernel"].startswith("k_chain2<") and st["scratch_bytes"] > 0 and st["cols"] == 5, st
        assert st["chains"] == 60, st
    assert sts[1]["mode"] == lib.L1_CHAIN_CARRY and sts[1]["kernel"] == "k_chain_c<5>" and sts[1]["scratch_bytes"] == 0, sts[1]
    assert sts[1]["chains"] == 60 and sts[1]["chain_calls"] == sts[0]["chain_calls"] == sts[2]["chain_calls"], sts


def test_multi_context_of_two_on_one_gpu():
    scs = _l1cases.scenarios(501, 60)
    m = gam.MultiContext([0, 0])
    try:
        m.set_l1_chain(lib.L1_CHAIN_CARRY)
        masters = gam.MultiSequenceSet(m, [sc["master"].encode() for sc in scs])
        slaves = gam.MultiSequenceSet(m, [sc["slave"].encode() for sc in scs])
        mbs = make_mbs(scs)
        gam.PctgBuilder(m, masters, slaves).alignMergeBlocks(mbs, audit=16)
        per_ctx = m.l1_chain_stats()
    finally:
        m.close()
    for sc, mb in zip(scs, mbs):
        o, oaud = _oracle(sc, 150)
        assert (mb.status, mb.align_ok, mb.coords_set, mb.n_dp, mb.cells) == (o.status, bool(o.align_ok), bool(o.touched), o.n_dp, o.cells), sc["kind"]
        if o.touched:
            assert (mb.align_rev, mb.m_start, mb.m_end, mb.s_start, mb.s_end) == (bool(o.align_rev), o.m_start, o.m_end, o.s_start, o.s_end)
        assert [a.key() for a in mb.audit] == oaud, sc["kind"]
    assert all(s["mode"] == lib.L1_CHAIN_CARRY and s["kernel"] == "k_chain_c<5>" and s["chains"] > 0 for s in per_ctx), per_ctx
    assert sum(s["chains"] for s in per_ctx) == 60, per_ctx


# ---- other ways through a call, in fresh processes (the switches are read once per process) ------------------------------------

@pytest.mark.parametrize("extra", [{}, {"GAMDP_L1_COHORTS": "3", "GAMDP_L1_COHORT_MIN": "8"}], ids=["env-switch", "cohorts3"])
def test_the_parity_tests_in_a_fresh_process_with_the_environment_switch(extra):
    """GAMDP_L1_CHAIN_CARRY=1 makes CARRY the mode of every new context: the merge-block tests of test_gpu_l1_parity.py once more"""
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(extra, GAMDP_L1_CHAIN_CARRY="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.join(HERE, "test_gpu_l1_parity.py"),
                        "-k", "merge_blocks_match_oracle or single_merge_block or reference_exception or one_n_around_every_edge"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2500:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-1000:]


def test_the_environment_switch_sets_the_mode_of_new_contexts():
    """GAMDP_L1_CHAIN_CARRY=1 -> CARRY, unset -> WALK: the mode the first call of a fresh context reports"""
    for value, mode in (("1", lib.L1_CHAIN_CARRY), (None, lib.L1_CHAIN_WALK)):
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        if value:
            env["GAMDP_L1_CHAIN_CARRY"] = value
        assert _mode_of_a_first_call(env) == mode


def _mode_of_a_first_call(env):
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import _l1cases, gam_ngs_amd as gam, test_gpu_l1_chain_carry as T\n"
            "c = gam.Context(0); T.run(c, _l1cases.scenarios(12, 8))\n"
            "print('MODE', c.l1_chain_stats()['mode'])\n") % (os.path.dirname(HERE), HERE)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    return int(r.stdout.strip().splitlines()[-1].split()[1])


# ---- the replay still guards the new kernel ------------------------------------------------------------------------------------

def test_a_skewed_device_window_is_noticed():
    """Fault injection (diagnostics build, GAMDP_DIAG_CHAIN_SKEW=1): k_chain_c starts call 1 of every first attempt one slave base
    late.  The record it leaves is a plausible alignment; the host's replay derives the window itself and the call must fail with
    GAMDP_EHIP naming the merge block and begin_b.  The error is returned by the host: nothing faults."""
    from test_gpu_l0_parity import DIAG_LIB
    if not os.path.exists(DIAG_LIB):
        pytest.skip("libgamdp_diag.so not built")
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import _l1cases, gam_ngs_amd as gam, test_gpu_l1_chain_carry as T\n"
            "from gam_ngs_amd import lib as L\n"
            "c = gam.Context(0)\n"
            "try:\n"
            "    T.run(c, _l1cases.scenarios(503, 20))\n"
            "    print('NO ERROR', c.l1_chain_stats()['kernel'])\n"
            "except L.GamdpError as e:\n"
            "    print('ERROR:', e)\n") % (os.path.dirname(HERE), HERE)
    base = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env = dict(base, GAMDP_LIB=DIAG_LIB, GAMDP_L1_CHAIN_CARRY="1", GAMDP_DIAG_CHAIN_SKEW="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert "ERROR:" in r.stdout and "code %d" % lib.EHIP in r.stdout, r.stdout[-2000:] + r.stderr[-1500:]
    assert "merge block" in r.stdout and "begin_b" in r.stdout, r.stdout[-2000:]
    env = dict(base, GAMDP_LIB=DIAG_LIB, GAMDP_L1_CHAIN_CARRY="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert "NO ERROR k_chain_c<5>" in r.stdout, r.stdout[-2000:] + r.stderr[-1500:]
