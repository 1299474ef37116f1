"""The device merge-block path (gamdp_align_merge_blocks through gam.PctgBuilder.alignMergeBlocks) against the
reference's own PctgBuilder::alignMergeBlock directly, not through the oracle: every merge block stored in
tests/golden/l1_vs_ref.json.gz (seeded, GAGE-shaped and hand-built edge cases) must give the reference's outcome,
coordinates, number of DP calls, cells and DP trail (CRC32, and call by call where the whole trail is stored).

Four ways through a call: the default device chains (k_chain2), the round loop (GAMDP_L1_ROUNDS=1) and one orientation
after the other (GAMDP_L1_NO_TWINS=1) in fresh child processes -- the switches are read once per process -- and a
700 KB scratch arena, with which the longest chains do not fit and the call falls back to the round loop (all groups
but three, which hold a call that alone needs more scratch than that)."""
import os
import subprocess
import sys

import pytest

import _l1ref as R
import test_l1_oracle_vs_ref as T
import gam_ngs_amd as gam

pytestmark = pytest.mark.gpu

SWITCHES = ("GAMDP_L1_ROUNDS", "GAMDP_L1_NO_TWINS")
TOO_LONG_FOR_700KB = ("seeded_7108", "gage_31", "gage_33")


def device_answers(c, cases):
    masters = gam.SequenceSet(c, [sc["master"].encode() for sc in cases])
    slaves = gam.SequenceSet(c, [sc["slave"].encode() for sc in cases])
    mbs = [gam.MergeBlock(i, i, [gam.Block(*b) for b in sc["blocks"]], *sc["tails"]) for i, sc in enumerate(cases)]
    gam.PctgBuilder(c, masters, slaves).alignMergeBlocks(mbs, audit=T.AUDIT_CAP)
    out = []
    for mb in mbs:
        keys = [a.key() for a in mb.audit]
        assert mb.n_dp <= T.AUDIT_CAP
        out.append((dict(thrown=mb.status == 2, align_ok=bool(mb.align_ok), coords_set=bool(mb.coords_set),
                         align_rev=bool(mb.align_rev) if mb.coords_set else False, m_start=mb.m_start, m_end=mb.m_end,
                         s_start=mb.s_start, s_end=mb.s_end, n_dp=mb.n_dp, cells=mb.cells, trail_crc=R.trail_crc(keys)),
                    keys))
    masters.close()
    slaves.close()
    return out


def check_all(c, groups=None):
    n = 0
    for group in groups or T.GROUPS:
        cases = T.GROUPS[group]()
        answers = T.stored(group, cases)
        keep = [k for k, a in enumerate(answers) if a is not None]
        got = device_answers(c, [cases[k] for k in keep])
        for k, (g, keys) in zip(keep, got):
            d = T.differences(g, answers[k], keys)
            assert not d, "%s %s #%d: %s differ(s): device %s, reference %s" % (
                group, cases[k]["kind"], k, d, {x: g[x] for x in d if x in g}, {x: answers[k][x] for x in d if x in answers[k]})
            n += 1
    return n


def test_device_chains_match_the_reference():
    from _gpu import ctx
    assert check_all(ctx()) >= 1700


def test_round_loop_fallback_of_a_small_arena_matches_the_reference():
    """700 KB: the longest chains do not fit and fall back to the round loop.  Three groups hold a merge block one of whose
    DP calls alone needs more scratch than that, which the call refuses loudly ("scratch arena too small for one task")
    rather than answering: they are left out here (they run on the other three paths)"""
    c = gam.Context(0)
    c.set_arena_bytes(700 << 10)
    try:
        assert check_all(c, [g for g in T.GROUPS if g not in TOO_LONG_FOR_700KB]) >= 1500
    finally:
        c.set_arena_bytes(0)


@pytest.mark.parametrize("switch", SWITCHES)
def test_other_ways_through_a_call_match_the_reference_in_a_fresh_process(switch):
    if any(os.environ.get(s) for s in SWITCHES):
        pytest.skip("already inside the child")
    env = dict(os.environ, **{switch: "1"})
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__),
                        "-k", "device_chains_match_the_reference"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-2500:] + r.stderr[-2000:]
