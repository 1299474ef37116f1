"""The shapes of what the library launches, pinned to recorded values (tests/golden/launch_shapes.json): which kernel a call takes, its
column count, how many launches, slots, twins and bytes of scratch.  All of it is host arithmetic -- the band rule, the layout of a
scratch slot, the launch planner, the merge-block driver's slot plan and its choice of chain kernel -- and all of it is exact integers
and strings that do not depend on the chip's CU count at these sizes.  The results themselves are the other tests' business.

  merge-block calls   a dozen of the smallest merge blocks (small_shapes of test_gpu_l1_chain_carry.py, chains of 1 to 4000 rows: some
                      get a twin) at bands 31 .. 543, in the default mode (k_chain2 at band 150, else the round loop), with
                      GAMDP_L1_WALK_ANY_BAND (k_chain2g<C>) and in GAMDP_L1_CHAIN_CARRY (k_chain_c<C>), each with the automatic
                      arena and with one small enough for the chain slots to go in pieces: gamdp_ctx_l1_chain_stats
  batch calls         12 calls of 300 to 3000 rows per band under a small arena (the planner peels launches off): gamdp_ctx_launch_info
  fill-only calls     the same calls at bands 31, 100 and 300 in one batch: gamdp_ctx_score_info / gamdp_ctx_carry_info

The recorded values come from the library as it was before the slot layout and the kernel tables were stated once (band_cols,
slot_geom, KernelFamily, ChainKernel in gamdp_dev.h):  GAMDP_LIB=<that build's libgamdp.so> python tests/test_gpu_launch_shapes.py --record
"""
import functools
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(HERE), HERE]

import pytest

import _cases
import gam_ngs_amd as gam
from gam_ngs_amd import lib
from test_gpu_l1_chain_carry import run, small_shapes

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden", "launch_shapes.json")
L1_BANDS = (31, 64, 100, 150, 160, 300, 543)
L1_MODES = {"walk": (lib.L1_CHAIN_WALK, lib.L1_WALK_BAND_150), "walk_any_band": (lib.L1_CHAIN_WALK, lib.L1_WALK_ANY_BAND),
            "carry": (lib.L1_CHAIN_CARRY, lib.L1_WALK_BAND_150)}
L1_FIELDS = ("kernel", "cols", "scratch_bytes", "launches", "twins", "chains", "chain_calls", "round_loop_mbs")


def l1_small_arena(band):
    """half of it is the chain launch's: room for the longest chain's three slots, not for all chains at once (a direction per cell
    up to 5 columns per lane; checkpoint and boundary stores on top from 9)"""
    return (3 << 20) if band < 160 else (24 << 20)


BATCH_ARENA = {100: 1 << 20, 150: 1 << 20, 300: 4 << 20, 512: 6 << 20, 600: 32 << 20}   # a few slots of the longest task each
FILL_BANDS = (31, 100, 300)


def merge_blocks():
    """12 of the 60 smallest shapes: 1, 2 and 9 blocks, either order, either strand; those of 9 blocks have a chain of 1024 rows or more"""
    scs = small_shapes(41)[::5]
    assert len(scs) == 12 and sum(1 for sc in scs if sum(b[3] - b[2] + 1 for b in sc["blocks"]) >= 1024) >= 1
    return scs


def batch_calls(ctx):
    """12 pairs of 300 to 3000 bases, three of them with N; every call takes the whole pair"""
    rng = random.Random(77)
    lens = [300 + (2700 * k) // 11 for k in range(12)]
    seqs = []
    for k, n in enumerate(lens):
        a, b = _cases.related_pair(rng, n, n_frac=0.01 if k % 4 == 1 else 0.0)
        seqs += [a.encode(), b.encode()]
    sset = gam.SequenceSet(ctx, seqs)
    return [(sset.contig(2 * k), 0, len(seqs[2 * k]) - 1, sset.contig(2 * k + 1), 0, len(seqs[2 * k + 1]) - 1) for k in range(12)]


@functools.lru_cache(maxsize=1)
def measure():
    """every shape, once: JSON-ready (lists and dicts of integers and strings)"""
    out = {"merge_blocks": {}, "batch": {}, "score": [], "carry": []}
    scs = merge_blocks()
    for mode, (chain, walk_bands) in L1_MODES.items():
        c = gam.Context(0)
        try:
            c.set_l1_chain(chain)
            c.set_l1_walk_bands(walk_bands)
            for band in L1_BANDS:
                for arena in (0, l1_small_arena(band)):
                    c.set_arena_bytes(arena)
                    run(c, scs, band)
                    st = c.l1_chain_stats()
                    out["merge_blocks"]["%s band %d arena %d" % (mode, band, arena)] = {k: st[k] for k in L1_FIELDS}
            c.set_arena_bytes(0)
        finally:
            c.close()
    c = gam.Context(0)
    try:
        calls = batch_calls(c)
        for band, arena in sorted(BATCH_ARENA.items()):
            c.set_arena_bytes(arena)
            gam.BandedSmithWaterman(c, band).find_alignments(calls)
            out["batch"]["band %d arena %d" % (band, arena)] = [[li["kernel"], li["tasks"], li["units"], li["slots"], li["band_max"]] for li in c.launch_info()]
        c.set_arena_bytes(0)
        fill_calls = [cl for _ in FILL_BANDS for cl in calls]
        fill_bands = [band for band in FILL_BANDS for _ in calls]
        bsw = gam.BandedSmithWaterman(c)
        bsw.find_scores(fill_calls, bands=fill_bands)
        out["score"] = [[li["kernel"], li["cols"], li["tasks"], li["slots"], li["band_max"]] for li in c.score_info()]
        bsw.find_results(fill_calls, bands=fill_bands)
        out["carry"] = [[li["kernel"], li["cols"], li["tasks"], li["slots"], li["band_max"]] for li in c.carry_info()]
    finally:
        c.close()
    return out


@functools.lru_cache(maxsize=1)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_merge_block_calls_launch_what_was_recorded():
    got, want = measure()["merge_blocks"], golden()["merge_blocks"]
    assert sorted(got) == sorted(want) and len(got) == len(L1_MODES) * len(L1_BANDS) * 2
    for key in sorted(want):
        print(key, got[key])
        assert got[key] == want[key], key
    # (what the cases are there for: every chain kernel family, twins, pieces, the round loop)
    kernels = {v["kernel"] for v in want.values()}
    assert {"", "k_chain2<false>", "k_chain_c<2>", "k_chain_c<17>", "k_chain2g<2>", "k_chain2g<9>", "k_chain2g<17>"} <= kernels, kernels
    assert any(v["twins"] > 0 for v in want.values()) and any(v["launches"] > 1 for v in want.values())


def test_batch_calls_launch_what_was_recorded():
    got, want = measure()["batch"], golden()["batch"]
    assert sorted(got) == sorted(want) and len(got) == len(BATCH_ARENA)
    for key in sorted(want):
        print(key, got[key])
        assert got[key] == want[key], key
    assert any(len(v) > 1 for v in want.values())   # (the planner peeled a launch off)


def test_fill_only_calls_launch_what_was_recorded():
    for which in ("score", "carry"):
        got, want = measure()[which], golden()[which]
        print(which, got)
        assert got == want, which
        assert [row[1] for row in want] == [2, 5, 17] and [row[4] for row in want] == list(FILL_BANDS), want


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: GAMDP_LIB=<the library to record from> python tests/test_gpu_launch_shapes.py --record")
    with open(GOLDEN, "w") as f:
        json.dump(measure(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded", GOLDEN, "from", lib.library_path())
