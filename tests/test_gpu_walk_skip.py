"""GAMDP_WALK_SKIP_DIAG: the walks of the eight-task band-150 kernel (k_align_o<19,15>) jump over groups of 64 rows that provably hold
diagonal steps only (gam_ngs_amd/csrc/kernel_walk.inc, walk_many<..., SKIP>; gamdp_ctx_set_walk_skip).

Every case runs on ONE context with the property off and on: every field of every result equals the oracle's, and the two runs are
equal field by field (edit strings included where asked for).  What the walks did is read from gamdp_ctx_walk_skip_stats and
gamdp_ctx_launch_info.  The cases run in fresh child processes with GAMDP_QUAD_MIN=1 (a small batch reaches the eight-task kernel
only through that planner switch, read once per process), on the product library and on the diagnostics library
(libgamdp_diag.so, which also reports a packed value that left the exact f16 range).  Band 150, N-free pairs.

Sizes: the direction-free range of a call begins behind the ramp and the top blocks and ends with the last rows, in whole groups of
64 row-times; SHORT is the shortest length (a multiple of 16 bases, identical pair, whole sequences) at which the range holds at
least 3 groups -- found on the device by the child itself and asserted -- and the cases use SHORT, about twice SHORT and pairs of
3 - 6 kb."""
import os
import random

import pytest

import _cases
import _oracle as O
import _walkskip as W
import gam_ngs_amd as gam
from _walkskip import both, case, ctx, gap_free, one_indel, oracle_all, run, short_length, sizes, substituted
from gam_ngs_amd import lib as L

pytestmark = pytest.mark.gpu

FAMILY = "o19"           # of tests/_walkskip.py: every child of this file runs as that family (GAMDP_QUAD_MIN=1)
BAND, C = 150, 19
KERNEL = W.O19


# ---- in the child ------------------------------------------------------------------------------------------------------------------

def child_gap_free():
    """1. identical pairs and pairs with substitutions only: no strip at all with the property on"""
    rng = random.Random(1)
    # one call per length: the tasks of a wavefront then end together and the direction-free range reaches every task's end cell (a
    # task that outlasts the range of its wavefront enters it from tagged blocks, where no stored row tells H: one strip call)
    for n in sizes():
        a = _cases.rand_seq(rng, n)
        cases = [case(a, a), case(a, substituted(rng, a, 0.02))]
        want = oracle_all(cases)
        assert all(o.status == O.OK and gap_free(ops) and o.length >= n - 64 for o, ops in want)
        _, info0, info1, st0, st1 = both(cases, False, want)
        assert [r["units_dirfree"] for r in info1] == [1], info1
        assert sum(r["strips"] for r in info0) > 0, info0
        assert st1["strips"] == 0 and sum(r["strips"] for r in info1) == 0, (st1, info1)
        assert st1["groups_skipped"] > 0 and st1["groups_skipped"] == st1["groups_tested"], st1
        # every row of the direction-free range is jumped over: all rows but the ramp, the top blocks and a tagged block in front
        assert st1["rows_skipped"] >= 2 * (n - 400), (st1, n)
        both(cases, True, want)


def child_one_indel():
    """2. one 1-base insertion or deletion at row 64 g + d: a strip there, rows jumped over above and below"""
    rng = random.Random(2)
    n = 6000                           # 93 groups: a strip call serves 32 of them, so 50 and 70 have rows to jump over on either side
    cases, rows = [], []
    # d: around row 64 g, and around row-time 64 g of the lane the centred path runs in (lane 7 of 16: row-time = row + 7)
    for g in (50, 70):
        for d in (-2, -1, 0, 1, -10, -9, -8, -7):
            for kind in ("ins", "del"):
                cases.append(one_indel(rng, n, 64 * g + d, kind))
                rows.append(64 * g + d)
    want = oracle_all(cases)
    for (o, ops) in want:
        assert o.status == O.OK and sum(1 for ch in ops if ch in "AB") == 1, ops.count("A")
    # one call at a time: the statistics of a call are its own
    for cs, w, row in zip(cases, want, rows):
        _, info0, info1, st0, st1 = both([cs], False, [w])
        assert st1["strips"] >= 1 and st1["strips"] <= st0["strips"], (row, st0, st1)
        # rows above the indel, and rows below the 32 groups its strip call serves: more than either side alone has
        assert st1["tests"] >= 2 and st1["rows_skipped"] > max(n - row, row - 32 * 64) + 64, (row, st1)
    both(cases, True, want)


def child_periodic_indels():
    """3. an indel every ~200 rows: a passing prefix of groups followed by a failing one in the same test"""
    rng = random.Random(3)
    cases = []
    for n in sizes()[1:]:
        a = _cases.rand_seq(rng, n)
        b, at = [], 0
        while at < n:
            step = rng.randint(170, 230)
            seg = a[at:at + step]
            last = at + step >= n      # (the last stretch stays as it is: the span below the end cell passes)
            b.append(seg if last else (seg[:-1] if rng.random() < 0.5 else seg + rng.choice("ACGT")))
            at += step
        cases.append(case(a, "".join(b)))
    # one call each (a wavefront of one length, see child_gap_free): a strip call serves 32 groups, so the calls of 3 kb and more
    # test again below their first strip
    for cs in cases:
        _, info0, info1, st0, st1 = both([cs], False)
        assert st1["groups_skipped"] > 0 and st1["groups_tested"] > st1["groups_skipped"], st1
        assert 0 < st1["strips"] <= st0["strips"], (st0, st1)
        assert st1["tests"] >= (2 if len(cs["a"]) >= 3000 else 1), st1
    both(cases, True)


def child_tie_rich():
    """4. homopolymers, dinucleotide and tandem repeats: `up` / `left` tie with `diag` all along the path"""
    import _ties as TW
    cases = [cs for cs in TW.long_cases(BAND) if b"N" not in cs["a"] + cs["b"]]
    assert len(cases) >= 40 and {cs["tag"][0] for cs in cases} >= {"homopolymer", "ac_shift1", "tandem19", "complement"}
    want = TW.wants("long", BAND)
    want = [w for cs, w in zip(TW.long_cases(BAND), want) if b"N" not in cs["a"] + cs["b"]]
    _, info0, info1, st0, st1 = both(cases, False, want, only=False)
    assert sum(r["tasks"] for r in info1 if r["kernel"] == KERNEL) >= 40, info1
    assert st1["groups_skipped"] > 0 and st1["groups_tested"] > st1["groups_skipped"], st1
    both(cases, True, want, only=False)


def displaced(rng, y, n, begin_a, rate=0.02):
    """test_gpu_strip_widths.displaced() for band 150: an alignment that runs down band column y"""
    k = abs(y - BAND)
    if y >= BAND:
        a = _cases.rand_seq(rng, n + k)
        b = substituted(rng, a[k:], rate)
    else:
        a = _cases.rand_seq(rng, n - k)
        b = _cases.rand_seq(rng, k) + substituted(rng, a, rate)
    a = _cases.rand_seq(rng, begin_a) + a
    return case(a, b, begin_a=begin_a)


def child_displaced():
    """5. paths on the first and last column of a lane, in the first and last strip of the task, next to the band's edge columns"""
    rng = random.Random(5)
    s = short_length()
    ys = sorted({1, 2, 18, 19, 37, 38, 133, 151, 152, 170, 171, 266, 284, 285, 297, 298, 299})
    cases = []
    for i, y in enumerate(ys):
        cases.append(displaced(rng, y, 2 * s + 37 * (i % 5), 0))
        cases.append(displaced(rng, y, 3000 + 64 * (i % 3), 700, rate=0.0 if i % 2 else 0.02))
    want = oracle_all(cases)
    cols = set()
    for cs, (o, ops) in zip(cases, want):
        assert o.status == O.OK and o.length >= len(cs["b"]) - 300, (len(cs["a"]), len(cs["b"]), o.length)
        cols.add(o.begin_a - cs["begin_a"] - (o.begin_b - cs["begin_b"]) + BAND)
    assert min(cols) <= 3 and max(cols) >= 297 and len(cols) >= 12, sorted(cols)
    _, info0, info1, st0, st1 = both(cases, False, want)
    assert st1["groups_skipped"] > 10 * len(cases) and st1["strips"] < st0["strips"], (st0, st1)
    both(cases, True, want)


def child_clamps():
    """6. spans that would cross pos == 0, a b shorter than a span, force_start / force_end calls, suffix and reverse-complement views"""
    rng = random.Random(6)
    s = short_length()
    cases = []
    for k in (1, 63, 64, 65, 100, 149):           # b has k bases in front: the path reaches pos == 0 in row k, inside the top groups
        a = _cases.rand_seq(rng, 2 * s)
        cases.append(case(a, _cases.rand_seq(rng, k) + a))
        cases.append(case(a, _cases.rand_seq(rng, k) + a, begin_a=0, fs=True))
    for ba in (1, 2, 63, 64, 65, 127, 128, 129, 151, 300):   # the window begins ba bases into a
        a = _cases.rand_seq(rng, 2 * s + ba)
        cases.append(case(a, a[ba:], begin_a=ba))
        cases.append(case(a, a, begin_a=ba))
    for nb in (1, 40, 63, 64, 65, 130):           # b shorter than a span / than two
        a = _cases.rand_seq(rng, 3000)
        cases.append(case(a, a[:nb]))
    for fs, fe in ((True, False), (False, True), (True, True)):
        a = _cases.rand_seq(rng, 3 * s)
        b = substituted(rng, a, 0.01)
        cases.append(case(a, b, fs=fs, fe=fe))
        cases.append(case(a, b, begin_a=40, end_a=len(a) - 70, begin_b=35, end_b=len(b) - 90, fs=fs, fe=fe))
    _, info0, info1, st0, st1 = both(cases, False, only=False)
    assert st1["groups_skipped"] > 0, st1
    both(cases, True, only=False)
    # views: the o19 cell of tests/_views.py (all 16 view kinds, two 20 kb pairs), view call and copy call, both modes
    import _views as V
    import test_gpu_views as TV
    vcases = [cs for cs in V.matrix_cases() if cs["cell"] == "o19"]
    vwant = TV._oracle_all(vcases)
    c = ctx()
    seen = {}
    for mode in (L.WALK_STRIPS, L.WALK_SKIP_DIAG):
        c.set_walk_skip(mode)
        try:
            res = TV.run_view_and_copy(c, vcases, want_ops=False)
        finally:
            c.set_walk_skip(L.WALK_STRIPS)
        TV.compare(vcases, res, vwant, False, V.digest(vcases))
        seen[mode] = ([(rv.key(), rc_.key()) for rv, rc_ in res], c.walk_skip_stats())
    assert seen[0][0] == seen[1][0]
    assert seen[1][1]["groups_skipped"] > 0 and seen[0][1]["groups_skipped"] == 0, seen[1][1]
    print("  views: %s" % (seen[1][1],))


def child_mixed_units():
    """7. units of unequal lengths with padding copies, a unit in which some tasks want edit strings, a batch with N-holding calls"""
    rng = random.Random(7)
    s = short_length()
    cases = []
    # 11 calls: a unit of 5.2 - 6 kb and one of 0.5 - 1 kb with 5 padding copies (tasks that end within 64 blocks of each other: the
    # direction-free range then runs on behind the longest)
    for n in (s, s + 200, 2 * s, 5200, 5300, 5400, 5500, 5600, 5800, 6000, 5900):
        a = _cases.rand_seq(rng, n)
        cases.append(case(a, _cases.mutate(rng, a, 0.01, 0.001, 0.001)))
    _, info0, info1, st0, st1 = both(cases, False)
    assert sum(r["units"] for r in info1) == 2 and sum(r["tasks"] for r in info1) == 11, info1
    assert st1["groups_skipped"] > 0, st1
    # some tasks of a unit want their edit string: they keep the one-task walk, the others of the unit jump
    flags = [k % 3 == 0 for k in range(len(cases))]
    _, _, _, st0f, st1f = both(cases, flags)
    assert 0 < st1f["groups_skipped"] < st1["groups_skipped"], (st1f, st1)
    both(cases, True)
    # N-holding calls beside them (GAMDP_QUAD_MIN keeps the two launches apart): the N-aware launch is what it was, the statistics
    # are the eight-task launch's alone
    ncases = []
    for n in (2 * s, 3000, 4000):
        a = _cases.rand_seq(rng, n)
        b = list(_cases.mutate(rng, a, 0.01, 0.001, 0.001))
        b[len(b) // 2] = "N"
        ncases.append(case(a, "".join(b)))
    _, info0, info1, st0m, st1m = both(cases + ncases, False, only=False)
    for info in (info0, info1):
        assert sorted((r["n_aware"], r["tasks"]) for r in info) == [(0, len(cases)), (1, len(ncases))], info
        assert [r["kernel"] for r in info if not r["n_aware"]] == [KERNEL], info
    nstrips = [sum(r["strips"] for r in info if r["n_aware"]) for info in (info0, info1)]
    assert nstrips[0] == nstrips[1], nstrips
    assert (st1m["tests"], st1m["groups_tested"], st1m["groups_skipped"], st1m["rows_skipped"], st1m["strips"]) == \
           (st1["tests"], st1["groups_tested"], st1["groups_skipped"], st1["rows_skipped"], st1["strips"]), (st1m, st1)
    # a call without an eight-task launch: everything 0
    c = ctx()
    c.set_walk_skip(L.WALK_SKIP_DIAG)
    try:
        run(ncases, False)
        st = c.walk_skip_stats()
    finally:
        c.set_walk_skip(L.WALK_STRIPS)
    assert st == dict(tests=0, groups_tested=0, groups_skipped=0, rows_skipped=0, strips=0, mode=L.WALK_SKIP_DIAG), st


def child_defaults():
    """8. refusals, the statistics before any call, the environment default, two contexts of a multi handle in different modes"""
    import ctypes
    l = L.load_library()
    st = L.WalkSkipStats()
    assert l.gamdp_ctx_set_walk_skip(None, L.WALK_STRIPS) == L.EINVAL and l.gamdp_ctx_set_walk_skip(None, L.WALK_SKIP_DIAG) == L.EINVAL
    assert l.gamdp_ctx_walk_skip_stats(None, ctypes.byref(st)) == L.EINVAL
    c = gam.Context(0)
    assert l.gamdp_ctx_walk_skip_stats(c.handle, None) == L.EINVAL
    for mode in (-1, 2, 7, 1 << 20):
        assert l.gamdp_ctx_set_walk_skip(c.handle, mode) == L.EINVAL
        with pytest.raises(gam.GamdpError):
            c.set_walk_skip(mode)
    want_mode = L.WALK_SKIP_DIAG if os.environ.get("GAMDP_WALK_SKIP") == "1" else L.WALK_STRIPS
    assert c.walk_skip_stats() == dict(tests=0, groups_tested=0, groups_skipped=0, rows_skipped=0, strips=0, mode=0)
    # the mode of a fresh context: what its first call reports
    rng = random.Random(8)
    a = _cases.rand_seq(rng, 3000)
    cs = case(a, a)
    sset = gam.SequenceSet(c, [cs["a"], cs["b"]], ascii=True)
    call = [(sset.contig(0), 0, len(a) - 1, sset.contig(1), 0, len(a) - 1, False, False)]
    r = gam.BandedSmithWaterman(c).find_alignments(call, bands=[BAND])[0]
    st = c.walk_skip_stats()
    assert r.key() == oracle_all([cs])[0][0].key()
    assert st["mode"] == want_mode and (st["groups_skipped"] > 0) == (want_mode == L.WALK_SKIP_DIAG), st
    print("ENV_MODE %d" % st["mode"])
    sset.close()
    if os.environ.get("GAMDP_WALK_SKIP_TEST_ENV_ONLY"):
        return
    # gamdp_multi: two contexts on one device, one on and one off
    cases = []
    for n in (3000, 3300, 4000, 4800, 5200, 6000):
        x = _cases.rand_seq(rng, n)
        cases.append(case(x, _cases.mutate(rng, x, 0.01, 0.001, 0.001)))
    want = oracle_all(cases)
    seqs = []
    for k in cases:
        seqs += [k["a"], k["b"]]
    m = gam.MultiContext([0, 0])
    m.set_walk_skip(L.WALK_SKIP_DIAG, which=1)
    ms = gam.MultiSequenceSet(m, seqs, ascii=True)
    calls = [(ms.contig(2 * i), k["begin_a"], k["end_a"], ms.contig(2 * i + 1), k["begin_b"], k["end_b"], False, False) for i, k in enumerate(cases)]
    res = gam.BandedSmithWaterman(m).find_alignments(calls, bands=[BAND] * len(cases))
    sts = m.walk_skip_stats()
    ms.close()
    m.close()
    for r, (o, _) in zip(res, want):
        assert r.key() == o.key()
    assert [s["mode"] for s in sts] == [L.WALK_STRIPS, L.WALK_SKIP_DIAG], sts
    assert sts[0]["groups_skipped"] == 0 and sts[1]["groups_skipped"] > 0 and sts[0]["strips"] > 0, sts


def child_merge_blocks():
    """9. gamdp_align_merge_blocks on tests/_l1cases.py scenarios: gamdp_mb_out and the audit do not depend on the property"""
    import _l1cases
    import test_gpu_l1_chain_carry as T
    c = ctx()
    scs = _l1cases.scenarios(900, 48)
    outs = {}
    for mode in (L.WALK_STRIPS, L.WALK_SKIP_DIAG):
        c.set_walk_skip(mode)
        try:
            stats = T.check(c, scs)          # against the oracle's driver, audit included
            outs[mode] = [T.outcome(mb) for mb in T.run(c, scs)]
        finally:
            c.set_walk_skip(L.WALK_STRIPS)
        assert stats["ok"] >= 10, stats
    assert outs[0] == outs[1]


CHILDREN = {f.__name__[len("child_"):]: f for f in (child_gap_free, child_one_indel, child_periodic_indels, child_tie_rich, child_displaced,
                                                    child_clamps, child_mixed_units, child_defaults, child_merge_blocks)}


# ---- the tests: one fresh child each (never exec) --------------------------------------------------------------------------------

def run_child(name, diag=False, extra=None):
    return W.run_child("test_gpu_walk_skip", name, FAMILY, diag, extra)


LIBS = pytest.mark.parametrize("diag", (False, True), ids=("product", "diag"))


@LIBS
def test_gap_free_pairs_need_no_strip(diag):
    """Fails without the feature: with the property on not one strip is re-created for pairs whose alignment holds no gap."""
    run_child("gap_free", diag)


@LIBS
def test_one_indel_around_a_group_boundary(diag):
    run_child("one_indel", diag)


@LIBS
def test_periodic_indels_a_passing_prefix_then_a_failing_group(diag):
    run_child("periodic_indels", diag)


@LIBS
def test_tie_rich_pairs(diag):
    run_child("tie_rich", diag)


@LIBS
def test_displaced_paths(diag):
    run_child("displaced", diag)


@LIBS
def test_clamps_and_views(diag):
    run_child("clamps", diag)


@LIBS
def test_unequal_units_edit_strings_and_n_holding_calls(diag):
    run_child("mixed_units", diag)


def test_refusals_defaults_and_two_contexts_in_different_modes():
    out = run_child("defaults")
    assert "ENV_MODE 0" in out


def test_the_environment_default():
    out = run_child("defaults", extra={"GAMDP_WALK_SKIP": "1", "GAMDP_WALK_SKIP_TEST_ENV_ONLY": "1"})
    assert "ENV_MODE 1" in out
    out = run_child("defaults", extra={"GAMDP_WALK_SKIP": "0", "GAMDP_WALK_SKIP_TEST_ENV_ONLY": "1"})
    assert "ENV_MODE 0" in out


def test_merge_blocks_do_not_depend_on_it():
    run_child("merge_blocks")
