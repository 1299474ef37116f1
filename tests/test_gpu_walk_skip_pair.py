"""gamdp_ctx_set_walk_skip_pair: the walks of the two-task band-512 kernel (k_align_p<17,4>) jump over groups of 64 rows that provably
hold diagonal steps only -- side by side (kernel_walk.inc, walk_many<17, 4, ..., 2, 64, SKIP>) and one task after the other
(kernel_finish.inc, finish_walk<..., SKIP>).

Every case runs on ONE context with the property off and on: every field of every result equals the oracle's, and the two runs are
equal field by field (edit strings included where asked for).  What the walks did is read from gamdp_ctx_walk_skip_pair_stats and
gamdp_ctx_launch_info.  The cases run in fresh child processes, each child twice: with GAMDP_SIDE_WALK_ROUNDS=0 (every launch walks
one task after the other) and with GAMDP_SIDE_WALK_ROUNDS=1000000 (every launch walks its two tasks side by side) -- the path taken
is asserted from launches_one_by_one / launches_side_by_side -- on the product library and on the diagnostics library
(libgamdp_diag.so, which also reports a packed value that left the exact f16 range).  Band 512, N-free pairs.

Sizes: SHORT is the shortest length (scanning upward in steps of 64 bases, identical pair, whole sequences) at which the
direction-free range holds at least 3 groups -- found on the device by the child itself and asserted -- and the cases use SHORT, about
twice SHORT and pairs of 3 - 6 kb."""
import os
import random

import pytest

import _cases
import _oracle as O
import _walkskip as W
import gam_ngs_amd as gam
from _walkskip import both, case, check_path, ctx, gap_free, one_indel, oracle_all, run, short_length, sizes, substituted
from gam_ngs_amd import lib as L

pytestmark = pytest.mark.gpu

FAMILIES = ("p17_one", "p17_side")   # of tests/_walkskip.py: GAMDP_SIDE_WALK_ROUNDS=0 and =1000000, every child runs as both in turn
BAND, C = 512, 17
KERNEL = W.P17
ZERO = dict(tests=0, groups_tested=0, groups_skipped=0, rows_skipped=0, strips=0, mode=0, launches_side_by_side=0, launches_one_by_one=0)


# ---- in the child ------------------------------------------------------------------------------------------------------------------

def pair_strips(info):
    return sum(r["strips"] for r in info if r["kernel"] == KERNEL)


def child_gap_free():
    """1. identical pairs and pairs with substitutions only: no strip at all with the property on.  The statement of
    test_gpu_walk_skip.test_gap_free_pairs_need_no_strip holds in this format as it stands: the two tasks of a wavefront are of one
    length here, so the packed range runs on over both end cells and the span below an end cell takes the score as its upper value."""
    rng = random.Random(1)
    for n in sizes():
        a = _cases.rand_seq(rng, n)
        cases = [case(a, a), case(a, substituted(rng, a, 0.02))]
        want = oracle_all(cases)
        assert all(o.status == O.OK and gap_free(ops) and o.length >= n - 64 for o, ops in want)
        _, info0, info1, st0, st1 = both(cases, False, want)
        assert [r["units_dirfree"] for r in info1] == [1], info1
        assert pair_strips(info0) > 0, info0
        assert st1["strips"] == 0 and pair_strips(info1) == 0, (st1, info1)
        assert st1["groups_skipped"] > 0 and st1["groups_skipped"] == st1["groups_tested"], st1
        # every row of the direction-free range is jumped over: all rows but the ramp, the first eight blocks and a partial group
        assert st1["rows_skipped"] >= 2 * (n - 300), (st1, n)
        both(cases, True, want)


def child_one_indel():
    """2. one 1-base insertion or deletion at row 64 g + d: a strip there, rows jumped over above and below"""
    rng = random.Random(2)
    n = 6000                           # 94 groups: a strip call of the band's centre serves 32 of them
    cases, rows = [], []
    # d: around row 64 g, and around row-time 64 g of the lane the centred path runs in (lane 30 of 61: row-time = row + 30)
    for g in (50, 70):
        for d in (-2, -1, 0, 1, -32, -31, -30, -29):
            for kind in ("ins", "del"):
                cases.append(one_indel(rng, n, 64 * g + d, kind))
                rows.append(64 * g + d)
    want = oracle_all(cases)
    for (o, ops) in want:
        assert o.status == O.OK and sum(1 for ch in ops if ch in "AB") == 1, ops.count("A")
    # two calls at a time (one wavefront): the statistics of a call are its own
    for k in range(0, len(cases), 2):
        _, info0, info1, st0, st1 = both(cases[k:k + 2], False, want[k:k + 2])
        row = rows[k]
        assert st1["strips"] >= 2 and st1["strips"] <= st0["strips"], (row, st0, st1)
        # per task: rows above the indel, and rows below the 32 groups its strip call serves: more than either side alone has
        assert st1["tests"] >= 4 and st1["rows_skipped"] > 2 * (max(n - row, row - 32 * 64) + 64), (row, st1)
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
    for cs in cases:
        _, info0, info1, st0, st1 = both([cs, cs], False)
        assert st1["groups_skipped"] > 0 and st1["groups_tested"] > st1["groups_skipped"], st1
        assert 0 < st1["strips"] <= st0["strips"], (st0, st1)
    both(cases, True)


def child_tie_rich():
    """4. homopolymers, dinucleotide and tandem repeats: `up` / `left` tie with `diag` all along the path"""
    import _ties as TW
    every = TW.long_cases(BAND)
    keep = [k for k, cs in enumerate(every) if b"N" not in cs["a"] + cs["b"]]
    cases = [every[k] for k in keep]
    assert len(cases) >= 40 and {cs["tag"][0] for cs in cases} >= {"homopolymer", "ac_shift1", "tandem19", "complement"}
    allw = TW.wants("long", BAND)
    want = [allw[k] for k in keep]
    _, info0, info1, st0, st1 = both(cases, False, want, only=False)
    assert sum(r["tasks"] for r in info1 if r["kernel"] == KERNEL) >= 40, info1
    assert st1["groups_skipped"] > 0 and st1["groups_tested"] > st1["groups_skipped"], st1
    both(cases, True, want, only=False)


def child_displaced():
    """5. test_gpu_strip_widths.displaced(): paths on the first and last column of every strip (so of a lane's first and last column
    at the strips' borders), in the first and last strip of the task, next to the band's edge columns; with and without top blocks"""
    import test_gpu_strip_widths as SW
    cases = list(SW.displaced_cases())
    want = oracle_all(cases)
    cols = set()
    for cs, (o, ops) in zip(cases, want):
        assert o.status == O.OK
        cols.add(o.begin_a - cs["begin_a"] - (o.begin_b - cs["begin_b"]) + BAND)
    assert min(cols) <= 3 and max(cols) >= 2 * BAND - 3 and len(cols) >= 24, sorted(cols)
    _, info0, info1, st0, st1 = both(cases, False, want)
    assert st1["groups_skipped"] > 10 * len(cases) and st1["strips"] < st0["strips"], (st0, st1)
    both(cases, True, want)


def child_clamps():
    """6. spans that would cross pos == 0, a b shorter than a span, windows, the four force-flag combinations, rc and suffix views"""
    rng = random.Random(6)
    s = short_length()
    cases = []
    for k in (1, 63, 64, 65, 100, 511):           # b has k bases in front: the path reaches pos == 0 in row k, inside the top groups
        a = _cases.rand_seq(rng, 2 * s)
        cases.append(case(a, _cases.rand_seq(rng, k) + a))
        cases.append(case(a, _cases.rand_seq(rng, k) + a, begin_a=0, fs=True))
    for ba in (1, 2, 63, 64, 65, 127, 128, 129, 513, 700):   # the window begins ba bases into a
        a = _cases.rand_seq(rng, 2 * s + ba)
        cases.append(case(a, a[ba:], begin_a=ba))
        cases.append(case(a, a, begin_a=ba))
    for nb in (1, 40, 63, 64, 65, 130):           # b shorter than a span / than two
        a = _cases.rand_seq(rng, 3000)
        cases.append(case(a, a[:nb]))
        cases.append(case(a, a[:nb]))
    for fs, fe in ((False, False), (True, False), (False, True), (True, True)):
        a = _cases.rand_seq(rng, 3 * s)
        b = substituted(rng, a, 0.01)
        cases.append(case(a, b, fs=fs, fe=fe))
        cases.append(case(a, b, begin_a=40, end_a=len(a) - 70, begin_b=35, end_b=len(b) - 90, fs=fs, fe=fe))
    _, info0, info1, st0, st1 = both(cases, False, only=False)
    assert st1["groups_skipped"] > 0, st1
    both(cases, True, only=False)
    # views: the p17 cell of tests/_views.py (all view kinds), view call and copy call, both modes
    import _views as V
    import test_gpu_views as TV
    vcases = [cs for cs in V.matrix_cases() if cs["cell"] == "p17"]
    vwant = TV._oracle_all(vcases)
    c = ctx()
    seen = {}
    for mode in (L.WALK_STRIPS, L.WALK_SKIP_DIAG):
        c.set_walk_skip_pair(mode)
        try:
            res = TV.run_view_and_copy(c, vcases, want_ops=False)
        finally:
            c.set_walk_skip_pair(L.WALK_STRIPS)
        TV.compare(vcases, res, vwant, False, V.digest(vcases))
        seen[mode] = ([(rv.key(), rc_.key()) for rv, rc_ in res], c.walk_skip_pair_stats())
    assert seen[0][0] == seen[1][0]
    assert seen[1][1]["groups_skipped"] > 0 and seen[0][1]["groups_skipped"] == 0, seen[1][1]
    print("  views: %s" % (seen[1][1],))


def child_mixed_units():
    """7. tasks of a pair that differ in length by several groups, an odd batch, edit strings for some and for all, N-holding calls"""
    rng = random.Random(7)
    s = short_length()
    cases = []
    # the planner sorts by size: neighbours in this list share a wavefront; they differ by 3 - 12 groups
    for n in (s, s + 200, 2 * s, 2 * s + 800, 5200, 5400, 5500, 6000, 4000, 4700):
        a = _cases.rand_seq(rng, n)
        cases.append(case(a, _cases.mutate(rng, a, 0.01, 0.001, 0.001)))
    _, info0, info1, st0, st1 = both(cases, False)
    assert sum(r["units"] for r in info1) == 5 and sum(r["tasks"] for r in info1) == 10, info1
    assert st1["groups_skipped"] > 0, st1
    # some tasks want their edit string: they keep their strips (and the one-task walk), the others jump
    flags = [k % 3 == 0 for k in range(len(cases))]
    _, _, _, st0f, st1f = both(cases, flags)
    assert 0 < st1f["groups_skipped"] < st1["groups_skipped"], (st1f, st1)
    # all tasks want their edit string: nothing is tested
    _, _, _, _, st1a = both(cases, True)
    assert st1a["tests"] == 0 and st1a["groups_skipped"] == 0, st1a
    # an odd batch: the last task goes to another kernel, and its launch record is what it was
    odd = cases[:5]
    _, oinfo0, oinfo1, ost0, ost1 = both(odd, False, only=False)
    rest = lambda info: sorted((r["kernel"], r["tasks"], r["units"], r["strips"], r["units_dirfree"]) for r in info if r["kernel"] != KERNEL)
    assert rest(oinfo0) == rest(oinfo1), (oinfo0, oinfo1)
    assert sum(r["tasks"] for r in oinfo1) == 5 and ost1["groups_skipped"] > 0, (oinfo1, ost1)
    # N-holding calls beside the batch: the N-aware launch and its strip count are what they were, the statistics are the two-task launches' alone
    ncases = []
    for n in (2 * s, 3000, 4000):
        a = _cases.rand_seq(rng, n)
        b = list(_cases.mutate(rng, a, 0.01, 0.001, 0.001))
        b[len(b) // 2] = "N"
        ncases.append(case(a, "".join(b)))
    _, info0, info1, st0m, st1m = both(cases + ncases, False, only=False)
    nrec = lambda info: sorted((r["kernel"], r["tasks"], r["strips"]) for r in info if r["n_aware"])
    assert nrec(info0) == nrec(info1) and sum(t for _, t, _ in nrec(info1)) == len(ncases), (info0, info1)
    assert (st1m["tests"], st1m["groups_tested"], st1m["groups_skipped"], st1m["rows_skipped"], st1m["strips"]) == \
           (st1["tests"], st1["groups_tested"], st1["groups_skipped"], st1["rows_skipped"], st1["strips"]), (st1m, st1)
    # a call without a two-task launch: everything 0
    c = ctx()
    c.set_walk_skip_pair(L.WALK_SKIP_DIAG)
    try:
        run(ncases, False)
        st = c.walk_skip_pair_stats()
    finally:
        c.set_walk_skip_pair(L.WALK_STRIPS)
    assert st == ZERO, st


def child_independence():
    """8. the two properties are independent: gamdp_ctx_set_walk_skip alone leaves the pair counters at 0 at band 512, the new property
    alone leaves gamdp_ctx_walk_skip_stats at 0 at band 150"""
    rng = random.Random(8)
    c = ctx()
    a = _cases.rand_seq(rng, 3000)
    c512 = [case(a, a), case(a, substituted(rng, a, 0.01))]
    want = oracle_all(c512)
    c.set_walk_skip(L.WALK_SKIP_DIAG)
    try:
        res = run(c512, False)
        st, info = c.walk_skip_pair_stats(), c.launch_info()
    finally:
        c.set_walk_skip(L.WALK_STRIPS)
    assert [r.key() for r in res] == [o.key() for o, _ in want]
    assert {r["kernel"] for r in info} == {KERNEL}
    assert st["mode"] == L.WALK_STRIPS and st["tests"] == st["groups_tested"] == st["groups_skipped"] == st["rows_skipped"] == 0, st
    assert st["strips"] == pair_strips(info) > 0, (st, info)
    c150 = [dict(cs, band=150) for cs in c512] * 4
    want150 = oracle_all(c150[:2]) * 4
    c.set_walk_skip_pair(L.WALK_SKIP_DIAG)
    try:
        res = run(c150, False)
        st8, stp, info = c.walk_skip_stats(), c.walk_skip_pair_stats(), c.launch_info()
    finally:
        c.set_walk_skip_pair(L.WALK_STRIPS)
    assert [r.key() for r in res] == [o.key() for o, _ in want150]
    assert "k_align_o<19,15>" in {r["kernel"] for r in info}, info
    assert st8["mode"] == L.WALK_STRIPS and st8["tests"] == st8["groups_skipped"] == 0 and st8["strips"] > 0, st8
    assert stp == ZERO, stp


def child_defaults():
    """9. refusals, the statistics before any call, the environment default, two contexts of a multi handle in different modes"""
    import ctypes
    l = L.load_library()
    c = gam.Context(0)
    assert l.gamdp_ctx_walk_skip_pair_stats(c.handle, None) == L.EINVAL
    for mode in (-1, 2, 7, 1 << 20):
        assert l.gamdp_ctx_set_walk_skip_pair(c.handle, mode) == L.EINVAL
        with pytest.raises(gam.GamdpError):
            c.set_walk_skip_pair(mode)
    want_mode = L.WALK_SKIP_DIAG if os.environ.get("GAMDP_WALK_SKIP_PAIR") == "1" else L.WALK_STRIPS
    assert c.walk_skip_pair_stats() == ZERO
    # the mode of a fresh context: what its first call reports
    rng = random.Random(9)
    a = _cases.rand_seq(rng, 3000)
    cs = case(a, a)
    sset = gam.SequenceSet(c, [cs["a"], cs["b"]] * 2, ascii=True)
    call = [(sset.contig(2 * k), 0, len(a) - 1, sset.contig(2 * k + 1), 0, len(a) - 1, False, False) for k in range(2)]
    res = gam.BandedSmithWaterman(c).find_alignments(call, bands=[BAND] * 2)
    st = c.walk_skip_pair_stats()
    check_path(st, c.launch_info())
    assert all(r.key() == oracle_all([cs])[0][0].key() for r in res)
    assert st["mode"] == want_mode and (st["groups_skipped"] > 0) == (want_mode == L.WALK_SKIP_DIAG), st
    print("ENV_MODE %d" % st["mode"])
    sset.close()
    if os.environ.get("GAMDP_WALK_SKIP_PAIR_TEST_ENV_ONLY"):
        return
    # gamdp_multi: two contexts on one device, one on and one off
    cases = []
    for n in (3000, 3300, 4000, 4800, 5200, 6000, 3100, 4100):
        x = _cases.rand_seq(rng, n)
        cases.append(case(x, _cases.mutate(rng, x, 0.01, 0.001, 0.001)))
    want = oracle_all(cases)
    seqs = []
    for k in cases:
        seqs += [k["a"], k["b"]]
    m = gam.MultiContext([0, 0])
    m.set_walk_skip_pair(L.WALK_SKIP_DIAG, which=1)
    ms = gam.MultiSequenceSet(m, seqs, ascii=True)
    calls = [(ms.contig(2 * i), k["begin_a"], k["end_a"], ms.contig(2 * i + 1), k["begin_b"], k["end_b"], False, False) for i, k in enumerate(cases)]
    res = gam.BandedSmithWaterman(m).find_alignments(calls, bands=[BAND] * len(cases))
    sts = m.walk_skip_pair_stats()
    ms.close()
    m.close()
    for r, (o, _) in zip(res, want):
        assert r.key() == o.key()
    assert [s["mode"] for s in sts] == [L.WALK_STRIPS, L.WALK_SKIP_DIAG], sts
    assert sts[0]["groups_skipped"] == 0 and sts[1]["groups_skipped"] > 0 and sts[0]["strips"] > 0, sts


CHILDREN = {f.__name__[len("child_"):]: f for f in (child_gap_free, child_one_indel, child_periodic_indels, child_tie_rich, child_displaced,
                                                    child_clamps, child_mixed_units, child_independence, child_defaults)}


# ---- the tests: fresh children (never exec), one per walk path -------------------------------------------------------------------

def run_child(name, diag=False, extra=None, families=FAMILIES):
    return [W.run_child("test_gpu_walk_skip_pair", name, f, diag, extra) for f in families]


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
def test_unequal_pairs_odd_batch_edit_strings_and_n_holding_calls(diag):
    run_child("mixed_units", diag)


@LIBS
def test_the_two_properties_are_independent(diag):
    run_child("independence", diag, extra={"GAMDP_QUAD_MIN": "1"})   # (a small band-150 batch reaches the eight-task kernel only through that switch)


def test_refusals_defaults_and_two_contexts_in_different_modes():
    for out in run_child("defaults"):
        assert "ENV_MODE 0" in out


def test_the_environment_default():
    for out in run_child("defaults", extra={"GAMDP_WALK_SKIP_PAIR": "1", "GAMDP_WALK_SKIP_PAIR_TEST_ENV_ONLY": "1"}):
        assert "ENV_MODE 1" in out
    for out in run_child("defaults", extra={"GAMDP_WALK_SKIP_PAIR": "0", "GAMDP_WALK_SKIP_PAIR_TEST_ENV_ONLY": "1"}, families=FAMILIES[:1]):
        assert "ENV_MODE 0" in out
