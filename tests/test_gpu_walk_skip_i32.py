"""gamdp_ctx_set_walk_skip_i32: the walks of the int32 direction-free kernels jump over groups of 64 rows that provably hold diagonal
steps only (kernel_finish.inc, finish_walk<..., SKIP> on int32 checkpoint images, with the reference's three-valued score where a
sequence may hold N).  Six kernels, each reached the way tests/_views.py CELLS reaches it:

    c17    k_align<17,4,false>      band 512, GAMDP_NO_PAIR=1
    c17n   k_align<17,4,true>       band 512, N-holding calls
    q19    k_align_q<19,15,false>   band 150, GAMDP_NO_PAIR=1 GAMDP_QUAD_MIN=1
    q19n   k_align_q<19,15,true>    band 150, N-holding calls, GAMDP_QUAD_MIN=1
    gen9   k_align<9,-1,true>       band 200
    gen17  k_align<17,-1,true>      band 300

Every case runs on ONE context with the property off and on: every field of every result equals the oracle's, and the two runs are
equal field by field (edit strings included where asked for).  What the walks did is read from gamdp_ctx_walk_skip_i32_stats and
gamdp_ctx_launch_info; the kernel's name is asserted from the latter.  The cases run in fresh child processes (never exec), each with a
timeout of its own.

A call reaches c17n / q19n only if its window holds an N: route() gives a pair that has none one N at a[5], in the top blocks and far
from the direction-free range, so an "identical pair" of those two kernels is identical but for that base or holds it on both sides.

Sizes: SHORT is the shortest length (scanning upward in steps of 64 bases, identical pair, whole sequences) at which the
direction-free range holds at least 3 groups -- found on the device by the child itself and asserted -- and the cases use SHORT, about
twice SHORT + 21 and pairs of 3 - 6 kb.

Where the end cell lies.  These kernels end their direction-free range at the last whole group of 4 blocks (fill_task: df_hi =
b2 & ~3), and no checkpoint row is stored at df_hi: a walk that comes down into the range from tagged blocks above it has no upper
value for its first span and takes one strip there (16 groups) before it tests again.  The span below an END cell takes the score as
its upper value, so a walk whose end cell lies inside the range needs no strip at all.  "Gap-free pairs need no strip" is that second
statement, so the lengths of the cases that assert it are rounded up by fit(): rows + LE a multiple of 64 (LE = the lane of the
band's last column), which makes the task's last block the last block of a group -- the whole END run lies in the range."""
import os
import random

import pytest

import _cases
import _oracle as O
import _walkskip as W
import gam_ngs_amd as gam
from _walkskip import (SIX, both, case, check_stats, ctx, fit, gap_free, mine, one_indel, oracle_all, run, setup, short_length, sizes, substituted,
                       trimmed)
from _walkskip import F as K     # the kernel this child is about (setup()): cell, kernel, band, C, lpt, need_n, LE, lc
from gam_ngs_amd import lib as L

pytestmark = pytest.mark.gpu

KERNELS = {cell: W.FAMILIES[cell] for cell in W.I32}    # the families of tests/_walkskip.py that are named after their cell of tests/_views.py
ZERO = dict(tests=0, groups_tested=0, groups_skipped=0, rows_skipped=0, strips=0, mode=0, launches=0)
STRIP_GROUPS = 16        # groups one strip call re-creates in these kernels (strips of 4 lanes: kernel_fill.inc Strip::groups_of)


# ---- in the child ------------------------------------------------------------------------------------------------------------------

def range_rows(n):
    """rows of an identical pair of length n = fit(n) between the first row-time of the direction-free range and the end cell
    (begin_a = 0: fill_task's lo = first group start behind the top blocks and one tagged block)"""
    bt = (max(K.LE + 1, K.band + 1) + 15) // 16
    lo = (bt + 1 + 3) & ~3
    return (n - 1 + K.lc) - 16 * lo + 1


def takes(cs):
    """whether the kernel under test takes this call by its bases (a window without N inside an N-holding pair: the launch record tells)"""
    has_n = b"N" in cs["a"] + cs["b"]
    return K.need_n is None or K.need_n == has_n


def six_strips(info):
    return sum(r["strips"] for r in info if r["kernel"] in SIX)


def sprinkled(a, b, every=37):
    """N into both sequences at equal indices, in turn on a's side, on b's side and on both: N-base, base-N and N-N pairs on the path
    of a gap-free alignment"""
    a, b = list(a), list(b)
    kinds = set()
    for k, at in enumerate(range(every, min(len(a), len(b)) - 1, every)):
        if k % 3 != 1:
            a[at] = "N"
        if k % 3 != 0:
            b[at] = "N"
        kinds.add(k % 3)
    assert kinds == {0, 1, 2}
    return "".join(a), "".join(b)


def child_gap_free():
    """1. identical pairs, pairs with substitutions only and (N-aware kernels) the same with N on either and on both sides: no strip at
    all with the property on"""
    rng = random.Random(1)
    for n in sizes():
        a = _cases.rand_seq(rng, n)
        cases = [case(a, a, same=True), case(a, substituted(rng, a, 0.02))]
        if K.need_n is not False:
            cases += [case(*sprinkled(a, a)), case(*sprinkled(a, substituted(rng, a, 0.02)))]
        want = oracle_all(cases)      # (asserted gap-free on the CPU before the GPU is asked anything)
        assert all(o.status == O.OK and gap_free(ops) and o.length >= n - 64 for o, ops in want)
        assert all(o.n_match == ops.count("M") > 0 for o, ops in want)
        _, info0, info1, st0, st1 = both(cases, False, want)
        assert sum(r["units_dirfree"] for r in info1) == sum(r["units"] for r in info1) > 0, info1
        assert st0["strips"] > 0, (st0, info0)
        assert st1["strips"] == 0 and six_strips(info1) == 0, (st1, info1)
        assert st1["groups_skipped"] > 0 and st1["groups_skipped"] == st1["groups_tested"], st1
        # every row of the direction-free range below the end cells is jumped over
        assert st1["rows_skipped"] >= len(cases) * range_rows(n), (st1, n, range_rows(n))
        both(cases, True, want)


def child_one_indel():
    """2. one 1-base insertion or deletion at row 64 g + d: a strip there, rows jumped over above and below"""
    rng = random.Random(2)
    n = 6000                           # 94 groups: a strip call serves 16 of them
    cases, rows = [], []
    # d: around row 64 g, and around row-time 64 g of the lane the centred path runs in (row-time = row + lc)
    for g in (50, 70):
        for d in (-2, -1, 0, 1, -2 - K.lc, -1 - K.lc, -K.lc, 1 - K.lc):
            for kind in ("ins", "del"):
                cases.append(one_indel(rng, n, 64 * g + d, kind))
                rows.append(64 * g + d)
    want = oracle_all(cases)
    for (o, ops) in want:
        assert o.status == O.OK and sum(1 for ch in ops if ch in "AB") == 1, ops.count("A")
    # one call at a time: the statistics of a call are its own
    for k in range(len(cases)):
        _, info0, info1, st0, st1 = both(cases[k:k + 1], False, want[k:k + 1])
        row, rows_k = rows[k], len(cases[k]["b"])
        assert 1 <= st1["strips"] <= st0["strips"], (row, st0, st1)
        # rows above the indel, and rows below the 16 groups its strip call serves: more than either side alone has
        assert st1["tests"] >= 2 and st1["rows_skipped"] > max(rows_k - row, row - (STRIP_GROUPS - 1) * 64) + 64, (row, st1)
    both(cases, True, want, only=K.lpt == 64)


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
            last = at + 2 * step >= n      # (the last stretch stays as it is: the span below the end cell passes)
            b.append(seg if last else (seg[:-1] if rng.random() < 0.5 else seg + rng.choice("ACGT")))
            at += step
        cases.append(case(*trimmed(a, "".join(b))))
    for cs in cases:
        _, info0, info1, st0, st1 = both([cs], False)
        assert st1["groups_skipped"] > 0 and st1["groups_tested"] > st1["groups_skipped"], st1
        assert 0 < st1["strips"] <= st0["strips"], (st0, st1)
    both(cases, True)


def tie_cases():
    """_ties.long_cases(band) at the two bands it knows (150, 512); the same construction on the 6 kb pairs at the bands
    of the generic kernels -> (cases, oracle answers)"""
    import _ties as TW
    if K.band in TW.LONG_BANDS:
        return list(TW.long_cases(K.band)), list(TW.wants("long", K.band))
    tie = _cases.tie_window_cases(TW.SEED, (K.band,), (6000,), 4)
    rng = random.Random(7700 + K.band)
    out = []
    for cs in tie:
        a = _cases.rand_seq(rng, len(cs["a"]))
        b = (_cases.mutate(rng, a) + _cases.rand_seq(rng, 64))[:len(cs["b"])]
        out.append(cs)
        out.append(dict(cs, a=a.encode(), b=b.encode(), fs=False, fe=False, tag=("partner of",) + cs["tag"]))
    return out, oracle_all(out)


def child_tie_rich():
    """4. homopolymers, dinucleotide and tandem repeats (`up` / `left` tie with `diag` all along the path), N-holding ones for the N-aware
    kernels; paths displaced to the first and last column of a lane and to the band's edge columns"""
    every, allw = tie_cases()
    keep = [k for k, cs in enumerate(every) if takes(cs)]
    cases, want = [every[k] for k in keep], [allw[k] for k in keep]
    kinds = {cs["tag"][0] for cs in cases}
    assert len(cases) >= 12 and kinds >= {"homopolymer", "ac_shift1"} and any(t.startswith("tandem") for t in kinds), (len(cases), kinds)
    if K.need_n is not False:
        assert any(b"N" in cs["a"] + cs["b"] for cs in cases)
    _, info0, info1, st0, st1 = both(cases, False, want, only=False)
    # (a window that holds none of its pair's N goes to another kernel: half of the N-holding cases at least stay)
    assert sum(r["tasks"] for r in mine(info1)) >= (6 if K.need_n else 12), info1
    assert st1["groups_skipped"] > 0 and st1["groups_tested"] > st1["groups_skipped"], st1
    both(cases, True, want, only=False)
    cases = [cs for cs in _cases.displaced_path_cases(K.band) if takes(cs)]
    want = oracle_all(cases)
    cols = set()
    for cs, (o, ops) in zip(cases, want):
        assert o.status == O.OK
        cols.add(o.begin_a - cs["begin_a"] - (o.begin_b - cs["begin_b"]) + K.band)
    assert len(cols) >= 6 and (K.need_n or (min(cols) <= 3 and max(cols) >= 2 * K.band - 3)), sorted(cols)
    _, info0, info1, st0, st1 = both(cases, False, want, only=False)
    assert sum(r["tasks"] for r in mine(info1)) >= 6, info1
    assert st1["groups_skipped"] > 0 and st1["strips"] <= st0["strips"], (st0, st1)
    both(cases, True, want, only=False)


def child_clamps():
    """5. spans that would cross pos == 0, a b shorter than a span, windows, the four force-flag combinations, rc and suffix views"""
    rng = random.Random(6)
    s = short_length()
    cases = []
    for k in (1, 63, 64, 65, 100, K.band - 1):    # b has k bases in front: the path reaches pos == 0 in row k
        a = _cases.rand_seq(rng, 2 * s)
        cases.append(case(a, _cases.rand_seq(rng, k) + a))
        cases.append(case(a, _cases.rand_seq(rng, k) + a, begin_a=0, fs=True))
    for ba in (1, 2, 63, 64, 65, 127, 128, 129, K.band + 1, K.band + 190):   # the window begins ba bases into a
        a = _cases.rand_seq(rng, 2 * s + ba)
        if K.need_n:
            a = a[:ba + 70] + "N" + a[ba + 71:]     # (inside the window: route()'s N at a[5] may lie in front of it)
        cases.append(case(a, a[ba:], begin_a=ba))
        cases.append(case(a, a, begin_a=ba))
    for nb in (1, 40, 63, 64, 65, 130):           # b shorter than a span / than two
        a = _cases.rand_seq(rng, 3000)
        cases.append(case(a, a[:nb]))
        cases.append(case(a, a[:nb]))
    for fs, fe in ((False, False), (True, False), (False, True), (True, True)):
        a = _cases.rand_seq(rng, 3 * s)
        if K.need_n:
            a = a[:300] + "N" + a[301:]
        b = substituted(rng, a, 0.01)
        cases.append(case(a, b, fs=fs, fe=fe))
        cases.append(case(a, b, begin_a=40, end_a=len(a) - 70, begin_b=35, end_b=len(b) - 90, fs=fs, fe=fe))
    _, info0, info1, st0, st1 = both(cases, False, only=False)
    assert sum(r["tasks"] for r in mine(info1)) >= len(cases) - 12, info1
    assert st1["groups_skipped"] > 0, st1
    both(cases, True, only=False)
    # views: the kernel's cell of tests/_views.py (all view kinds), view call and copy call, both modes
    import _views as V
    import test_gpu_views as TV
    vcases = [cs for cs in V.matrix_cases() if cs["cell"] == K.cell]
    assert vcases
    vwant = TV._oracle_all(vcases)
    c = ctx()
    seen = {}
    for mode in (L.WALK_STRIPS, L.WALK_SKIP_DIAG):
        c.set_walk_skip_i32(mode)
        try:
            res = TV.run_view_and_copy(c, vcases, want_ops=False)
        finally:
            c.set_walk_skip_i32(L.WALK_STRIPS)
        TV.compare(vcases, res, vwant, False, V.digest(vcases))
        info, st = c.launch_info(), c.walk_skip_i32_stats()
        assert mine(info), info
        check_stats(st, info, mode)
        seen[mode] = ([(rv.key(), rc_.key()) for rv, rc_ in res], st)
    assert seen[0][0] == seen[1][0]
    assert seen[1][1]["tests"] > 0 and (K.cell not in V.LONG_CELLS or seen[1][1]["groups_skipped"] > 0), seen[1][1]
    print("  views: %s" % (seen[1][1],))


def child_quad_units():
    """6. four-task kernels: the four tasks of a wavefront differ in length by several groups, and the batch is not a multiple of 4"""
    assert K.lpt == 16
    rng = random.Random(7)
    s = short_length()
    cases = []
    # the planner sorts by size: neighbours in this list share a wavefront; they differ by 3 - 12 groups
    for n in (s, s + 200, 2 * s, 2 * s + 800, 5200, 5400, 5600, 6000, 4000, 4700):
        a = _cases.rand_seq(rng, n)
        cases.append(case(a, _cases.mutate(rng, a, 0.01, 0.001, 0.001)))
    _, info0, info1, st0, st1 = both(cases, False)
    assert sum(r["units"] for r in info1) == 3 and sum(r["tasks"] for r in info1) == 10, info1
    assert st1["groups_skipped"] > 0, st1
    both(cases, True)
    both(cases[:5], False)


def child_edit_strings():
    """7. edit strings wanted for some tasks (those never test) and for all (nothing is tested)"""
    rng = random.Random(8)
    s = short_length()
    cases = []
    for n in (fit(2 * s), fit(3000), fit(4000), fit(4700), fit(5200), fit(6000)):
        a = _cases.rand_seq(rng, n)
        cases.append(case(a, substituted(rng, a, 0.01)))
    _, _, _, st0, st1 = both(cases, False)
    assert st1["groups_skipped"] > 0, st1
    flags = [k % 3 == 0 for k in range(len(cases))]
    _, _, _, st0f, st1f = both(cases, flags)
    assert 0 < st1f["groups_skipped"] < st1["groups_skipped"], (st1f, st1)
    _, _, _, _, st1a = both(cases, True)
    assert st1a["tests"] == 0 and st1a["groups_skipped"] == 0 and st1a["launches"] > 0, st1a


def child_independence():
    """8. the three properties are independent (GAMDP_QUAD_MIN=1: band 512 N-free -> k_align_p<17,4>, band 150 N-free -> k_align_o<19,15>,
    band 150 N-holding -> k_align_q<19,15,true>)"""
    setup("q19n")
    rng = random.Random(9)
    c = ctx()
    a = _cases.rand_seq(rng, 3000)
    mk = lambda x, y, band: dict(a=x.encode(), b=y.encode(), band=band, begin_a=0, end_a=len(x) - 1, begin_b=0, end_b=len(y) - 1, fs=False, fe=False)
    an = a[:1500] + "N" + a[1501:]
    cn = [mk(an, an, 150), mk(an, substituted(rng, a, 0.01), 150)]
    wantn = oracle_all(cn)
    # the two older properties alone leave these counters at 0
    c.set_walk_skip(L.WALK_SKIP_DIAG)
    c.set_walk_skip_pair(L.WALK_SKIP_DIAG)
    try:
        res = run(cn, False)
        st, info = c.walk_skip_i32_stats(), c.launch_info()
    finally:
        c.set_walk_skip(L.WALK_STRIPS)
        c.set_walk_skip_pair(L.WALK_STRIPS)
    assert [r.key() for r in res] == [o.key() for o, _ in wantn]
    assert {r["kernel"] for r in info} == {K.kernel}, info
    check_stats(st, info, L.WALK_STRIPS)
    assert st["strips"] > 0, st
    # this property alone leaves theirs at 0, and the launches of their kernels as they were
    b = substituted(rng, a, 0.01)
    packed = [mk(a, a, 512), mk(a, b, 512)] + [mk(a, a, 150), mk(a, b, 150)] * 4
    wantp = oracle_all(packed[:4])
    wantp = wantp[:2] + wantp[2:] * 4
    seen = {}
    for mode in (L.WALK_STRIPS, L.WALK_SKIP_DIAG):
        c.set_walk_skip_i32(mode)
        try:
            res = run(packed, False)
            seen[mode] = (c.launch_info(), c.walk_skip_stats(), c.walk_skip_pair_stats(), c.walk_skip_i32_stats())
        finally:
            c.set_walk_skip_i32(L.WALK_STRIPS)
        assert [r.key() for r in res] == [o.key() for o, _ in wantp]
    timeless = lambda info: [{k: v for k, v in r.items() if "ms" not in k} for r in info]
    assert {r["kernel"] for r in seen[1][0]} == {"k_align_p<17,4>", "k_align_o<19,15>"}, seen[1][0]
    assert timeless(seen[0][0]) == timeless(seen[1][0]), (seen[0][0], seen[1][0])
    for mode in (0, 1):
        _, st8, stp, sti = seen[mode]
        assert st8["tests"] == st8["groups_skipped"] == 0 and st8["strips"] > 0 and st8["mode"] == L.WALK_STRIPS, st8
        assert stp["tests"] == stp["groups_skipped"] == 0 and stp["strips"] > 0 and stp["mode"] == L.WALK_STRIPS, stp
        assert sti == ZERO, sti       # a call without a launch of the six kernels: everything 0
    # ... and with all three on, each counts its own kernel
    c.set_walk_skip(L.WALK_SKIP_DIAG)
    c.set_walk_skip_pair(L.WALK_SKIP_DIAG)
    c.set_walk_skip_i32(L.WALK_SKIP_DIAG)
    try:
        res = run(packed + cn, False)
        info, st8, stp, sti = c.launch_info(), c.walk_skip_stats(), c.walk_skip_pair_stats(), c.walk_skip_i32_stats()
    finally:
        c.set_walk_skip(L.WALK_STRIPS)
        c.set_walk_skip_pair(L.WALK_STRIPS)
        c.set_walk_skip_i32(L.WALK_STRIPS)
    assert [r.key() for r in res] == [o.key() for o, _ in wantp + wantn]
    check_stats(sti, info, L.WALK_SKIP_DIAG)
    assert sti["launches"] == 1 and sti["groups_skipped"] > 0 and st8["groups_skipped"] > 0 and stp["groups_skipped"] > 0, (st8, stp, sti)


def child_defaults():
    """9. refusals, the statistics before any call, the environment default, two contexts of a multi handle in different modes, a
    merge-block call at band 200"""
    import ctypes
    setup("gen9")
    l = L.load_library()
    c = gam.Context(0)
    assert l.gamdp_ctx_walk_skip_i32_stats(c.handle, None) == L.EINVAL
    assert l.gamdp_ctx_set_walk_skip_i32(None, L.WALK_SKIP_DIAG) == L.EINVAL
    for mode in (-1, 2, 7, 1 << 20):
        assert l.gamdp_ctx_set_walk_skip_i32(c.handle, mode) == L.EINVAL
        with pytest.raises(gam.GamdpError):
            c.set_walk_skip_i32(mode)
    want_mode = L.WALK_SKIP_DIAG if os.environ.get("GAMDP_WALK_SKIP_I32") == "1" else L.WALK_STRIPS
    assert c.walk_skip_i32_stats() == ZERO
    # the mode of a fresh context: what its first call reports
    rng = random.Random(9)
    a = _cases.rand_seq(rng, fit(3000))
    cs = case(a, a)
    sset = gam.SequenceSet(c, [cs["a"], cs["b"]], ascii=True)
    call = [(sset.contig(0), 0, len(a) - 1, sset.contig(1), 0, len(a) - 1, False, False)]
    res = gam.BandedSmithWaterman(c).find_alignments(call, bands=[K.band])
    st, info = c.walk_skip_i32_stats(), c.launch_info()
    assert [r["kernel"] for r in info] == [K.kernel], info
    assert all(r.key() == oracle_all([cs])[0][0].key() for r in res)
    check_stats(st, info, want_mode)
    assert (st["groups_skipped"] > 0) == (want_mode == L.WALK_SKIP_DIAG), st
    print("ENV_MODE %d" % st["mode"])
    sset.close()
    if os.environ.get("GAMDP_WALK_SKIP_I32_TEST_ENV_ONLY"):
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
    m.set_walk_skip_i32(L.WALK_SKIP_DIAG, which=1)
    ms = gam.MultiSequenceSet(m, seqs, ascii=True)
    calls = [(ms.contig(2 * i), k["begin_a"], k["end_a"], ms.contig(2 * i + 1), k["begin_b"], k["end_b"], False, False) for i, k in enumerate(cases)]
    res = gam.BandedSmithWaterman(m).find_alignments(calls, bands=[K.band] * len(cases))
    sts = m.walk_skip_i32_stats()
    ms.close()
    m.close()
    for r, (o, _) in zip(res, want):
        assert r.key() == o.key()
    assert [s["mode"] for s in sts] == [L.WALK_STRIPS, L.WALK_SKIP_DIAG], sts
    assert sts[0]["groups_skipped"] == 0 and sts[1]["groups_skipped"] > 0 and sts[0]["strips"] > 0, sts
    # gamdp_align_merge_blocks at band 200 (the round loop launches k_align<9,-1,true>): gamdp_mb_out and the audit do not depend on the property
    import _l1cases
    import test_gpu_l1_chain_carry as T
    scs = _l1cases.scenarios(900, 24)
    outs = {}
    for mode in (L.WALK_STRIPS, L.WALK_SKIP_DIAG):
        c.set_walk_skip_i32(mode)
        try:
            stats = T.check(c, scs, K.band)          # against the oracle's driver, audit included
            outs[mode] = [T.outcome(mb) for mb in T.run(c, scs, K.band)]
        finally:
            c.set_walk_skip_i32(L.WALK_STRIPS)
        assert stats["ok"] >= 3, stats
    assert outs[0] == outs[1]


CHILDREN = {f.__name__[len("child_"):]: f for f in (child_gap_free, child_one_indel, child_periodic_indels, child_tie_rich, child_clamps,
                                                    child_quad_units, child_edit_strings, child_independence, child_defaults)}


# ---- the tests: one fresh child each (never exec) --------------------------------------------------------------------------------

def run_child(name, cell=None, diag=False, extra=None):
    return W.run_child("test_gpu_walk_skip_i32", name, cell, diag, extra)


CELLS = pytest.mark.parametrize("cell", sorted(KERNELS))


@CELLS
@pytest.mark.parametrize("diag", (False, True), ids=("product", "diag"))
def test_gap_free_pairs_need_no_strip(cell, diag):
    """Fails without the feature: with the property on not one strip is re-created for pairs whose alignment holds no gap."""
    run_child("gap_free", cell, diag)


@CELLS
def test_one_indel_around_a_group_boundary(cell):
    run_child("one_indel", cell)


@CELLS
def test_periodic_indels_a_passing_prefix_then_a_failing_group(cell):
    run_child("periodic_indels", cell)


@CELLS
def test_tie_rich_pairs_and_displaced_paths(cell):
    run_child("tie_rich", cell)


@CELLS
def test_clamps_and_views(cell):
    run_child("clamps", cell)


@pytest.mark.parametrize("cell", ("q19", "q19n"))
def test_unequal_tasks_of_a_wavefront_and_a_batch_that_is_no_multiple_of_four(cell):
    run_child("quad_units", cell)


@CELLS
def test_edit_strings_for_some_and_for_all(cell):
    run_child("edit_strings", cell)


def test_the_three_properties_are_independent():
    run_child("independence", extra={"GAMDP_QUAD_MIN": "1"})


def test_refusals_defaults_two_contexts_in_different_modes_and_merge_blocks():
    assert "ENV_MODE 0" in run_child("defaults")


def test_the_environment_default():
    assert "ENV_MODE 1" in run_child("defaults", extra={"GAMDP_WALK_SKIP_I32": "1", "GAMDP_WALK_SKIP_I32_TEST_ENV_ONLY": "1"})
    assert "ENV_MODE 0" in run_child("defaults", extra={"GAMDP_WALK_SKIP_I32": "0", "GAMDP_WALK_SKIP_I32_TEST_ENV_ONLY": "1"})
