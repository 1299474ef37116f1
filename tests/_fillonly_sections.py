"""The sections the GPU tests of the fill-only calls share -- gamdp_score_batch (tests/test_gpu_score_batch.py), gamdp_carry_batch
(tests/test_gpu_carry_batch.py) and, for views, refusals, the other calls' records, few rows and all edge bands, gamdp_carry_ops_batch
(tests/test_gpu_carry_ops.py) -- each stated once as a function of `kind`, with its parameters and the kinds that have it; tests_for(kind)
gives a test file its tests, under the ids they have always had.  No test collects from here.

What is compared and where the expected values come from: tests/_fillonly.py.  The min_ok caps and the counts asserted beside the
results hold for the oracle alone.

Nothing here is built to fault: every input is a valid call, or one the library documents that it refuses on the host before any launch.
"""
import inspect
import random
from concurrent.futures import ThreadPoolExecutor

import pytest

import _cases
import _fillonly as F
import _golden
import _mixed
import _oracle as O
import _views as V
from _gpu import ctx
import gam_ngs_amd as gam
from gam_ngs_amd import api
from gam_ngs_amd import lib as L

BOTH, ALL = ("score", "carry"), ("score", "carry", "carry_ops")
SECTIONS = []   # (function of kind and the parameters, the kinds that have the section, parametrize arguments or None, test name), in file order


def section(kinds, params=None, name=None):
    def register(fn):
        SECTIONS.append((fn, kinds, params, name or "test_" + fn.__name__))
        return fn
    return register


def tests_for(kind, names=()):
    """{test name: test} of the sections the kind has, for the globals() of its test file; names: {name here: the name the file has
    always had for it}"""
    def bound(fn, params):
        def test(**kw):
            fn(kind, **kw)
        test.__signature__ = inspect.Signature(list(inspect.signature(fn).parameters.values())[1:])   # (what pytest parametrises)
        test.__doc__ = fn.__doc__
        return pytest.mark.parametrize(*params)(test) if params else test
    return {dict(names).get(name, name): bound(fn, params) for fn, kinds, params, name in SECTIONS if kind in kinds}


def n_ok(answers):
    return sum(1 for o, _ in answers if o.status == O.OK)


# ---- 1. the reference's golden vectors ----------------------------------------------------------------------------------

@section(BOTH)
def golden_l0_cases(kind):
    cases, want = F.golden_l0(kind)   # (673 of them)
    F.check(cases, F.run(kind, ctx(), cases), want, "golden l0")
    assert sum(1 for _, _, e in _golden.l0_cases() if e["status"] == O.OK and not e["first_found"]) >= 5, "alignments without a MATCH"


@section(BOTH)
def golden_adversarial_cases(kind):
    """3 - 20 kb pairs built against the packed kernels' range argument; the golden file holds the CRC32 of their edit strings: the
    oracle's string is taken once it matches that CRC."""
    specs = _golden.adversarial_cases()
    assert len(specs) == 48
    cases = [F.coded(cs) for _, cs, _ in specs]
    needs_ops = F.KINDS[kind].needs_ops

    def one(k):
        cs, e = cases[k], specs[k][2]
        o, ops = O.oracle_align(cs["a"], cs["b"], cs["band"], cs["begin_a"], cs["end_a"], cs["begin_b"], cs["end_b"], False, False, want_ops=needs_ops)
        assert tuple(o.key()) == _golden.expect_key(e), specs[k][0]
        if needs_ops:
            _golden.check_ops(e, ops)
        return F.KINDS[kind].want(F.GoldenAnswer(e, o.cells), ops)
    with ThreadPoolExecutor(16) as ex:
        want = list(ex.map(one, range(len(cases))))
    F.check(cases, F.run(kind, ctx(), cases), want, "golden adversarial")


# ---- 2. random cases against the oracle ---------------------------------------------------------------------------------

@section(BOTH)
def random_small_cases(kind):
    cases = [F.coded(cs) for cs in _cases.cases(20261019, 1500) + _cases.cases(7, 300, max_len=1200, bands=(0, 2, 31, 32, 63, 64, 100, 300, 543))]
    F.check_against_oracle(kind, cases, "random", min_ok=0.5)


@section(BOTH)
def windows_that_begin_beyond_a(kind):
    F.check_against_oracle(kind, [F.coded(cs) for cs in _cases.beyond_cases(99, 600)], "beyond")


@section(BOTH, ("band", [150, 512]))
def window_cases_on_long_pairs(kind, band):
    F.check_against_oracle(kind, [F.coded(cs) for cs in _cases.window_cases(3, band, count=40)], "windows", min_ok=0.5)


@section(BOTH, ("band", [150, 512, 20]))
def one_n_around_every_edge_of_the_window(kind, band):
    cases = [dict(a=O.encode(a), b=O.encode(b), band=band, begin_a=ba, end_a=ea, begin_b=bb, end_b=eb, fs=False, fe=False)
             for a, b, ba, ea, bb, eb, _ in _cases.n_edge_cases(band)]
    F.check_against_oracle(kind, cases, "n edges", min_ok=1.0)


@section(BOTH)
def forced_starts_and_ends_around_the_gap_limit(kind):
    cases = F.force_cases()
    answers = F.check_against_oracle(kind, cases, "force")
    assert n_ok(answers) > len(cases) // 3 and len({o.status for o, _ in answers}) >= 2, "forced calls of both outcomes"


@section(ALL)
def matrices_of_1_2_16_17_rows(kind):
    rng = random.Random(1617)
    cases = []
    for rows in (1, 2, 16, 17):
        for band in (0, 1, 5, 40, 150, 512):
            for fs, fe in ((False, False), (True, False), (False, True), (True, True)):
                a, b = _cases.related_pair(rng, 90)
                begin_a, begin_b = rng.choice((0, 1, band, 30)), rng.randint(0, 20)
                cases.append(F.coded(dict(a=a.encode(), b=b.encode(), band=band, begin_a=begin_a, end_a=rng.choice((len(a) - 1, begin_a + rows, begin_a)),
                                          begin_b=begin_b, end_b=begin_b + rows - 1, fs=fs, fe=fe)))
    answers = F.check_against_oracle(kind, cases, "few rows")
    assert {o.cells // (2 * cs["band"] + 1) for cs, (o, _) in zip(cases, answers)} >= {1, 2, 16, 17}


# ---- 3. every instantiation at the bands where it takes over -----------------------------------------------------------

@section(BOTH, ("band", F.EDGE_BANDS))
def every_instantiation_at_its_edges(kind, band):
    c = ctx()
    cases = F.edge_cases(band)
    answers = F.check_against_oracle(kind, cases, "band %d" % band, min_ok=0.5)
    # the intended instantiation ran: its name from the host's launch, its column count as the wavefronts wrote it into their records
    info = F.info(kind, c)
    cols = F.cols_for(band)
    launched = sum(1 for o, _ in answers if o.status == O.OK or o.cells > 0)   # (at most: the pre-checks settle some calls that sized a matrix)
    assert len(info) == 1 and info[0]["kernel"] == F.KINDS[kind].kernel % cols and info[0]["cols"] == cols, info
    assert info[0]["band_max"] == band and 0 < info[0]["tasks"] <= launched and 0 < info[0]["slots"] <= info[0]["tasks"], info


@section(ALL)
def a_batch_of_all_edge_bands_takes_five_launches(kind):
    c = ctx()
    cases = [cs for band in F.EDGE_BANDS for cs in F.edge_cases(band)[:6]]
    F.check_against_oracle(kind, cases, "all bands")
    info = F.info(kind, c)
    assert [(r["kernel"], r["cols"]) for r in info] == [(F.KINDS[kind].kernel % k, k) for k in (2, 3, 5, 9, 17)], info
    assert [r["band_max"] for r in info] == [63, 95, 159, 287, 543], info


# ---- 4. views -----------------------------------------------------------------------------------------------------------

@section(ALL, ("cell,band", F.VIEW_CELLS))
def views_equal_explicit_copies_equal_the_oracle(kind, cell, band):
    c = ctx()
    cases = [cs for cs in F.view_cases() if cs["cell"] == cell]
    assert {tuple(cs["tag"]["kinds"]) for cs in cases} == set(V.KIND_PAIRS)   # the 16 rc / suffix combinations
    seqs = []
    for cs in cases:
        seqs += [cs["stored_a"], cs["stored_b"], cs["a"], cs["b"]]
    sset = gam.SequenceSet(c, seqs, ascii=False)
    calls = []
    for i, cs in enumerate(cases):
        calls.append((sset.contig(4 * i, *cs["va"]), cs["begin_a"], cs["end_a"], sset.contig(4 * i + 1, *cs["vb"]), cs["begin_b"], cs["end_b"], cs["fs"], cs["fe"]))
        calls.append((sset.contig(4 * i + 2), cs["begin_a"], cs["end_a"], sset.contig(4 * i + 3), cs["begin_b"], cs["end_b"], cs["fs"], cs["fe"]))
    res = F.run_calls(kind, c, calls, band=band)
    sset.close()
    answers = F.oracle_answers(cases, F.KINDS[kind].needs_ops)
    want = F.wants_of(kind, answers)
    bad = [(cs["tag"], res[2 * i], res[2 * i + 1], want[i]) for i, cs in enumerate(cases) if not (tuple(res[2 * i]) == tuple(res[2 * i + 1]) == tuple(want[i]))]
    assert not bad, (len(bad), bad[:3])
    assert n_ok(answers) >= 0.9 * len(cases)
    assert [r["cols"] for r in F.info(kind, c)] == [F.cols_for(band)]


# ---- 5. against gamdp_align_batch at the shapes the packed kernels run: (score, status, cells) of a score, every field of a carry ----

@section(BOTH)
def mixed_batch_of_2048_calls_equals_align_batch_and_the_oracle(kind):
    c = ctx()
    seqs, calls = _mixed.mixed_batch(20261019, 256, 8, band=150)
    assert len(calls) == 2048
    sset = gam.SequenceSet(c, seqs, ascii=False)
    tasks = (L.Task * len(calls))()
    _mixed.fill_tasks(tasks, calls)
    out, rec, _, _ = F.align_and(kind, c, sset, tasks, len(calls))
    sset.close()
    assert sum(1 for r in out if r.status == O.OK) > 1800
    sample = random.Random(5).sample(range(len(calls)), 32)
    cases = [dict(a=seqs[cl["a_id"]][cl["a_off"]:], b=seqs[cl["b_id"]], band=cl["band"], begin_a=cl["begin_a"], end_a=cl["end_a"], begin_b=cl["begin_b"],
                  end_b=cl["end_b"], fs=cl["fs"], fe=cl["fe"]) for cl in (calls[i] for i in sample)]
    F.check(cases, [F.KINDS[kind].got(rec[i], None) for i in sample], F.oracle_wants(kind, cases), "mixed sample")


_SYNTH = {}


def synth_batch(kind, c, band):
    """64 synthetic 50 kb pairs at `band` through gamdp_align_batch and the kind's call, once per kind and band
    -> (every field of the kind's results, their compared tuples, launches of gamdp_align_batch)"""
    if (kind, band) not in _SYNTH:
        sset = gam.SequenceSet.synthetic(c, F.SYNTH_FIRST, F.SYNTH_PAIRS, F.SYNTH_LEN)
        tasks = F.synth_tasks(sset, band)
        out, rec, _, launches = F.align_and(kind, c, sset, tasks, F.SYNTH_PAIRS)
        sset.close()
        assert all(r.status == O.OK for r in out)
        _SYNTH[kind, band] = ([F.whole(r) for r in rec], [F.KINDS[kind].got(r, None) for r in rec], launches)
    return _SYNTH[kind, band]


@section(BOTH, ("band,packed", [(150, None), (512, "k_align_p<17,4>")]), "test_64_synthetic_50kb_pairs_equal_align_batch_and_the_oracle")
def synthetic_50kb_pairs_equal_align_batch_and_the_oracle(kind, band, packed):
    c = ctx()
    _, got, launches = synth_batch(kind, c, band)
    if packed:   # (band 512: the two-task packed kernel is what a batch of this shape runs)
        assert {r["kernel"] for r in launches} == {packed}, launches
    sample = random.Random(band).sample(range(F.SYNTH_PAIRS), 32)
    cases = []
    for k in sample:
        a, b = api.synth_pair(F.SYNTH_FIRST + k, F.SYNTH_LEN)
        cases.append(dict(a=a, b=b, band=band, begin_a=0, end_a=F.SYNTH_LEN - 1, begin_b=0, end_b=len(b) - 1, fs=False, fe=False))
    F.check(cases, [got[k] for k in sample], F.oracle_wants(kind, cases), "synthetic band %d" % band)


# ---- 6. refusals, and what the context reports ----------------------------------------------------------------------------

@section(ALL)
def refusals_leave_the_context_usable(kind):
    c = ctx()
    k = F.KINDS[kind]
    sset, seqs = F.small_set(c)
    n = 8
    out, fp = F.outputs(kind, n)
    call = lambda tasks, cnt=n, s=sset, f=fp: F.call(kind, c, s, s, tasks, cnt, out, f)  # noqa: E731
    state = lambda: ([F.whole(r) for r in out], fp and list(fp))  # noqa: E731
    good = F.plain_tasks(seqs, n)
    assert call(good) == 0, c.last_error()
    first = state()
    assert all(r.status == O.OK and r.score > 0 for r in out)
    if k.struct is L.Result:
        assert all(r.n_match > 0 and r.length > 0 and r.first_found and r.last_found for r in out)
    if k.with_fp:
        assert all(first[1]) and first[1][:4] == first[1][4:]
        assert call(good, f=None) == L.EINVAL                    # NULL ops_fp
        assert call(good, 0, f=None) == L.EINVAL
    # a band above GAMDP_MAX_TUNED_BAND anywhere in the batch: the whole call, by name; then the same context again
    wide = F.plain_tasks(seqs, n)
    wide[5].band = 544
    assert call(wide) == L.ENOTSUP
    assert k.symbol in c.last_error() and "task 5" in c.last_error() and "544" in c.last_error(), c.last_error()
    assert call(good) == 0 and state() == first
    wide[5].band = 543
    assert call(wide) == 0, c.last_error()
    assert call(None, 0) == 0                                   # n == 0
    assert call(good, 0) == 0
    bad_id = F.plain_tasks(seqs, n)
    bad_id[3].b_id = 8
    assert call(bad_id) == L.EINVAL
    assert call(None, 1) == L.EINVAL
    synth = gam.SequenceSet.synthetic(c, 1, 2, 500)
    rc_task = (L.Task * 1)()
    rc_task[0].a_id, rc_task[0].b_id, rc_task[0].band, rc_task[0].b_rc = 0, 1, 20, 1
    rc_task[0].end_a, rc_task[0].end_b = 499, synth.lengths[1] - 1
    assert call(rc_task, 1, synth) == L.EINVAL                  # reverse complement of a packed-only set
    rc_task[0].b_rc = 0
    assert call(rc_task, 1, synth) == 0 and out[0].status == O.OK and (not k.with_fp or fp[0] != 0)
    if k.with_fp:   # what the pre-checks settle keeps a fingerprint of 0, whatever the array held
        settled = F.plain_tasks(seqs, n)
        settled[2].begin_b = len(seqs[5]) + 7
        for i in range(n):
            fp[i] = 0xDEADBEEF
        others = [i for i in range(n) if i != 2]
        assert call(settled) == 0 and out[2].status != O.OK and fp[2] == 0 and [fp[i] for i in others] == [first[1][i] for i in others]
    assert call(good) == 0 and state() == first
    synth.close()
    sset.close()


@section(ALL)
def the_other_calls_records_stay_and_kernel_time_grows(kind):
    """gamdp_align_batch and the two other calls first; then the kind's call leaves their launch logs as they were"""
    c = ctx()
    sset, seqs = F.small_set(c)
    n = 8
    tasks = F.plain_tasks(seqs, n)

    def one(which):
        out, fp = F.outputs(which, n)
        assert F.call(which, c, sset, sset, tasks, n, out, fp) == 0, c.last_error()
        if F.KINDS[which].struct is L.Result:
            assert [F.whole(r) for r in out] == [F.whole(r) for r in res], which
    res = (L.Result * n)()
    assert c.lib.gamdp_align_batch(c.handle, sset.handle, sset.handle, tasks, n, res, None) == 0, c.last_error()
    others = [w for w in F.KINDS if w != kind]
    for which in others:
        one(which)
    before, before_others = c.launch_info(), {w: F.info(w, c) for w in others}
    ms0, n0 = c.kernel_time()
    one(kind)
    ms1, n1 = c.kernel_time()
    assert c.launch_info() == before and before and before[0]["kernel"].startswith("k_align")
    for w in others:
        assert F.info(w, c) == before_others[w] and [r["kernel"] for r in before_others[w]] == [F.KINDS[w].kernel % 2], w
    assert n1 == n0 + 1 and ms1 > ms0
    info = F.info(kind, c)
    assert [(r["kernel"], r["cols"], r["tasks"], r["band_max"]) for r in info] == [(F.KINDS[kind].kernel % 2, 2, n, 20)] and 0 < info[0]["slots"] <= n, info
    sset.close()


# ---- 7. no scratch arena ------------------------------------------------------------------------------------------------------

@section(BOTH)
def a_batch_the_arena_cannot_hold_is_filled_all_the_same(kind):
    """With the arena bounded to 1 MB gamdp_align_batch cannot place the direction words of one 50 kb call (4 MB at band 150) and refuses
    the batch with GAMDP_ENOMEM; a fill-only call needs no arena and returns what it returned without the bound."""
    c = ctx()
    want, _, _ = synth_batch(kind, c, 150)
    sset = gam.SequenceSet.synthetic(c, F.SYNTH_FIRST, F.SYNTH_PAIRS, F.SYNTH_LEN)
    tasks = F.synth_tasks(sset, 150)
    try:
        c.set_arena_bytes(1 << 20)
        res = (L.Result * F.SYNTH_PAIRS)()
        assert c.lib.gamdp_align_batch(c.handle, sset.handle, sset.handle, tasks, F.SYNTH_PAIRS, res, None) == L.ENOMEM
        rec, fp = F.outputs(kind, F.SYNTH_PAIRS)
        assert F.call(kind, c, sset, sset, tasks, F.SYNTH_PAIRS, rec, fp) == 0, c.last_error()
        assert [F.whole(r) for r in rec] == want
    finally:
        c.set_arena_bytes(0)
        sset.close()
