"""gamdp_carry_batch (k_carry, gam_ngs_amd/csrc/gamdp_carry.hip): the whole result of find_alignment from a fill alone.

tests/test_gpu_score_batch.py taken section by section -- its generators, its bands, its min_ok caps (they hold for the oracle alone: that
file asserts them) -- with the comparison widened from (score, end cell, status, cells) to every field: the key of the result (status,
begin, score, n_match, length, first and last match, homology) and cells equal the CPU oracle's, which tests/test_oracle_golden.py and
tests/test_oracle_vs_ref.py pin to the reference.  The tie-rich pairs of tests/test_gpu_tie_windows.py come on top: the step the
traceback takes from a cell (banded_smith_waterman.cc:229-308) is a tie rule, and it is what this kernel restates.  At the shapes the
packed kernels run, every field of every result is compared with gamdp_align_batch's, and a sample with the oracle.

Nothing here is built to fault: every input is a valid call, or one the library documents that it refuses on the host before any launch.
"""
import random
from concurrent.futures import ThreadPoolExecutor

import pytest

import _cases
import _golden
import _mixed
import _oracle as O
import _views as V
import test_gpu_score_batch as S      # the generators and bands of the score tests
import test_gpu_tie_windows as W      # the tie-rich windowed and forced pairs, and what the oracle says about them
from _gpu import ctx
import gam_ngs_amd as gam
from gam_ngs_amd import api
from gam_ngs_amd import lib as L

pytestmark = pytest.mark.gpu

FIELDS = tuple(f for f, _ in L.Result._fields_ if f != "pad_")


def whole(r):
    """every field of a gamdp_result"""
    return tuple(getattr(r, f) for f in FIELDS)


def got_of(r):
    """(key, cells) of a MyAlignment / gamdp_result / oracle result"""
    return (tuple(r.key()), r.cells)


def oracle_wants(cases):
    """cases on code bytes -> [(key, cells)] of the oracle"""
    def one(cs):
        o, _ = O.oracle_align(cs["a"], cs["b"], cs["band"], cs["begin_a"], cs["end_a"], cs["begin_b"], cs["end_b"], cs["fs"], cs["fe"], want_ops=False)
        return got_of(o)
    with ThreadPoolExecutor(16) as ex:   # (the oracle's C code runs outside the GIL)
        return list(ex.map(one, cases))


def run_results(c, cases, ascii=False):
    """One gamdp_carry_batch call over cases that each bring their own pair of sequences"""
    seqs = []
    for cs in cases:
        seqs += [cs["a"], cs["b"]]
    sset = gam.SequenceSet(c, seqs, ascii=ascii)
    calls = [(sset.contig(2 * i), cs["begin_a"], cs["end_a"], sset.contig(2 * i + 1), cs["begin_b"], cs["end_b"], cs["fs"], cs["fe"])
             for i, cs in enumerate(cases)]
    res = gam.BandedSmithWaterman(c).find_results(calls, bands=[cs["band"] for cs in cases])
    sset.close()
    assert all(r.ops is None for r in res)
    return [got_of(r) for r in res]


def check(cases, got, want, what):
    assert len(got) == len(want) == len(cases)
    bad = [(i, got[i], want[i]) for i in range(len(cases)) if got[i] != want[i]]
    assert not bad, (what, len(bad), [(dict(cases[i], a=len(cases[i]["a"]), b=len(cases[i]["b"])), g, w) for i, g, w in bad[:3]])


def check_against_oracle(cases, what, min_ok=0.0):
    """cases on code bytes; the calls the oracle declines (INVALID) must be INVALID here too, everything else equal"""
    got = run_results(ctx(), cases)
    want = oracle_wants(cases)
    check(cases, got, want, what)
    n_ok = sum(1 for w in want if w[0][0] == O.OK)
    assert n_ok >= min_ok * len(cases), (what, n_ok, len(cases))
    return got, want


# ---- 1. the reference's golden vectors ----------------------------------------------------------------------------------

def test_golden_l0_cases():
    cases, want = [], []
    for name, cs, e in _golden.l0_cases():
        cc = S.coded(cs)
        o, _ = O.oracle_align(cc["a"], cc["b"], cs["band"], cs["begin_a"], cs["end_a"], cs["begin_b"], cs["end_b"], cs["fs"], cs["fe"], want_ops=False)
        cases.append(cc)
        want.append((_golden.expect_key(e), o.cells))   # (the golden vectors record no cell count)
    assert len(cases) == 673
    check(cases, run_results(ctx(), cases), want, "golden l0")
    assert sum(1 for w in want if w[0][0] == O.OK and not w[0][8]) >= 5, "alignments without a MATCH"


def test_golden_adversarial_cases():
    specs = _golden.adversarial_cases()
    assert len(specs) == 48
    cases = [S.coded(cs) for _, cs, _ in specs]
    cells = [w[1] for w in oracle_wants(cases)]
    check(cases, run_results(ctx(), cases), [(_golden.expect_key(e), n) for (_, _, e), n in zip(specs, cells)], "golden adversarial")


# ---- 2. random cases against the oracle ---------------------------------------------------------------------------------

def test_random_small_cases():
    cases = [S.coded(cs) for cs in _cases.cases(20261019, 1500) + _cases.cases(7, 300, max_len=1200, bands=(0, 2, 31, 32, 63, 64, 100, 300, 543))]
    check_against_oracle(cases, "random", min_ok=0.5)


def test_windows_that_begin_beyond_a():
    check_against_oracle([S.coded(cs) for cs in _cases.beyond_cases(99, 600)], "beyond")


@pytest.mark.parametrize("band", [150, 512])
def test_window_cases_on_long_pairs(band):
    check_against_oracle([S.coded(cs) for cs in _cases.window_cases(3, band, count=40)], "windows", min_ok=0.5)


@pytest.mark.parametrize("band", [150, 512, 20])
def test_one_n_around_every_edge_of_the_window(band):
    cases = [dict(a=O.encode(a), b=O.encode(b), band=band, begin_a=ba, end_a=ea, begin_b=bb, end_b=eb, fs=False, fe=False)
             for a, b, ba, ea, bb, eb, _ in _cases.n_edge_cases(band)]
    check_against_oracle(cases, "n edges", min_ok=1.0)


def test_forced_starts_and_ends_around_the_gap_limit():
    cases = S.force_cases()
    _, want = check_against_oracle(cases, "force")
    assert sum(1 for w in want if w[0][0] == O.OK) > len(cases) // 3 and len({w[0][0] for w in want}) >= 2, "forced calls of both outcomes"


def test_matrices_of_1_2_16_17_rows():
    rng = random.Random(1617)
    cases = []
    for rows in (1, 2, 16, 17):
        for band in (0, 1, 5, 40, 150, 512):
            for fs, fe in ((False, False), (True, False), (False, True), (True, True)):
                a, b = _cases.related_pair(rng, 90)
                begin_a, begin_b = rng.choice((0, 1, band, 30)), rng.randint(0, 20)
                cases.append(S.coded(dict(a=a.encode(), b=b.encode(), band=band, begin_a=begin_a, end_a=rng.choice((len(a) - 1, begin_a + rows, begin_a)),
                                          begin_b=begin_b, end_b=begin_b + rows - 1, fs=fs, fe=fe)))
    _, want = check_against_oracle(cases, "few rows")
    assert {w[1] // (2 * cs["band"] + 1) for cs, w in zip(cases, want)} >= {1, 2, 16, 17}


# ---- 3. every instantiation at the bands where it takes over -----------------------------------------------------------

@pytest.mark.parametrize("band", S.EDGE_BANDS)
def test_every_instantiation_at_its_edges(band):
    c = ctx()
    cases = S.edge_cases(band)
    _, want = check_against_oracle(cases, "band %d" % band, min_ok=0.5)
    # the intended instantiation ran: its name from the host's launch, its column count as the wavefronts wrote it into their records
    info = c.carry_info()
    cols = S.cols_for(band)
    launched = sum(1 for w in want if w[0][0] == O.OK or w[1] > 0)   # (at most: the pre-checks settle some calls that sized a matrix)
    assert len(info) == 1 and info[0]["kernel"] == "k_carry<%d>" % cols and info[0]["cols"] == cols, info
    assert info[0]["band_max"] == band and 0 < info[0]["tasks"] <= launched and 0 < info[0]["slots"] <= info[0]["tasks"], info


def test_a_batch_of_all_edge_bands_takes_five_launches():
    c = ctx()
    cases = [cs for band in S.EDGE_BANDS for cs in S.edge_cases(band)[:6]]
    check_against_oracle(cases, "all bands")
    info = c.carry_info()
    assert [(r["kernel"], r["cols"]) for r in info] == [("k_carry<%d>" % k, k) for k in (2, 3, 5, 9, 17)], info
    assert [r["band_max"] for r in info] == [63, 95, 159, 287, 543], info


# ---- 4. views -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cell,band", S.VIEW_CELLS)
def test_views_equal_explicit_copies_equal_the_oracle(cell, band):
    c = ctx()
    cases = [cs for cs in S.view_cases() if cs["cell"] == cell]
    assert {tuple(cs["tag"]["kinds"]) for cs in cases} == set(V.KIND_PAIRS)   # the 16 rc / suffix combinations
    seqs = []
    for cs in cases:
        seqs += [cs["stored_a"], cs["stored_b"], cs["a"], cs["b"]]
    sset = gam.SequenceSet(c, seqs, ascii=False)
    calls = []
    for i, cs in enumerate(cases):
        calls.append((sset.contig(4 * i, *cs["va"]), cs["begin_a"], cs["end_a"], sset.contig(4 * i + 1, *cs["vb"]), cs["begin_b"], cs["end_b"], cs["fs"], cs["fe"]))
        calls.append((sset.contig(4 * i + 2), cs["begin_a"], cs["end_a"], sset.contig(4 * i + 3), cs["begin_b"], cs["end_b"], cs["fs"], cs["fe"]))
    res = [got_of(r) for r in gam.BandedSmithWaterman(c, band).find_results(calls)]
    sset.close()
    want = oracle_wants(cases)
    bad = [(cs["tag"], res[2 * i], res[2 * i + 1], want[i]) for i, cs in enumerate(cases) if not (res[2 * i] == res[2 * i + 1] == want[i])]
    assert not bad, (len(bad), bad[:3])
    assert sum(1 for w in want if w[0][0] == O.OK) >= 0.9 * len(cases)
    assert [r["cols"] for r in c.carry_info()] == [S.cols_for(band)]


# ---- 5. ties: the step rule on homopolymers, dinucleotide and tandem repeats, with windows, force flags and N ---------------

def check_ties(cases, want, band):
    got = run_results(ctx(), cases, ascii=True)
    assert len(got) == len(cases) == len(want)
    for cs, g, (o, _) in zip(cases, got, want):
        assert g == got_of(o), (W.what(cs), g, got_of(o))
    info = ctx().carry_info()
    assert [r["kernel"] for r in info] == ["k_carry<%d>" % S.cols_for(band)], info


@pytest.mark.parametrize("band", W.SCORE_BANDS)
def test_tie_rich_windows_by_band(band):
    check_ties(W.band_cases(band), W.wants("band", band), band)


@pytest.mark.parametrize("band", W.LONG_BANDS)
def test_tie_rich_long_pairs_with_partners(band):
    cases, want = W.long_cases(band), W.wants("long", band)
    assert {len(cs["a"]) for cs in cases} >= {6000, 20000}
    check_ties(cases, want, band)


# ---- 6. every field against gamdp_align_batch at the shapes the packed kernels run -------------------------------------------

def align_and_carry(c, sset, tasks, n):
    out = (L.Result * n)()
    assert c.lib.gamdp_align_batch(c.handle, sset.handle, sset.handle, tasks, n, out, None) == 0, c.last_error()
    info = c.launch_info()
    ca = (L.Result * n)()
    assert c.lib.gamdp_carry_batch(c.handle, sset.handle, sset.handle, tasks, n, ca) == 0, c.last_error()
    bad = [i for i in range(n) if whole(ca[i]) != whole(out[i])]
    assert not bad, (len(bad), bad[:5], FIELDS, [(whole(ca[i]), whole(out[i])) for i in bad[:3]])
    return out, ca, info


def test_mixed_batch_of_2048_calls_equals_align_batch_and_the_oracle():
    c = ctx()
    seqs, calls = _mixed.mixed_batch(20261019, 256, 8, band=150)
    assert len(calls) == 2048
    sset = gam.SequenceSet(c, seqs, ascii=False)
    tasks = (L.Task * len(calls))()
    _mixed.fill_tasks(tasks, calls)
    out, ca, _ = align_and_carry(c, sset, tasks, len(calls))
    sset.close()
    assert sum(1 for r in out if r.status == O.OK) > 1800
    sample = random.Random(5).sample(range(len(calls)), 32)
    cases = [dict(a=seqs[cl["a_id"]][cl["a_off"]:], b=seqs[cl["b_id"]], band=cl["band"], begin_a=cl["begin_a"], end_a=cl["end_a"], begin_b=cl["begin_b"],
                  end_b=cl["end_b"], fs=cl["fs"], fe=cl["fe"]) for cl in (calls[i] for i in sample)]
    check(cases, [got_of(ca[i]) for i in sample], oracle_wants(cases), "mixed sample")


_SYNTH = {}


def synth_batch(c, band):
    """64 synthetic 50 kb pairs at `band` through both calls, once per band -> (results of gamdp_carry_batch, launches of gamdp_align_batch)"""
    if band not in _SYNTH:
        sset = gam.SequenceSet.synthetic(c, S.SYNTH_FIRST, S.SYNTH_PAIRS, S.SYNTH_LEN)
        tasks = S.synth_tasks(sset, band)
        out, ca, info = align_and_carry(c, sset, tasks, S.SYNTH_PAIRS)
        sset.close()
        assert all(r.status == O.OK for r in out)
        _SYNTH[band] = ([whole(r) for r in ca], [got_of(r) for r in ca], info)
    return _SYNTH[band]


@pytest.mark.parametrize("band,packed", [(150, None), (512, "k_align_p<17,4>")])
def test_64_synthetic_50kb_pairs_equal_align_batch_and_the_oracle(band, packed):
    c = ctx()
    _, got, info = synth_batch(c, band)
    if packed:   # (band 512: the two-task packed kernel is what a batch of this shape runs)
        assert {r["kernel"] for r in info} == {packed}, info
    sample = random.Random(band).sample(range(S.SYNTH_PAIRS), 32)
    cases = []
    for k in sample:
        a, b = api.synth_pair(S.SYNTH_FIRST + k, S.SYNTH_LEN)
        cases.append(dict(a=a, b=b, band=band, begin_a=0, end_a=S.SYNTH_LEN - 1, begin_b=0, end_b=len(b) - 1, fs=False, fe=False))
    check(cases, [got[k] for k in sample], oracle_wants(cases), "synthetic band %d" % band)


# ---- 7. refusals, and what the context reports ----------------------------------------------------------------------------

def test_refusals_leave_the_context_usable():
    c = ctx()
    sset, seqs = S.small_set(c)
    n = 8
    out = (L.Result * n)()
    call = lambda tasks, cnt=n, s=sset: c.lib.gamdp_carry_batch(c.handle, s.handle, s.handle, tasks, cnt, out)
    good = S.plain_tasks(seqs, n)
    assert call(good) == 0, c.last_error()
    first = [whole(r) for r in out]
    assert all(r.status == O.OK and r.score > 0 and r.n_match > 0 and r.first_found and r.last_found for r in out)
    # a band above GAMDP_MAX_TUNED_BAND anywhere in the batch: the whole call, by name; then the same context again
    wide = S.plain_tasks(seqs, n)
    wide[5].band = 544
    assert call(wide) == L.ENOTSUP
    assert "gamdp_carry_batch" in c.last_error() and "task 5" in c.last_error() and "544" in c.last_error(), c.last_error()
    assert call(good) == 0 and [whole(r) for r in out] == first
    wide[5].band = 543
    assert call(wide) == 0, c.last_error()
    assert call(None, 0) == 0                                   # n == 0
    assert c.lib.gamdp_carry_batch(c.handle, sset.handle, sset.handle, good, 0, out) == 0
    bad_id = S.plain_tasks(seqs, n)
    bad_id[3].b_id = 8
    assert call(bad_id) == L.EINVAL
    assert call(None, 1) == L.EINVAL
    synth = gam.SequenceSet.synthetic(c, 1, 2, 500)
    rc_task = (L.Task * 1)()
    rc_task[0].a_id, rc_task[0].b_id, rc_task[0].band, rc_task[0].b_rc = 0, 1, 20, 1
    rc_task[0].end_a, rc_task[0].end_b = 499, synth.lengths[1] - 1
    assert call(rc_task, 1, synth) == L.EINVAL                  # reverse complement of a packed-only set
    rc_task[0].b_rc = 0
    assert call(rc_task, 1, synth) == 0 and out[0].status == O.OK
    assert call(good) == 0 and [whole(r) for r in out] == first
    synth.close()
    sset.close()


def test_launch_info_and_score_info_stay_and_kernel_time_grows():
    c = ctx()
    sset, seqs = S.small_set(c)
    n = 8
    tasks = S.plain_tasks(seqs, n)
    res = (L.Result * n)()
    assert c.lib.gamdp_align_batch(c.handle, sset.handle, sset.handle, tasks, n, res, None) == 0, c.last_error()
    sc = (L.ScoreResult * n)()
    assert c.lib.gamdp_score_batch(c.handle, sset.handle, sset.handle, tasks, n, sc) == 0, c.last_error()
    before, before_score = c.launch_info(), c.score_info()
    ms0, n0 = c.kernel_time()
    out = (L.Result * n)()
    assert c.lib.gamdp_carry_batch(c.handle, sset.handle, sset.handle, tasks, n, out) == 0, c.last_error()
    ms1, n1 = c.kernel_time()
    assert c.launch_info() == before and before and before[0]["kernel"].startswith("k_align")
    assert c.score_info() == before_score and [r["kernel"] for r in before_score] == ["k_score<2>"]
    assert n1 == n0 + 1 and ms1 > ms0
    assert [r["kernel"] for r in c.carry_info()] == ["k_carry<2>"]
    assert [whole(r) for r in out] == [whole(r) for r in res]
    sset.close()


# ---- 8. no scratch arena ------------------------------------------------------------------------------------------------------

def test_a_batch_the_arena_cannot_hold_is_carried_all_the_same():
    """With the arena bounded to 1 MB gamdp_align_batch cannot place the direction words of one 50 kb call (4 MB at band 150) and refuses
    the batch with GAMDP_ENOMEM; gamdp_carry_batch needs no arena and returns what it returned without the bound."""
    c = ctx()
    want, _, _ = synth_batch(c, 150)
    sset = gam.SequenceSet.synthetic(c, S.SYNTH_FIRST, S.SYNTH_PAIRS, S.SYNTH_LEN)
    tasks = S.synth_tasks(sset, 150)
    try:
        c.set_arena_bytes(1 << 20)
        res = (L.Result * S.SYNTH_PAIRS)()
        assert c.lib.gamdp_align_batch(c.handle, sset.handle, sset.handle, tasks, S.SYNTH_PAIRS, res, None) == L.ENOMEM
        ca = (L.Result * S.SYNTH_PAIRS)()
        assert c.lib.gamdp_carry_batch(c.handle, sset.handle, sset.handle, tasks, S.SYNTH_PAIRS, ca) == 0, c.last_error()
        assert [whole(r) for r in ca] == want
    finally:
        c.set_arena_bytes(0)
        sset.close()
