"""gamdp_score_batch (k_score, gam_ngs_amd/csrc/gamdp_score.hip): score and end cell of find_alignment without the traceback.

Expected values come from the reference's golden vectors (tests/golden) and from the CPU oracle, never from the library: status, score
and cells as they are, the end cell from the expected alignment and its edit string --
    end_a = begin_a + #MATCH + #MISMATCH + #GAP_B - 1,   end_b = begin_b + #MATCH + #MISMATCH + #GAP_A - 1
(the rule itself is checked on the CPU against the golden vectors, tests/test_score_batch_cabi.py).  Reference:
BandedSmithWaterman::find_alignment, lib/src/alignment/banded_smith_waterman.cc:80-215.

Nothing here is built to fault: every input is a valid call, or one the library documents that it refuses on the host before any launch.
"""
import functools
import random
from concurrent.futures import ThreadPoolExecutor

import pytest

import _cases
import _golden
import _mixed
import _oracle as O
import _views as V
from _gpu import ctx
import gam_ngs_amd as gam
from gam_ngs_amd import api
from gam_ngs_amd import lib as L

pytestmark = pytest.mark.gpu

EDGE_BANDS = (0, 1, 2, 63, 64, 95, 96, 159, 160, 287, 288, 543)   # where 2*band+1 crosses 64*C


def cols_for(band):
    """The smallest C of {2, 3, 5, 9, 17} with 2*band+1 <= 64*C (the issue's rule, restated here)."""
    return next(c for c in (2, 3, 5, 9, 17) if 2 * band + 1 <= 64 * c)


def end_cell(begin_a, begin_b, ops):
    m = ops.count("M") + ops.count("X")
    return begin_a + m + ops.count("B") - 1, begin_b + m + ops.count("A") - 1


def want_of(o, ops):
    """(score, end_a, end_b, status, cells) from an oracle result and its edit string"""
    if o.status != O.OK:
        return (0, 0, 0, o.status, o.cells)
    assert ops, "an alignment without an edit string has no end cell"
    return (o.score,) + end_cell(o.begin_a, o.begin_b, ops) + (O.OK, o.cells)


def oracle_wants(cases):
    """cases on code bytes -> [want or None (the oracle declines: undefined behaviour in the reference)]"""
    def one(cs):
        o, ops = O.oracle_align(cs["a"], cs["b"], cs["band"], cs["begin_a"], cs["end_a"], cs["begin_b"], cs["end_b"], cs["fs"], cs["fe"], want_ops=True)
        return want_of(o, ops)
    with ThreadPoolExecutor(16) as ex:   # (the oracle's C code runs outside the GIL)
        return list(ex.map(one, cases))


def coded(cs):
    return dict(cs, a=O.encode(cs["a"]), b=O.encode(cs["b"]))


def run_scores(c, cases, ascii=False):
    """One gamdp_score_batch call over cases that each bring their own pair of sequences"""
    seqs = []
    for cs in cases:
        seqs += [cs["a"], cs["b"]]
    sset = gam.SequenceSet(c, seqs, ascii=ascii)
    calls = [(sset.contig(2 * i), cs["begin_a"], cs["end_a"], sset.contig(2 * i + 1), cs["begin_b"], cs["end_b"], cs["fs"], cs["fe"])
             for i, cs in enumerate(cases)]
    res = gam.BandedSmithWaterman(c).find_scores(calls, bands=[cs["band"] for cs in cases])
    sset.close()
    return res


def check(cases, got, want, what):
    assert len(got) == len(want) == len(cases)
    bad = [(i, got[i], want[i]) for i in range(len(cases)) if tuple(got[i]) != tuple(want[i])]
    assert not bad, (what, len(bad), [(dict(cases[i], a=len(cases[i]["a"]), b=len(cases[i]["b"])), g, w) for i, g, w in bad[:3]])


def check_against_oracle(cases, what, min_ok=0.0):
    """cases on code bytes; the calls the oracle declines (INVALID) must be INVALID here too, everything else equal"""
    got = run_scores(ctx(), cases)
    want = oracle_wants(cases)
    check(cases, got, want, what)
    n_ok = sum(1 for w in want if w[3] == O.OK)
    assert n_ok >= min_ok * len(cases), (what, n_ok, len(cases))
    return got, want


# ---- 1. the reference's golden vectors ----------------------------------------------------------------------------------

def test_golden_l0_cases():
    cases, want = [], []
    for name, cs, e in _golden.l0_cases():
        if "ops" not in e:
            continue
        cc = coded(cs)
        o, _ = O.oracle_align(cc["a"], cc["b"], cs["band"], cs["begin_a"], cs["end_a"], cs["begin_b"], cs["end_b"], cs["fs"], cs["fe"], want_ops=False)
        if e["status"] == O.OK:
            w = (e["score"],) + end_cell(e["begin_a"], e["begin_b"], e["ops"]) + (O.OK, o.cells)
        else:
            w = (0, 0, 0, e["status"], o.cells)
        cases.append(cc)
        want.append(w)
    assert len(cases) == 673
    check(cases, run_scores(ctx(), cases), want, "golden l0")


def test_golden_adversarial_cases():
    """3 - 20 kb pairs built against the packed kernels' range argument; the golden file holds the CRC32 of their edit strings: the
    oracle's string is taken once it matches that CRC."""
    specs = _golden.adversarial_cases()
    cases = [coded(cs) for _, cs, _ in specs]

    def one(k):
        cs, e = cases[k], specs[k][2]
        o, ops = O.oracle_align(cs["a"], cs["b"], cs["band"], cs["begin_a"], cs["end_a"], cs["begin_b"], cs["end_b"], False, False, want_ops=True)
        assert tuple(o.key()) == _golden.expect_key(e), specs[k][0]
        _golden.check_ops(e, ops)
        return (e["score"],) + end_cell(e["begin_a"], e["begin_b"], ops) + (e["status"], o.cells) if e["status"] == O.OK else (0, 0, 0, e["status"], o.cells)
    with ThreadPoolExecutor(16) as ex:
        want = list(ex.map(one, range(len(cases))))
    check(cases, run_scores(ctx(), cases), want, "golden adversarial")


# ---- 2. random cases against the oracle ---------------------------------------------------------------------------------

def test_random_small_cases():
    cases = [coded(cs) for cs in _cases.cases(20261019, 1500) + _cases.cases(7, 300, max_len=1200, bands=(0, 2, 31, 32, 63, 64, 100, 300, 543))]
    check_against_oracle(cases, "random", min_ok=0.5)


def test_windows_that_begin_beyond_a():
    check_against_oracle([coded(cs) for cs in _cases.beyond_cases(99, 600)], "beyond")


@pytest.mark.parametrize("band", [150, 512])
def test_window_cases_on_long_pairs(band):
    check_against_oracle([coded(cs) for cs in _cases.window_cases(3, band, count=40)], "windows", min_ok=0.5)


@pytest.mark.parametrize("band", [150, 512, 20])
def test_one_n_around_every_edge_of_the_window(band):
    cases = [dict(a=O.encode(a), b=O.encode(b), band=band, begin_a=ba, end_a=ea, begin_b=bb, end_b=eb, fs=False, fe=False)
             for a, b, ba, ea, bb, eb, _ in _cases.n_edge_cases(band)]
    check_against_oracle(cases, "n edges", min_ok=1.0)


def force_cases():
    """force_start / force_end with 9, 10, 11 unrelated bases in front of / behind the homology, on either sequence, around
    FORCE_MAXGAP_LEN = 10; windows that begin inside the band's left triangle (pos == 0 in rows up to band - begin_a) included"""
    rng = random.Random(1011)
    out = []
    for t in (9, 10, 11):
        for band in (2, 12, 40, 150, 300):
            for begin_a in (0, 3, band):
                a, b = _cases.related_pair(rng, rng.randint(60, 400), 0.02 if rng.random() < 0.3 else 0.0)
                pa, pb, junk = "C" * begin_a, "", _cases.rand_seq(rng, t)
                for a2, b2 in ((junk + a, b), (a, junk + b)):
                    out.append(dict(a=pa + a2, b=pb + b2, band=band, begin_a=begin_a, end_a=len(pa + a2) - 1, begin_b=0, end_b=len(b2) - 1, fs=True, fe=False))
                for a2, b2 in ((a + junk, b), (a, b + junk)):
                    for fs in (False, True):
                        out.append(dict(a=pa + a2, b=b2, band=band, begin_a=begin_a, end_a=len(pa + a) - 1 + rng.choice((0, t, -3)), begin_b=0,
                                        end_b=len(b2) - 1, fs=fs, fe=True))
    return [coded(dict(cs, a=cs["a"].encode(), b=cs["b"].encode())) for cs in out]


def test_forced_starts_and_ends_around_the_gap_limit():
    cases = force_cases()
    _, want = check_against_oracle(cases, "force")
    assert sum(1 for w in want if w[3] == O.OK) > len(cases) // 3 and len({w[3] for w in want}) >= 2, "forced calls of both outcomes"


def test_matrices_of_1_2_16_17_rows():
    rng = random.Random(1617)
    cases = []
    for rows in (1, 2, 16, 17):
        for band in (0, 1, 5, 40, 150, 512):
            for fs, fe in ((False, False), (True, False), (False, True), (True, True)):
                a, b = _cases.related_pair(rng, 90)
                begin_a, begin_b = rng.choice((0, 1, band, 30)), rng.randint(0, 20)
                cases.append(coded(dict(a=a.encode(), b=b.encode(), band=band, begin_a=begin_a, end_a=rng.choice((len(a) - 1, begin_a + rows, begin_a)),
                                        begin_b=begin_b, end_b=begin_b + rows - 1, fs=fs, fe=fe)))
    _, want = check_against_oracle(cases, "few rows")
    assert {w[4] // (2 * cs["band"] + 1) for cs, w in zip(cases, want)} >= {1, 2, 16, 17}


# ---- 3. every instantiation at the bands where it takes over -----------------------------------------------------------

def edge_cases(band):
    rng = random.Random(4000 + band)
    out = []
    for k in range(24):
        n = rng.randint(40, 700)
        a, b = _cases.related_pair(rng, n, 0.0, div=rng.choice((0.0, 1.0, 2.0)))
        kind = k % 6
        begin_a = rng.randint(0, min(n // 3, 60))
        end_a = len(a) - 1
        if kind == 0 and band > 0:       # cells with pos <= 0
            begin_a = rng.randint(0, min(band - 1, n // 3))
        elif kind == 1:                  # end_a >= |a|
            end_a = len(a) + rng.randint(0, 2 * band + 5)
        elif kind == 2:                  # end_a < begin_a + band: the anti-diagonal starts in row 0
            end_a = begin_a + rng.randint(0, max(0, band - 1))
        elif kind == 3:                  # N runs at the window's start and end
            a = "N" * rng.randint(1, 9) + a[9:-9] + "N" * rng.randint(1, 9)
            b = "N" * rng.randint(1, 5) + b[5:]
            begin_a, end_a = 0, len(a) - 1
        elif kind == 4:                  # b outlasts a: rows bounded by |a| + band - begin_a, positions >= |a|
            b = b + _cases.rand_seq(rng, band + 30)
        begin_b = rng.randint(0, 8)
        out.append(dict(a=a.encode(), b=b.encode(), band=band, begin_a=begin_a, end_a=end_a, begin_b=begin_b, end_b=len(b) - 1,
                        fs=kind == 5 and k % 2 == 0, fe=kind == 5 and k % 2 == 1))
    return [coded(cs) for cs in out]


@pytest.mark.parametrize("band", EDGE_BANDS)
def test_every_instantiation_at_its_edges(band):
    c = ctx()
    cases = edge_cases(band)
    _, want = check_against_oracle(cases, "band %d" % band, min_ok=0.5)
    # the intended instantiation ran: its name from the host's launch, its column count as the wavefronts wrote it into their records
    info = c.score_info()
    cols = cols_for(band)
    launched = sum(1 for w in want if w[3] == O.OK or w[4] > 0)   # (at most: the pre-checks settle some calls that sized a matrix)
    assert len(info) == 1 and info[0]["kernel"] == "k_score<%d>" % cols and info[0]["cols"] == cols, info
    assert info[0]["band_max"] == band and 0 < info[0]["tasks"] <= launched and 0 < info[0]["slots"] <= info[0]["tasks"], info


def test_a_batch_of_all_edge_bands_takes_five_launches():
    c = ctx()
    cases = [cs for band in EDGE_BANDS for cs in edge_cases(band)[:6]]
    check_against_oracle(cases, "all bands")
    info = c.score_info()
    assert [(r["kernel"], r["cols"]) for r in info] == [("k_score<%d>" % k, k) for k in (2, 3, 5, 9, 17)], info
    assert [r["band_max"] for r in info] == [63, 95, 159, 287, 543], info


# ---- 4. views -----------------------------------------------------------------------------------------------------------

VIEW_CELLS = (("gen2", 63), ("gen3", 95), ("gen5", 159), ("gen9", 287), ("gen17", 543))   # one band per instantiation


@functools.lru_cache(maxsize=1)
def view_cases():
    return [cs for cs in V.matrix_cases() if (cs["cell"], cs["band"]) in VIEW_CELLS]


@pytest.mark.parametrize("cell,band", VIEW_CELLS)
def test_views_equal_explicit_copies_equal_the_oracle(cell, band):
    c = ctx()
    cases = [cs for cs in view_cases() if cs["cell"] == cell]
    assert {tuple(cs["tag"]["kinds"]) for cs in cases} == set(V.KIND_PAIRS)   # the 16 rc / suffix combinations
    seqs = []
    for cs in cases:
        seqs += [cs["stored_a"], cs["stored_b"], cs["a"], cs["b"]]
    sset = gam.SequenceSet(c, seqs, ascii=False)
    calls = []
    for i, cs in enumerate(cases):
        calls.append((sset.contig(4 * i, *cs["va"]), cs["begin_a"], cs["end_a"], sset.contig(4 * i + 1, *cs["vb"]), cs["begin_b"], cs["end_b"], cs["fs"], cs["fe"]))
        calls.append((sset.contig(4 * i + 2), cs["begin_a"], cs["end_a"], sset.contig(4 * i + 3), cs["begin_b"], cs["end_b"], cs["fs"], cs["fe"]))
    res = gam.BandedSmithWaterman(c, band).find_scores(calls)
    sset.close()
    want = oracle_wants(cases)
    bad = [(cs["tag"], res[2 * i], res[2 * i + 1], want[i]) for i, cs in enumerate(cases) if not (tuple(res[2 * i]) == tuple(res[2 * i + 1]) == tuple(want[i]))]
    assert not bad, (len(bad), bad[:3])
    assert sum(1 for w in want if w[3] == O.OK) >= 0.9 * len(cases)
    assert [r["cols"] for r in c.score_info()] == [cols_for(band)]


# ---- 5. cross-check with gamdp_align_batch at the shapes the packed kernels run ----------------------------------------

def align_and_score(c, sset, tasks, n):
    out = (L.Result * n)()
    assert c.lib.gamdp_align_batch(c.handle, sset.handle, sset.handle, tasks, n, out, None) == 0, c.last_error()
    info = c.launch_info()
    sc = (L.ScoreResult * n)()
    assert c.lib.gamdp_score_batch(c.handle, sset.handle, sset.handle, tasks, n, sc) == 0, c.last_error()
    bad = [i for i in range(n) if (sc[i].score, sc[i].status, sc[i].cells) != (out[i].score, out[i].status, out[i].cells)]
    assert not bad, (len(bad), bad[:5], [(sc[i].score, sc[i].status, sc[i].cells, out[i].score, out[i].status, out[i].cells) for i in bad[:3]])
    return out, sc, info


def test_mixed_batch_of_2048_calls_equals_align_batch_and_the_oracle():
    c = ctx()
    seqs, calls = _mixed.mixed_batch(20261019, 256, 8, band=150)
    assert len(calls) == 2048
    sset = gam.SequenceSet(c, seqs, ascii=False)
    tasks = (L.Task * len(calls))()
    _mixed.fill_tasks(tasks, calls)
    out, sc, _ = align_and_score(c, sset, tasks, len(calls))
    sset.close()
    assert sum(1 for r in out if r.status == O.OK) > 1800
    sample = random.Random(5).sample(range(len(calls)), 32)
    cases = [dict(a=seqs[cl["a_id"]][cl["a_off"]:], b=seqs[cl["b_id"]], band=cl["band"], begin_a=cl["begin_a"], end_a=cl["end_a"], begin_b=cl["begin_b"],
                  end_b=cl["end_b"], fs=cl["fs"], fe=cl["fe"]) for cl in (calls[i] for i in sample)]
    want = oracle_wants(cases)
    check(cases, [(sc[i].score, sc[i].end_a, sc[i].end_b, sc[i].status, sc[i].cells) for i in sample], want, "mixed sample")


SYNTH_PAIRS, SYNTH_LEN, SYNTH_FIRST = 64, 50000, 4242
_SYNTH = {}


def synth_batch(c, band):
    """64 synthetic 50 kb pairs at `band` through both calls, once per band -> (scores of gamdp_score_batch, launches of gamdp_align_batch)"""
    if band not in _SYNTH:
        sset = gam.SequenceSet.synthetic(c, SYNTH_FIRST, SYNTH_PAIRS, SYNTH_LEN)
        tasks = synth_tasks(sset, band)
        out, sc, info = align_and_score(c, sset, tasks, SYNTH_PAIRS)
        sset.close()
        assert all(r.status == O.OK for r in out)
        _SYNTH[band] = ([(r.score, r.end_a, r.end_b, r.status, r.cells) for r in sc], info)
    return _SYNTH[band]


def synth_tasks(sset, band):
    tasks = (L.Task * SYNTH_PAIRS)()
    for k in range(SYNTH_PAIRS):
        t = tasks[k]
        t.a_id, t.b_id, t.band = 2 * k, 2 * k + 1, band
        t.begin_a, t.end_a, t.begin_b, t.end_b = 0, SYNTH_LEN - 1, 0, sset.lengths[2 * k + 1] - 1
    return tasks


@pytest.mark.parametrize("band,packed", [(150, None), (512, "k_align_p<17,4>")])
def test_64_synthetic_50kb_pairs_equal_align_batch_and_the_oracle(band, packed):
    c = ctx()
    got, info = synth_batch(c, band)
    if packed:   # (band 512: the two-task packed kernel is what a batch of this shape runs)
        assert {r["kernel"] for r in info} == {packed}, info
    sample = random.Random(band).sample(range(SYNTH_PAIRS), 32)
    cases = []
    for k in sample:
        a, b = api.synth_pair(SYNTH_FIRST + k, SYNTH_LEN)
        cases.append(dict(a=a, b=b, band=band, begin_a=0, end_a=SYNTH_LEN - 1, begin_b=0, end_b=len(b) - 1, fs=False, fe=False))
    check(cases, [got[k] for k in sample], oracle_wants(cases), "synthetic band %d" % band)


# ---- 6. refusals, and what the context reports ----------------------------------------------------------------------------

def small_set(c):
    rng = random.Random(66)
    pairs = [_cases.related_pair(rng, 300) for _ in range(4)]
    seqs = [s.encode() for p in pairs for s in p]
    return gam.SequenceSet(c, seqs, ascii=True), seqs


def plain_tasks(seqs, n, band=20):
    tasks = (L.Task * n)()
    for k in range(n):
        t = tasks[k]
        t.a_id, t.b_id, t.band = 2 * (k % 4), 2 * (k % 4) + 1, band
        t.begin_a, t.end_a, t.begin_b, t.end_b = 0, len(seqs[2 * (k % 4)]) - 1, 0, len(seqs[2 * (k % 4) + 1]) - 1
    return tasks


def test_refusals_leave_the_context_usable():
    c = ctx()
    sset, seqs = small_set(c)
    n = 8
    out = (L.ScoreResult * n)()
    call = lambda tasks, cnt=n, s=sset: c.lib.gamdp_score_batch(c.handle, s.handle, s.handle, tasks, cnt, out)
    good = plain_tasks(seqs, n)
    assert call(good) == 0, c.last_error()
    first = [(r.score, r.end_a, r.end_b, r.status, r.cells) for r in out]
    assert all(r[3] == O.OK and r[0] > 0 for r in first)
    # a band above GAMDP_MAX_TUNED_BAND anywhere in the batch: the whole call, by name; then the same context again
    wide = plain_tasks(seqs, n)
    wide[5].band = 544
    assert call(wide) == L.ENOTSUP
    assert "task 5" in c.last_error() and "544" in c.last_error(), c.last_error()
    assert call(good) == 0 and [(r.score, r.end_a, r.end_b, r.status, r.cells) for r in out] == first
    wide[5].band = 543
    assert call(wide) == 0, c.last_error()
    assert call(None, 0) == 0                                   # n == 0
    assert c.lib.gamdp_score_batch(c.handle, sset.handle, sset.handle, good, 0, out) == 0
    bad_id = plain_tasks(seqs, n)
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
    assert call(good) == 0 and [(r.score, r.end_a, r.end_b, r.status, r.cells) for r in out] == first
    synth.close()
    sset.close()


def test_launch_info_stays_with_align_batch_and_kernel_time_grows():
    c = ctx()
    sset, seqs = small_set(c)
    n = 8
    tasks = plain_tasks(seqs, n)
    res = (L.Result * n)()
    assert c.lib.gamdp_align_batch(c.handle, sset.handle, sset.handle, tasks, n, res, None) == 0, c.last_error()
    before = c.launch_info()
    ms0, n0 = c.kernel_time()
    out = (L.ScoreResult * n)()
    assert c.lib.gamdp_score_batch(c.handle, sset.handle, sset.handle, tasks, n, out) == 0, c.last_error()
    ms1, n1 = c.kernel_time()
    assert c.launch_info() == before and before and before[0]["kernel"].startswith("k_align")
    assert n1 == n0 + 1 and ms1 > ms0
    assert [r["kernel"] for r in c.score_info()] == ["k_score<2>"]
    sset.close()


# ---- 7. no scratch arena ------------------------------------------------------------------------------------------------------

def test_a_batch_the_arena_cannot_hold_is_scored_all_the_same():
    """With the arena bounded to 1 MB gamdp_align_batch cannot place the direction words of one 50 kb call (4 MB at band 150) and refuses
    the batch with GAMDP_ENOMEM; gamdp_score_batch needs no arena and returns what it returned without the bound."""
    c = ctx()
    want, _ = synth_batch(c, 150)
    sset = gam.SequenceSet.synthetic(c, SYNTH_FIRST, SYNTH_PAIRS, SYNTH_LEN)
    tasks = synth_tasks(sset, 150)
    try:
        c.set_arena_bytes(1 << 20)
        res = (L.Result * SYNTH_PAIRS)()
        assert c.lib.gamdp_align_batch(c.handle, sset.handle, sset.handle, tasks, SYNTH_PAIRS, res, None) == L.ENOMEM
        sc = (L.ScoreResult * SYNTH_PAIRS)()
        assert c.lib.gamdp_score_batch(c.handle, sset.handle, sset.handle, tasks, SYNTH_PAIRS, sc) == 0, c.last_error()
        assert [(r.score, r.end_a, r.end_b, r.status, r.cells) for r in sc] == want
    finally:
        c.set_arena_bytes(0)
        sset.close()
