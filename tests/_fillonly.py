"""The kit of the fill-only calls' GPU tests -- gamdp_score_batch, gamdp_carry_batch, gamdp_carry_ops_batch (include/gamdp.h) -- and of
the tests that take one of them as a second opinion: the case generators, the end-cell rule, the fingerprint's definition, one table of
what the three calls differ in, and run / oracle_wants / check / check_against_oracle / align_and on top of it.  No test collects from here.

Expected values come from the reference's golden vectors (tests/golden) and from the CPU oracle, never from the library.  Of a score
they are status, score and cells as they are and the end cell from the expected alignment and its edit string --
    end_a = begin_a + #MATCH + #MISMATCH + #GAP_B - 1,   end_b = begin_b + #MATCH + #MISMATCH + #GAP_A - 1
(the rule itself is checked on the CPU against the golden vectors, tests/test_fill_only_cabi.py); of a carry the key of the result
(status, begin, score, n_match, length, first and last match, homology) and cells; of a carry with fingerprints that and the
fingerprint of the oracle's edit string where the status is OK, 0 everywhere else.  Reference: BandedSmithWaterman::find_alignment,
lib/src/alignment/banded_smith_waterman.cc:80-215.
"""
import collections
import ctypes
import functools
import random
from concurrent.futures import ThreadPoolExecutor

import _cases
import _fpmodel
import _golden
import _oracle as O
import _views as V
from _gpu import ctx
import gam_ngs_amd as gam
from gam_ngs_amd import lib as L

EDGE_BANDS = (0, 1, 2, 63, 64, 95, 96, 159, 160, 287, 288, 543)   # where 2*band+1 crosses 64*C


def cols_for(band):
    """The smallest C of {2, 3, 5, 9, 17} with 2*band+1 <= 64*C (the issue's rule, restated here)."""
    return next(c for c in (2, 3, 5, 9, 17) if 2 * band + 1 <= 64 * c)


# ---- what is compared ---------------------------------------------------------------------------------------------------------

def end_cell(begin_a, begin_b, ops):
    m = ops.count("M") + ops.count("X")
    return begin_a + m + ops.count("B") - 1, begin_b + m + ops.count("A") - 1


def want_of(o, ops):
    """(score, end_a, end_b, status, cells) from an oracle result and its edit string"""
    if o.status != O.OK:
        return (0, 0, 0, o.status, o.cells)
    assert ops, "an alignment without an edit string has no end cell"
    return (o.score,) + end_cell(o.begin_a, o.begin_b, ops) + (O.OK, o.cells)


FIELDS = tuple(f for f, _ in L.Result._fields_ if f != "pad_")


def whole(r):
    """every field of a gamdp_result (FIELDS) or a gamdp_score_result"""
    return tuple(getattr(r, f) for f, _ in r._fields_ if f != "pad_")


def got_of(r):
    """(key, cells) of a MyAlignment / gamdp_result / oracle result"""
    return (tuple(r.key()), r.cells)


def fp_of(ops):
    """the definition, of an edit string over O.OPS"""
    return _fpmodel.fp_def(O.OPS.index(ch) for ch in ops)


def score_of(r):
    """(score, end_a, end_b, status, cells) of what find_scores returns for a call, or of a gamdp_score_result"""
    return tuple(r) if isinstance(r, tuple) else (r.score, r.end_a, r.end_b, r.status, r.cells)


# One row per call.  method: of BandedSmithWaterman; symbol, struct: the C call and its result; info: the Context getter of its launch
# log; kernel: the names the host's family tables give its instantiations (gamdp_host.cpp: score_family, carry_family,
# carry_ops_family); with_fp: a fingerprint per call comes back beside the results; needs_ops: the wanted tuple takes the edit string;
# got(result, fingerprint or None) and want(oracle result, edit string or None) -> the tuple that is compared; versus_align(record) ->
# what must equal gamdp_align_batch's result of the same task.
Kind = collections.namedtuple("Kind", "method symbol struct info kernel with_fp needs_ops got want versus_align")
KINDS = {
    "score": Kind("find_scores", "gamdp_score_batch", L.ScoreResult, "score_info", "k_score<%d>", False, True,
                  lambda r, fp: score_of(r), want_of, lambda r: (r.score, r.status, r.cells)),
    "carry": Kind("find_results", "gamdp_carry_batch", L.Result, "carry_info", "k_carry<%d>", False, False,
                  lambda r, fp: got_of(r), lambda o, ops: got_of(o), whole),
    "carry_ops": Kind("find_results_with_ops_fingerprints", "gamdp_carry_ops_batch", L.Result, "carry_ops_info", "k_carry_f<%d>", True, True,
                      lambda r, fp: (got_of(r), fp), lambda o, ops: (got_of(o), fp_of(ops) if o.status == O.OK else 0), whole),
}


def info(kind, c):
    """the launches of the kind's last call on the context"""
    return getattr(c, KINDS[kind].info)()


def call(kind, c, sa, sb, tasks, n, out, fp=None):
    """the kind's C call as it is; fp: the fingerprint array of a call that has one (None is passed on: the call refuses it)"""
    k = KINDS[kind]
    return getattr(c.lib, k.symbol)(c.handle, sa.handle, sb.handle, tasks, n, out, *([fp] if k.with_fp else []))


def outputs(kind, n):
    """(result array, fingerprint array or None) for n tasks"""
    k = KINDS[kind]
    return (k.struct * n)(), ((ctypes.c_uint32 * n)() if k.with_fp else None)


def run_calls(kind, c, calls, band=None, bands=None):
    """One call of the kind's BandedSmithWaterman method -> the compared tuple of every call"""
    k = KINDS[kind]
    bsw = gam.BandedSmithWaterman(c) if band is None else gam.BandedSmithWaterman(c, band)
    res = getattr(bsw, k.method)(calls, bands=bands)
    res, fps = res if k.with_fp else (res, [None] * len(res))
    assert len(fps) == len(res) == len(calls)
    if k.struct is L.Result:
        assert all(r.ops is None for r in res)
    return [k.got(r, f) for r, f in zip(res, fps)]


def run(kind, c, cases, ascii=False):
    """One call of the kind over cases that each bring their own pair of sequences"""
    seqs = []
    for cs in cases:
        seqs += [cs["a"], cs["b"]]
    sset = gam.SequenceSet(c, seqs, ascii=ascii)
    calls = [(sset.contig(2 * i), cs["begin_a"], cs["end_a"], sset.contig(2 * i + 1), cs["begin_b"], cs["end_b"], cs["fs"], cs["fe"])
             for i, cs in enumerate(cases)]
    got = run_calls(kind, c, calls, bands=[cs["band"] for cs in cases])
    sset.close()
    return got


def oracle_answers(cases, want_ops=True):
    """cases on code bytes -> [(oracle result, edit string or None)]; a call the oracle declines (undefined behaviour in the reference)
    has status INVALID"""
    def one(cs):
        return O.oracle_align(cs["a"], cs["b"], cs["band"], cs["begin_a"], cs["end_a"], cs["begin_b"], cs["end_b"], cs["fs"], cs["fe"], want_ops=want_ops)
    with ThreadPoolExecutor(16) as ex:   # (the oracle's C code runs outside the GIL)
        return list(ex.map(one, cases))


def wants_of(kind, answers):
    return [KINDS[kind].want(o, ops) for o, ops in answers]


def oracle_wants(kind, cases):
    """cases on code bytes -> the wanted tuple of every case"""
    return wants_of(kind, oracle_answers(cases, KINDS[kind].needs_ops))


def check(cases, got, want, what):
    assert len(got) == len(want) == len(cases)
    bad = [(i, got[i], want[i]) for i in range(len(cases)) if tuple(got[i]) != tuple(want[i])]
    assert not bad, (what, len(bad), [(dict(cases[i], a=len(cases[i]["a"]), b=len(cases[i]["b"])), g, w) for i, g, w in bad[:3]])


def check_against_oracle(kind, cases, what, min_ok=0.0):
    """cases on code bytes; the calls the oracle declines (INVALID) must be INVALID here too, everything else equal
    -> [(oracle result, edit string or None)]"""
    got = run(kind, ctx(), cases)
    answers = oracle_answers(cases, KINDS[kind].needs_ops)
    check(cases, got, wants_of(kind, answers), what)
    n_ok = sum(1 for o, _ in answers if o.status == O.OK)
    assert n_ok >= min_ok * len(cases), (what, n_ok, len(cases))
    return answers


def align_and(kind, c, sset, tasks, n):
    """gamdp_align_batch, then the kind's call on the same tasks: what the kind shares with a gamdp_result equal, task by task
    -> gamdp_align_batch's results, the kind's results, its fingerprints or None, gamdp_align_batch's launches"""
    k = KINDS[kind]
    out = (L.Result * n)()
    assert c.lib.gamdp_align_batch(c.handle, sset.handle, sset.handle, tasks, n, out, None) == 0, c.last_error()
    launches = c.launch_info()
    rec, fp = outputs(kind, n)
    assert call(kind, c, sset, sset, tasks, n, rec, fp) == 0, c.last_error()
    bad = [i for i in range(n) if k.versus_align(rec[i]) != k.versus_align(out[i])]
    assert not bad, (len(bad), bad[:5], FIELDS, [(k.versus_align(rec[i]), k.versus_align(out[i])) for i in bad[:3]])
    return out, rec, fp, launches


class GoldenAnswer:
    """a golden expectation and the oracle's cell count (the golden vectors record none) in the shape of an oracle result"""

    def __init__(self, e, cells):
        self.e, self.cells = e, cells
        self.status, self.score, self.begin_a, self.begin_b = e["status"], e["score"], e["begin_a"], e["begin_b"]

    def key(self):
        return _golden.expect_key(self.e)


def golden_l0(kind):
    """the reference's small golden vectors -> cases on code bytes, the wanted tuples from the reference's own results and edit strings"""
    cases, want = [], []
    for name, cs, e in _golden.l0_cases():
        cc = coded(cs)
        o, _ = O.oracle_align(cc["a"], cc["b"], cs["band"], cs["begin_a"], cs["end_a"], cs["begin_b"], cs["end_b"], cs["fs"], cs["fe"], want_ops=False)
        cases.append(cc)
        want.append(KINDS[kind].want(GoldenAnswer(e, o.cells), e["ops"]))
    assert len(cases) == 673
    return cases, want


# ---- the cases (seeded: the same in every file that takes them) -----------------------------------------------------------------

def coded(cs):
    return dict(cs, a=O.encode(cs["a"]), b=O.encode(cs["b"]))


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


VIEW_CELLS = (("gen2", 63), ("gen3", 95), ("gen5", 159), ("gen9", 287), ("gen17", 543))   # one band per instantiation


@functools.lru_cache(maxsize=1)
def view_cases():
    return [cs for cs in V.matrix_cases() if (cs["cell"], cs["band"]) in VIEW_CELLS]


SYNTH_PAIRS, SYNTH_LEN, SYNTH_FIRST = 64, 50000, 4242


def synth_tasks(sset, band):
    tasks = (L.Task * SYNTH_PAIRS)()
    for k in range(SYNTH_PAIRS):
        t = tasks[k]
        t.a_id, t.b_id, t.band = 2 * k, 2 * k + 1, band
        t.begin_a, t.end_a, t.begin_b, t.end_b = 0, SYNTH_LEN - 1, 0, sset.lengths[2 * k + 1] - 1
    return tasks


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
