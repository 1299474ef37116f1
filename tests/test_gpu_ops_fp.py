"""Fingerprints of edit strings that stay on the device: gamdp_ops_fingerprint_batch (k_ops_fp<true> on strings a caller uploads -- the
kernel on its own) and gamdp_align_batch_fp (gamdp_align_batch's own strings, left where the walks wrote them, folded by
k_ops_fp<false>); gam_ngs_amd/csrc/gamdp_ops_fp.hip.

The fingerprints are held against the three-line definition (tests/_fpmodel.py: fp_def) of strings from three independent sources --
the reference's golden edit strings, the CPU oracle's, and the strings gamdp_align_batch delivers through gamdp_ops -- and against
gamdp_carry_ops_batch's; the results against the golden keys, the oracle and gamdp_align_batch field by field.  The boundary lengths
come from what gamdp_ctx_ops_fp_info reports (segment_bytes, lane_bytes), not from constants of this file.

Nothing here is built to fault: every input is a valid call, or one the library documents that it refuses on the host before any launch.
"""
import ctypes
import functools
import random

import pytest

import _cases
import _fpmodel as F
import _fillonly as S       # coded, cols_for, edge_cases, view_cases, small_set, plain_tasks, fp_of, whole, got_of
import _golden
import _oracle as O
from _gpu import ctx
import gam_ngs_amd as gam
from gam_ngs_amd import api
from gam_ngs_amd import lib as L

pytestmark = pytest.mark.gpu

fp_of, whole, got_of = S.fp_of, S.whole, S.got_of


def geometry(c):
    info = c.ops_fp_info()
    assert info["segment_bytes"] > 0 and info["lane_bytes"] > 0 and info["segment_bytes"] % info["lane_bytes"] == 0, info
    return info["segment_bytes"], info["lane_bytes"]


# ---- 1. the kernel on its own: gamdp_ops_fingerprint_batch against the definition ---------------------------------------------

def test_strings_of_every_boundary_length_equal_the_definition():
    c = ctx()
    seg, lane = geometry(c)
    strings, want = list(F.strings(seg, lane)), list(F.definition_of_strings(seg, lane))
    assert {len(s) for s in strings} == set(F.boundary_lengths(seg, lane)) and max(len(s) for s in strings) == 3 * seg + 1
    for at in (0, 7, len(strings) // 2, len(strings)):   # a few empty strings in between (back to back: every offset unaligned)
        strings.insert(at, b"")
        want.insert(at, 0)
    n_empty = sum(1 for s in strings if not s)
    got = api.ops_fingerprint_many(c, strings)
    bad = [(i, len(strings[i]), got[i], want[i]) for i in range(len(strings)) if got[i] != want[i]]
    assert not bad, (len(bad), bad[:5])
    info = c.ops_fp_info()
    assert info["kernel"] == "k_ops_fp<true>" and info["chunks"] == 1 and info["tasks"] == len(strings) - n_empty, info
    assert info["bytes"] == sum(len(s) for s in strings) and info["segments"] == sum(-(-len(s) // seg) for s in strings) and info["kernel_ms"] > 0, info
    # the same in many chunks, strings longer than a chunk included
    c.set_ops_chunk_bytes(seg)
    try:
        again = api.ops_fingerprint_many(c, strings)
        info = c.ops_fp_info()
    finally:
        c.set_ops_chunk_bytes(0)
    assert again == want
    assert info["chunks"] > len(strings) * seg // (4 * seg) > 1 and info["tasks"] == len(strings) - n_empty and info["bytes"] == sum(len(s) for s in strings), info
    assert api.ops_fingerprint_many(c, ["MMXAB", b"", [2, 2, 3, 0, 1]]) == [fp_of("MMXAB"), 0, fp_of("MMXAB")]
    assert c.ops_fp_info()["chunks"] == 1


# ---- 2. the reference's golden vectors, against the reference's own edit strings ---------------------------------------------

def case_calls(sset, cases, stride=2):
    return [(sset.contig(stride * i), cs["begin_a"], cs["end_a"], sset.contig(stride * i + 1), cs["begin_b"], cs["end_b"], cs["fs"], cs["fe"])
            for i, cs in enumerate(cases)]


def run_fp(c, cases):
    """One gamdp_align_batch_fp call over cases (on code bytes) that each bring their own pair of sequences -> results, fingerprints"""
    sset = gam.SequenceSet(c, [s for cs in cases for s in (cs["a"], cs["b"])], ascii=False)
    res, fps = gam.BandedSmithWaterman(c).find_alignments_with_ops_fingerprints(case_calls(sset, cases), bands=[cs["band"] for cs in cases])
    sset.close()
    assert all(r.ops is None for r in res) and len(fps) == len(res) == len(cases)
    return res, fps


def test_golden_l0_cases():
    c = ctx()
    specs = _golden.l0_cases()
    assert len(specs) == 673
    cases = [S.coded(cs) for _, cs, _ in specs]
    res, fps = run_fp(c, cases)
    n_ok = 0
    for (name, _, e), r, f in zip(specs, res, fps):
        assert tuple(r.key()) == _golden.expect_key(e), name
        assert f == (fp_of(e["ops"]) if e["status"] == O.OK else 0), (name, f)
        n_ok += e["status"] == O.OK
    assert n_ok > 500 and c.ops_fp_info()["kernel"] == "k_ops_fp<false>" and c.ops_fp_info()["tasks"] >= n_ok


# ---- 3. against the library's two other sources of the fingerprint; 5. chunking ------------------------------------------------

@functools.lru_cache(maxsize=1)
def small_batch():
    """the small case sets of the score / carry tests: every band at which an instantiation takes over, and the view matrix"""
    plain = [cs for band in S.EDGE_BANDS for cs in S.edge_cases(band)]
    views = list(S.view_cases())
    assert {S.cols_for(cs["band"]) for cs in plain} == {S.cols_for(cs["band"]) for cs in views} == {2, 3, 5, 9, 17}
    return plain, views


def small_batch_calls(c):
    plain, views = small_batch()
    seqs = [s for cs in plain for s in (cs["a"], cs["b"])]
    base = len(seqs)
    for cs in views:
        seqs += [cs["stored_a"], cs["stored_b"]]
    sset = gam.SequenceSet(c, seqs, ascii=False)
    calls = case_calls(sset, plain)
    for i, cs in enumerate(views):
        calls.append((sset.contig(base + 2 * i, *cs["va"]), cs["begin_a"], cs["end_a"], sset.contig(base + 2 * i + 1, *cs["vb"]), cs["begin_b"], cs["end_b"], cs["fs"], cs["fe"]))
    return sset, calls, [cs["band"] for cs in plain + views]


_SMALL = {}


def small_batch_reference(c):
    """gamdp_align_batch with edit strings and gamdp_carry_ops_batch over the small batch, once"""
    if not _SMALL:
        sset, calls, bands = small_batch_calls(c)
        bsw = gam.BandedSmithWaterman(c)
        _SMALL["align"] = bsw.find_alignments(calls, want_ops=True, bands=bands)
        _SMALL["carry"] = bsw.find_results_with_ops_fingerprints(calls, bands=bands)
        sset.close()
    return _SMALL["align"], _SMALL["carry"]


def run_small_batch(c):
    sset, calls, bands = small_batch_calls(c)
    res, fps = gam.BandedSmithWaterman(c).find_alignments_with_ops_fingerprints(calls, bands=bands)
    sset.close()
    return [(got_of(r), r.n_match, r.first_found, r.last_found) for r in res], fps


def check_small_batch(c, got, fps):
    al, (carry, carry_fps) = small_batch_reference(c)
    assert len(got) == len(fps) == len(al) == len(carry) > 300
    n_ok = 0
    for i, a in enumerate(al):
        assert got[i] == (got_of(a), a.n_match, a.first_found, a.last_found) and got[i][0] == got_of(carry[i]), (i, got[i], got_of(a))
        want = fp_of(a.ops) if a.status == O.OK else 0
        assert fps[i] == want == carry_fps[i], (i, fps[i], want, carry_fps[i])
        n_ok += a.status == O.OK
    assert n_ok >= 0.6 * len(al) and any(a.status != O.OK for a in al)
    assert len({a.ops for a in al if a.status == O.OK}) == len({f for a, f in zip(al, fps) if a.status == O.OK})   # distinct strings, distinct fingerprints


def test_small_batch_equals_align_batch_s_strings_and_carry_ops():
    c = ctx()
    got, fps = run_small_batch(c)
    info = c.ops_fp_info()
    check_small_batch(c, got, fps)
    assert info["kernel"] == "k_ops_fp<false>" and info["chunks"] == 1 and info["segments"] >= info["tasks"] > 0, info
    assert len(c.launch_info()) >= 5, c.launch_info()   # (the alignment launches of the chunk: an instantiation per column count at least)


def test_small_batch_in_chunks():
    c = ctx()
    plain, views = small_batch()
    caps = sorted(api.task_ops_cap(len(cs["a"]), len(cs["b"]), cs["band"], cs["begin_a"], cs["end_a"], cs["begin_b"], cs["end_b"], cs["fs"], cs["fe"]) for cs in plain)
    caps = [x for x in caps if x]
    whole_got, whole_fps = run_small_batch(c)
    n_tasks = len(whole_got)
    for budget, lo, hi in ((16, n_tasks, n_tasks), (3 * caps[len(caps) // 2], 8, n_tasks)):   # below any task's room; about three tasks' rooms
        assert budget == 16 < caps[0] or budget > caps[len(caps) // 2]
        c.set_ops_chunk_bytes(budget)
        try:
            got, fps = run_small_batch(c)
            info = c.ops_fp_info()
        finally:
            c.set_ops_chunk_bytes(0)
        assert (got, fps) == (whole_got, whole_fps), budget
        assert lo <= info["chunks"] <= hi, (budget, info)
    check_small_batch(c, whole_got, whole_fps)


# ---- 4. strings that cross segments; the wide kernel ------------------------------------------------------------------------------

def near_identical(rng, n, band):
    a = _cases.rand_seq(rng, n)
    b = _cases.mutate(rng, a, 0.01, 0.003, 0.003)
    return S.coded(dict(a=a.encode(), b=b.encode(), band=band, begin_a=0, end_a=len(a) - 1, begin_b=0, end_b=len(b) - 1, fs=False, fe=False))


def test_strings_that_cross_one_and_two_segments_and_the_wide_kernel():
    c = ctx()
    seg, _ = geometry(c)
    rng = random.Random(20261020)
    cases = [near_identical(rng, seg + n, 150) for n in (100, 140)] + [near_identical(rng, 2 * seg + n, 150) for n in (100, 180)]
    cases += [near_identical(rng, seg + 300, 512), near_identical(rng, 400, 600)]
    res, fps = run_fp(c, cases)
    info, launches = c.ops_fp_info(), c.launch_info()
    assert "k_align_w" in {r["kernel"] for r in launches}, launches
    for i, cs in enumerate(cases):
        o, ops = O.oracle_align(cs["a"], cs["b"], cs["band"], cs["begin_a"], cs["end_a"], cs["begin_b"], cs["end_b"], False, False, want_ops=True)
        assert o.status == O.OK and got_of(res[i]) == got_of(o), (i, got_of(res[i]), got_of(o))
        assert fps[i] == fp_of(ops), (i, len(ops), fps[i], fp_of(ops))
        assert len(ops) > (seg, seg, 2 * seg, 2 * seg, seg, 0)[i] and ("A" in ops or "B" in ops)
    assert info["segments"] == sum(-(-r.length() // seg) for r in res) == 2 + 2 + 3 + 3 + 2 + 1 and info["bytes"] == sum(r.length() for r in res), info


# ---- 6. statuses and refusals ---------------------------------------------------------------------------------------------------

def test_statuses_refusals_and_what_the_context_reports():
    c = ctx()
    sset, seqs = S.small_set(c)
    n = 8
    out, fp = (L.Result * n)(), (ctypes.c_uint32 * n)()
    call = lambda tasks, cnt=n, s=sset, f=fp, o=out: c.lib.gamdp_align_batch_fp(c.handle, s.handle, s.handle, tasks, cnt, o, f)  # noqa: E731
    good = S.plain_tasks(seqs, n)
    ms0, n0 = c.kernel_time()
    assert call(good) == 0, c.last_error()
    ms1, n1 = c.kernel_time()
    assert n1 >= n0 + 2 and ms1 > ms0                            # the alignment launch and k_ops_fp
    first, first_fp = [whole(r) for r in out], list(fp)
    assert all(r.status == O.OK and r.length > 0 for r in out) and all(first_fp) and first_fp[:4] == first_fp[4:]
    # ... exactly gamdp_align_batch's results and the fingerprints of its strings
    bsw = gam.BandedSmithWaterman(c, 20)
    al = bsw.find_alignments([(sset.contig(2 * (k % 4)), 0, len(seqs[2 * (k % 4)]) - 1, sset.contig(2 * (k % 4) + 1), 0, len(seqs[2 * (k % 4) + 1]) - 1) for k in range(n)], want_ops=True)
    assert [fp_of(a.ops) for a in al] == first_fp
    ref = (L.Result * n)()
    assert c.lib.gamdp_align_batch(c.handle, sset.handle, sset.handle, good, n, ref, None) == 0
    assert [whole(r) for r in ref] == first
    assert call(good) == 0 and c.launch_info() and c.launch_info()[0]["kernel"].startswith("k_align")
    # a batch mixing OK, EMPTY, OUT_OF_RANGE and INVALID calls: zeros in the right places, whatever the array held
    mixed = S.plain_tasks(seqs, n)
    mixed[1].begin_b, mixed[1].end_b = 9, 8                       # end_b < begin_b: EMPTY
    mixed[2].begin_b, mixed[2].end_b = len(seqs[5]) + 7, len(seqs[5]) + 9   # b.at(begin_b) throws: OUT_OF_RANGE
    mixed[4].b_off = len(seqs[1]) + 1                             # a suffix view beyond the sequence: INVALID
    mixed[6].begin_a = len(seqs[4]) + 20 + 5                      # the window begins beyond a: settled by the end-cell scan
    for k in range(n):
        fp[k] = 0xDEADBEEF
    assert call(mixed) == 0, c.last_error()
    assert (out[1].status, out[2].status, out[4].status) == (O.EMPTY, O.OUT_OF_RANGE, O.INVALID) and out[6].status != O.OK
    assert [fp[k] for k in (1, 2, 4, 6)] == [0, 0, 0, 0] and [fp[k] for k in (0, 3, 5, 7)] == [first_fp[k] for k in (0, 3, 5, 7)]
    ref2 = (L.Result * n)()
    assert c.lib.gamdp_align_batch(c.handle, sset.handle, sset.handle, mixed, n, ref2, None) == 0
    assert [whole(r) for r in out] == [whole(r) for r in ref2]
    # refusals, each followed by a good call on the same context
    assert call(None, 0) == 0 and call(good, 0) == 0              # n == 0
    assert call(good, f=None) == L.EINVAL and call(good, o=None) == L.EINVAL and call(None, 1) == L.EINVAL
    bad_id = S.plain_tasks(seqs, n)
    bad_id[3].b_id = 8
    assert call(bad_id) == L.EINVAL
    synth = gam.SequenceSet.synthetic(c, 1, 2, 500)
    rc_task = (L.Task * 1)()
    rc_task[0].a_id, rc_task[0].b_id, rc_task[0].band, rc_task[0].b_rc = 0, 1, 20, 1
    rc_task[0].end_a, rc_task[0].end_b = 499, synth.lengths[1] - 1
    assert call(rc_task, 1, synth) == L.EINVAL                   # reverse complement of a packed-only set
    rc_task[0].b_rc = 0
    assert call(rc_task, 1, synth) == 0 and out[0].status == O.OK and fp[0] != 0
    assert call(good) == 0 and [whole(r) for r in out] == first and list(fp) == first_fp
    # the stand-alone call's refusals
    off, ln, one = (ctypes.c_uint64 * 1)(0), (ctypes.c_uint64 * 1)(3), (ctypes.c_uint32 * 1)()
    assert c.lib.gamdp_ops_fingerprint_batch(c.handle, None, off, ln, 1, one) == L.EINVAL            # NULL ops with a string that is not empty
    assert c.lib.gamdp_ops_fingerprint_batch(c.handle, b"\x02\x02\x03", None, ln, 1, one) == L.EINVAL
    assert c.lib.gamdp_ops_fingerprint_batch(c.handle, None, None, None, 0, one) == 0                 # n == 0
    assert c.lib.gamdp_ops_fingerprint_batch(c.handle, b"\x02\x02\x03", off, ln, 1, one) == 0 and one[0] == fp_of("MMX")
    assert call(good) == 0 and list(fp) == first_fp
    synth.close()
    sset.close()
