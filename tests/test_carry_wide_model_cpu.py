"""A carry fill that keeps three anti-diagonals instead of the band matrix, as the plain-Python model tests/_carrywmodel.py -- the
skewed sweep over the live cells only, the three-slab ring, every entry tagged with the (step, row) that wrote it and every read
checked against the tag it expects -- pinned to the reference's recorded output: every golden L0 case, key by key, and the
fingerprint of the recorded edit string.  The ring of a call is sized by gamdp_task_live_columns, so it wraps: what is checked is
that the function's value is enough, and (the last test) not more than enough."""
import pytest

import _carrywmodel as W
import _golden
from gam_ngs_amd import api

MULT = 0x9E3779B1


def fp_py(codes):
    f = 0
    for e in codes:
        f = (f * MULT + e + 1) & 0xFFFFFFFF
    return f


def _args(cs):
    return (cs["a"], cs["b"], cs["band"], cs["begin_a"], cs["end_a"], cs["begin_b"], cs["end_b"], cs["fs"], cs["fe"])


def _live(cs):
    return api.task_live_columns(len(cs["a"]), len(cs["b"]), cs["band"], cs["begin_a"], cs["end_a"], cs["begin_b"], cs["end_b"], cs["fs"], cs["fe"])


def test_the_model_gives_the_recorded_result_and_fingerprint_on_every_golden_l0_case_with_a_ring_of_the_live_width():
    cases = _golden.l0_cases()
    assert len(cases) == 673
    bad, wrapped, statuses = [], 0, set()
    for name, cs, e in cases:
        M = _live(cs)
        ring = W.Ring(max(1, M))
        stats = {}
        got, fp = W.find_result(*_args(cs), ring=ring, M=max(1, M), stats=stats)
        want_fp = fp_py("ABMX".index(ch) for ch in e["ops"]) if e["status"] == W.OK else 0
        if got != _golden.expect_key(e) or fp != want_fp:
            bad.append((name, got, _golden.expect_key(e), fp, want_fp))
        if stats:
            assert stats["M"] == W.live_columns(len(cs["a"]), cs["band"], cs["begin_a"], stats["X"]) or M == 0, name   # the library's closed form is the model's
            assert stats["steps"] <= 2 * stats["X"] + M, (name, stats)   # no step without a live cell to speak of
        wrapped += ring.wraps > 0
        statuses.add(e["status"])
    assert not bad, (len(bad), bad[:3])
    assert statuses >= {W.OK, W.EMPTY, W.OUT_OF_RANGE}
    assert wrapped > 100, wrapped   # rows beyond the ring's length: the entries of a slab were reused


def test_a_slot_handed_from_call_to_call_never_shows_the_call_before():
    """one Ring for many calls, as a workgroup's slot: a read that met an entry of an earlier call would fail on its tag"""
    cases = _golden.l0_cases()[::5]
    cap = max(max(1, _live(cs)) for _, cs, _ in cases)
    ring = W.Ring(cap)
    for name, cs, e in cases:
        got, _ = W.find_result(*_args(cs), ring=ring, M=max(1, _live(cs)))
        assert got == _golden.expect_key(e), name
    assert ring.task > 100 and ring.reads > 100000


def test_a_ring_one_entry_short_is_caught():
    """a band wider than a: one step holds a cell of every one of |a| rows, as many as the widest row has live cells -- the ring of
    gamdp_task_live_columns entries is exactly enough, and the model notices one fewer"""
    import _carrymodel as M0
    a = b = b"ACGTTGCAAT" * 2
    args = (a, b, 40, 0, 19, 0, 19, False, False)
    M = api.task_live_columns(20, 20, 40, 0, 19, 0, 19)
    assert M == 20
    stats = {}
    got, _ = W.find_result(*args, M=M, stats=stats)
    assert got == M0.find_result(*args) and got[0] == W.OK and stats["rows_max"] == M
    with pytest.raises(AssertionError):
        W.find_result(*args, M=M - 1)
