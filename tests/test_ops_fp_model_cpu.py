"""The decomposition k_ops_fp uses (tests/_fpmodel.py: segments, lanes, the lane table, the segment factor, the masks at a string's
ends, both directions) against the three-line definition of the fingerprint, on the CPU: every length within one of a multiple of
16, of a lane's bytes and of a segment's, up to three segments and one byte, over ops, arbitrary bytes, all 0 and all 255."""
import random

import pytest

import _fpmodel as F


def test_the_lengths_and_patterns():
    lens = F.boundary_lengths()
    assert lens[:5] == [0, 1, 15, 16, 17] and lens[-1] == 3 * F.SEGMENT_BYTES + 1
    for k in (F.LANE_BYTES, F.SEGMENT_BYTES, 2 * F.SEGMENT_BYTES, 3 * F.SEGMENT_BYTES, 5 * 16, 3 * F.LANE_BYTES + F.SEGMENT_BYTES):
        assert {k - 1, k, k + 1} <= set(lens)
    strings = F.strings()
    assert {len(s) for s in strings} == set(lens)
    assert any(s and set(s) <= {0, 1, 2, 3} and len(set(s)) == 4 for s in strings) and any(len(set(s)) > 200 for s in strings)
    for n in (F.SEGMENT_BYTES - 1, F.SEGMENT_BYTES, F.SEGMENT_BYTES + 1, 3 * F.SEGMENT_BYTES + 1):
        assert bytes(n) in strings and bytes([255]) * n in strings


def test_the_pieces_of_the_model():
    assert F.fp_def(b"") == 0 and F.fp_def([0]) == 1 and F.fp_def([255]) == 256 and F.fp_def([0, 0]) == (F.MULT + 1) & F.MASK
    assert F.mpow(F.MULT, 0) == 1 and F.mpow(F.MULT, 5) == pow(F.MULT, 5, 1 << 32) and F.mpow(F.mpow(F.MULT, 4096), 3) == pow(F.MULT, 12288, 1 << 32)
    rng = random.Random(1)
    chunk = rng.randbytes(64)
    for forward in (False, True):
        want = sum((b + 1) * pow(F.MULT, (63 - q) if forward else q, 1 << 32) for q, b in enumerate(chunk)) & F.MASK
        assert F.lane_poly(chunk, 0, 64, forward) == want                                  # four bytes at a time
        assert int(F.full_lanes_poly(F.np.frombuffer(chunk, F.np.uint8).reshape(1, 64), forward)[0]) == want
        for lo, hi in ((0, 63), (1, 64), (0, 1), (17, 40), (63, 64), (5, 5)):                     # byte by byte, masked
            want = sum((b + 1) * pow(F.MULT, (63 - q) if forward else q, 1 << 32) for q, b in enumerate(chunk) if lo <= q < hi) & F.MASK
            assert F.lane_poly(chunk, lo, hi, forward) == want, (forward, lo, hi)


@pytest.mark.parametrize("forward", [False, True], ids=["traceback_order", "forward_order"])
def test_the_model_equals_the_definition(forward):
    strings, want = F.strings(), F.definition_of_strings()
    assert len(strings) > 2300
    for s, w in zip(strings, want):
        got = F.model_forward_order(s) if forward else F.model_traceback_order(s[::-1])
        assert got == w, (forward, len(s), s[:8], got, w)


@pytest.mark.parametrize("segment_bytes,lane_bytes", [(1024, 16), (2048, 32), (8192, 128)])
def test_the_model_does_not_depend_on_the_constants(segment_bytes, lane_bytes):
    """other segment and lane sizes (a lane a multiple of 16 bytes, 64 lanes per segment): the same function"""
    rng = random.Random(segment_bytes)
    for n in (0, 1, lane_bytes - 1, lane_bytes + 1, segment_bytes - 1, segment_bytes, segment_bytes + 1, 2 * segment_bytes + lane_bytes + 5):
        for s in (rng.randbytes(n), bytes(n), bytes([255]) * n):
            assert F.model_traceback_order(s[::-1], segment_bytes=segment_bytes, lane_bytes=lane_bytes) == F.fp_def(s)
            assert F.model_forward_order(s, segment_bytes=segment_bytes, lane_bytes=lane_bytes) == F.fp_def(s)
