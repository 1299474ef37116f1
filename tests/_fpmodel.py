"""k_ops_fp's decomposition of the edit-string fingerprint (gam_ngs_amd/csrc/gamdp_ops_fp.hip) in plain Python: segments of
`segment_bytes`, one lane per `lane_bytes` of a segment, a lane's Horner sum four bytes at a time (or byte by byte where the string
begins or ends inside the lane), the lane table M^(lane_bytes * l), the segment factor by square-and-multiply, the masks of the bytes
outside the string -- in both directions.  tests/test_ops_fp_model_cpu.py holds it against the three-line definition; the GPU tests take
their lengths and patterns from here."""
import functools
import random

import numpy as np

MULT = 0x9E3779B1
MASK = 0xFFFFFFFF
SEGMENT_BYTES, LANE_BYTES = 4096, 64


def fp_def(codes):
    """F(empty) = 0, F(s . e) = F(s) * M + (e + 1) mod 2^32: the definition (include/gamdp.h, gamdp_ops_fingerprint)"""
    f = 0
    for e in codes:
        f = (f * MULT + e + 1) & MASK
    return f


def mpow(b, e):
    """b^e mod 2^32 by square-and-multiply, as the kernel's mpow"""
    r = 1
    while e:
        if e & 1:
            r = (r * b) & MASK
        b = (b * b) & MASK
        e >>= 1
    return r


def lane_poly(chunk, lo, hi, forward):
    """A lane's share of its `len(chunk)` bytes (zero-filled where nothing was loaded): v_q = byte + 1 for lo <= q < hi, 0 otherwise;
    sum v_q M^q, or (forward) sum v_q M^(n - 1 - q).  All bytes inside the string: four at a time, the four "+ 1" as one constant."""
    n = len(chunk)
    m2, m3 = (MULT * MULT) & MASK, (MULT * MULT * MULT) & MASK
    m4, k4 = (m2 * m2) & MASK, (1 + MULT + m2 + m3) & MASK
    h = 0
    if lo == 0 and hi == n:
        words = [chunk[4 * k:4 * k + 4] for k in range(n // 4)]
        for b0, b1, b2, b3 in (words if forward else reversed(words)):
            part = (b0 * m3 + b1 * m2 + b2 * MULT + b3) if forward else (b0 + b1 * MULT + b2 * m2 + b3 * m3)
            h = (h * m4 + part + k4) & MASK
    else:
        for k in range(n):
            q = k if forward else n - 1 - k
            h = (h * MULT + (chunk[q] + 1 if lo <= q < hi else 0)) & MASK
    return h


def full_lanes_poly(lanes, forward):
    """lane_poly's four-bytes-at-a-time branch for many lanes at once: lanes is a (k, lane_bytes) uint8 array of lanes that lie
    wholly inside the string; uint32 arithmetic wraps mod 2^32"""
    m1, m2, m3, m4 = (np.uint32(pow(MULT, k, 1 << 32)) for k in (1, 2, 3, 4))
    k4 = np.uint32((1 + MULT + MULT ** 2 + MULT ** 3) & MASK)
    w = lanes.astype(np.uint32).reshape(lanes.shape[0], -1, 4)
    h = np.zeros(lanes.shape[0], np.uint32)
    order = range(w.shape[1]) if forward else range(w.shape[1] - 1, -1, -1)
    for k in order:
        b0, b1, b2, b3 = w[:, k, 0], w[:, k, 1], w[:, k, 2], w[:, k, 3]
        part = (b0 * m3 + b1 * m2 + b2 * m1 + b3) if forward else (b0 + b1 * m1 + b2 * m2 + b3 * m3)
        h = h * m4 + part + k4
    return h


def model(room, length, lead, forward, segment_bytes=SEGMENT_BYTES, lane_bytes=LANE_BYTES):
    """The fingerprint as the launch computes it.  room: the bytes at the task's offset; the string is room[lead:length] -- lead == 0
    and traceback order (forward False), or forward order with length a multiple of lane_bytes (forward True)."""
    lanes_per_seg = segment_bytes // lane_bytes
    assert segment_bytes == lanes_per_seg * lane_bytes and lane_bytes % 16 == 0 and (not forward or length % lane_bytes == 0)
    assert len(room) % 16 == 0 and len(room) >= length, "the room ends on a multiple of 16 at or after the string"
    table = [mpow(mpow(MULT, lane_bytes), l) for l in range(lanes_per_seg)]
    m_seg = mpow(MULT, segment_bytes)
    fp = 0
    n_segs = (length + segment_bytes - 1) // segment_bytes
    for s in range(n_segs):
        seg_at = s * segment_bytes
        m = min(length - seg_at, segment_bytes)
        # 16 bytes at a time, only the loads that begin inside the string: what lies behind the last of them is never read
        loaded = min(len(room), (length + 15) // 16 * 16) - seg_at
        seg = np.zeros(segment_bytes, np.uint8)
        seg[:min(loaded, segment_bytes)] = np.frombuffer(room, np.uint8, min(loaded, segment_bytes), seg_at)
        seg = seg.reshape(lanes_per_seg, lane_bytes)
        lo = [(0 if lead <= seg_at + l * lane_bytes else min(lead - seg_at - l * lane_bytes, lane_bytes)) if forward else 0 for l in range(lanes_per_seg)]
        hi = [max(0, min(length - seg_at - l * lane_bytes, lane_bytes)) for l in range(lanes_per_seg)]
        full = [l for l in range(lanes_per_seg) if lo[l] == 0 and hi[l] == lane_bytes]
        share = dict(zip(full, (int(v) for v in full_lanes_poly(seg[full], forward)))) if full else {}
        total = 0
        for lane in range(lanes_per_seg):
            if lo[lane] < hi[lane]:
                if lane not in share:   # the string begins or ends inside this lane
                    share[lane] = lane_poly(bytes(seg[lane]), lo[lane], hi[lane], forward)
                k = (m // lane_bytes - 1 - lane) if forward else lane
                assert 0 <= k < lanes_per_seg
                total = (total + share[lane] * table[k]) & MASK
        scale = mpow(mpow(MULT, lane_bytes), (length - seg_at - m) // lane_bytes) if forward else mpow(m_seg, s)
        fp = (fp + total * scale) & MASK
    return fp


def model_traceback_order(r, **kw):
    """r: a string as the alignment kernels leave it (r[k] = s[len - 1 - k]) in a room rounded up to 16 bytes of anything"""
    room = bytes(r) + bytes([0xEE]) * (-len(r) % 16)
    return model(room, len(r), 0, False, **kw)


def model_forward_order(s, lane_bytes=LANE_BYTES, **kw):
    """s: a string in forward order, staged so that it ends where a lane ends"""
    lead = -len(s) % lane_bytes
    return model(bytes(lead) + bytes(s), lead + len(s), lead, True, lane_bytes=lane_bytes, **kw)


def boundary_lengths(segment_bytes=SEGMENT_BYTES, lane_bytes=LANE_BYTES, segments=3):
    """0, 1, and every length within +-1 of a multiple of 16, of lane_bytes and of segment_bytes, up to `segments` segments + 1"""
    top = segments * segment_bytes + 1
    out = {0, 1}
    for step in (16, lane_bytes, segment_bytes):
        for k in range(0, top + step, step):
            out.update(n for n in (k - 1, k, k + 1) if 0 <= n <= top)
    return sorted(out)


PATTERNS = ("ops", "bytes", "zeros", "ones")


def pattern(kind, n, rng):
    if kind == "ops":
        return bytes(rng.randbytes(n).translate(bytes(b & 3 for b in range(256))))
    if kind == "bytes":
        return rng.randbytes(n)
    return bytes([0 if kind == "zeros" else 255]) * n


@functools.lru_cache(maxsize=None)
def strings(segment_bytes=SEGMENT_BYTES, lane_bytes=LANE_BYTES, seed=20261020):
    """Every boundary length, the four patterns dealt over them in turn and all four at the lengths around a segment's end; computed
    once and shared (a tuple of bytes)."""
    rng = random.Random(seed)
    out = []
    for i, n in enumerate(boundary_lengths(segment_bytes, lane_bytes)):
        near_seg = min(n % segment_bytes, -n % segment_bytes) <= 1
        for kind in (PATTERNS if near_seg else (PATTERNS[i % 4],)):
            out.append(pattern(kind, n, rng))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def definition_of_strings(segment_bytes=SEGMENT_BYTES, lane_bytes=LANE_BYTES):
    """fp_def of every string of strings(), computed once"""
    return tuple(fp_def(s) for s in strings(segment_bytes, lane_bytes))
