"""The two-task band-512 kernel (k_align_p<17,4>) re-creates its directions in strips of DIFFERENT widths: 2 lanes around the band's
middle column, 4 and 8 lanes towards its outer lanes (PairStripTable, gam_ngs_amd/csrc/kernel_fill.inc), on the 16 boundary slots the
fill always stored.  Everything here is band 512 on N-free pairs of 2.5 - 6 kb (the packed range exists from ~2.3 kb on), every field
and every edit string against the oracle: paths on the first and last column of every strip, paths that drift from the 2-lane strips
through the 4-lane into the 8-lane ones and back, wavefronts whose two tasks ask for different widths, calls whose groups do and do
not reach into the packed top blocks -- in both walk modes (walk_many by default in such small batches; the one-task walk of long
launches in a child process with GAMDP_SIDE_WALK_ROUNDS=0)."""
import functools
import os
import random
import subprocess
import sys

import pytest

import _cases
import _oracle as O
from _gpu import ctx, oracle_for, run_cases

pytestmark = pytest.mark.gpu

BAND, C = 512, 17
# PairStripTable: first lane + shift of strips 0 .. 15 (and where a 17th would begin); the shift that puts column 512 (lane 30) mid-strip is 1
FIRST_U = [0, 8, 16, 20, 24, 26, 28, 30, 32, 34, 36, 38, 40, 44, 48, 56, 64]
SHIFT = 1


def strip_of_column(y):
    u = y // C + SHIFT
    return max(q for q in range(16) if FIRST_U[q] <= u)


def width_of(q):
    return FIRST_U[q + 1] - FIRST_U[q]


def strip_columns(q):
    """first and last band column (1 .. 2 * BAND - 1: a path needs a neighbour column on either side to exist at all) of strip q"""
    return max(C * (FIRST_U[q] - SHIFT), 1), min(C * (FIRST_U[q + 1] - SHIFT) - 1, 2 * BAND - 1)


def test_the_table_as_the_tests_see_it():
    assert [width_of(q) for q in range(16)] == [8, 8, 4, 4] + [2] * 8 + [4, 4, 8, 8]
    q = strip_of_column(BAND)
    lo, hi = strip_columns(q)
    assert width_of(q) == 2 and min(BAND - lo, hi - BAND) >= 14      # the middle column: mid-strip, not at an edge
    assert strip_columns(0)[0] == 1 and strip_columns(15)[1] == 2 * BAND - 1   # every live lane in a strip


def displaced(rng, y, n, begin_a):
    """a pair (b: n bases) whose alignment runs down band column y; begin_a = 0: top blocks in the packed range, > band: none"""
    k = abs(y - BAND)
    if y >= BAND:
        a = _cases.rand_seq(rng, n + k)
        b = _cases.mutate(rng, a[k:], 0.02, 0.0, 0.0)
    else:
        a = _cases.rand_seq(rng, n - k)
        b = _cases.rand_seq(rng, k) + _cases.mutate(rng, a, 0.02, 0.0, 0.0)
    a = _cases.rand_seq(rng, begin_a) + a
    return dict(a=a.encode(), b=b.encode(), band=BAND, begin_a=begin_a, end_a=len(a) - 1, begin_b=0, end_b=len(b) - 1, fs=False, fe=False)


def drifting(rng, steps, seg=600):
    """block indels, `seg` rows apart: a step of +d moves the path d columns up the band (d bases only a has), -d down (only b has).
    (1 200 rows behind a step of 300: over 620 the aligner would rather run through unrelated bases than pay for 300 gaps twice.)"""
    a, b = [], []
    for d in [0] + steps:
        if d > 0:
            a.append(_cases.rand_seq(rng, d))
        elif d < 0:
            b.append(_cases.rand_seq(rng, -d))
        s = _cases.rand_seq(rng, 1200 if abs(d) == 300 else seg)
        a.append(s)
        b.append(_cases.mutate(rng, s, 0.01, 0.0, 0.0))
    a, b = "".join(a), "".join(b)
    return dict(a=a.encode(), b=b.encode(), band=BAND, begin_a=0, end_a=len(a) - 1, begin_b=0, end_b=len(b) - 1, fs=False, fe=False)


@functools.lru_cache(maxsize=None)
def displaced_cases():
    rng = random.Random(51217)
    ys = sorted({y for q in range(16) for y in strip_columns(q)})
    # the columns either side of every boundary between strips of different widths are among them
    for q in range(15):
        if width_of(q) != width_of(q + 1):
            assert strip_columns(q)[1] in ys and strip_columns(q)[1] + 1 in ys
    cases = []
    for i, y in enumerate(ys):
        cases.append(displaced(rng, y, 2600 + 37 * (i % 5), 0))
        if i % 2 == 0:
            cases.append(displaced(rng, y, 2700, 700))     # no top blocks: the plain instance of every width
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def drifting_cases():
    rng = random.Random(51218)
    return (drifting(rng, [150, 40, 300, -300, -40, -150]),        # 512 -> 662 -> 702 (4 lanes) -> 1002 (8 lanes) and back
            drifting(rng, [-150, -40, -300, 300, 40, 150]),        # 512 -> 362 -> 322 (4 lanes) -> 22 (8 lanes) and back
            drifting(rng, [40, -150, 300, -300, 150, -40]))


@functools.lru_cache(maxsize=None)
def mixed_cases():
    """neighbours of equal length (one wavefront each): a centred call next to one in a 4-lane or an 8-lane strip, either order"""
    rng = random.Random(51219)
    out = []
    for y, centred_first in ((BAND + 250, True), (BAND - 450, False), (BAND + 480, False), (BAND - 200, True)):
        pair = [displaced(rng, BAND, 3100, 0), displaced(rng, y, 3100, 0)]
        assert len(pair[0]["b"]) == len(pair[1]["b"])
        out += pair if centred_first else pair[::-1]
    return tuple(out)


_oracle_cache = {}


def oracle_of(cs):
    """(result, edit string) of the oracle, computed once per case (the record without the edit string is the same record)"""
    k = id(cs)
    if k not in _oracle_cache:
        _oracle_cache[k] = (cs, oracle_for(cs, True))      # (cs: kept alive, its id stays its own)
    return _oracle_cache[k][1]


def path_strips(cs, o, ops):
    """the strips the oracle's path visits, from its edit string"""
    x, pos = o.begin_b - cs["begin_b"], o.begin_a
    seen = set()
    for op in ops:
        seen.add(strip_of_column(pos - cs["begin_a"] - x + BAND))
        if op == "A":
            x += 1
        elif op == "B":
            pos += 1
        else:
            x += 1
            pos += 1
    return seen


def check(cases, min_ok):
    n_ok = 0
    for want_ops in (True, False):
        res = run_cases(list(cases), want_ops=want_ops)
        info = ctx().launch_info()
        assert {r["kernel"] for r in info} == {"k_align_p<17,4>"}, info
        assert sum(r["units_dirfree"] for r in info) > 0, info
        for k, (cs, r) in enumerate(zip(cases, res)):
            o, ops = oracle_of(cs)
            assert r.key() == o.key(), (want_ops, k, len(cs["a"]), len(cs["b"]), r.key(), o.key())
            assert (not want_ops) or r.ops == ops, k
            n_ok += o.status == O.OK
    assert n_ok >= min_ok


def test_paths_on_the_first_and_last_column_of_every_strip():
    cases = displaced_cases()
    check(cases, 2 * len(cases))
    seen = set()
    for cs in cases:
        seen |= path_strips(cs, *oracle_of(cs))
    assert seen == set(range(16))


def test_paths_drifting_through_strips_of_every_width_and_back():
    cases = drifting_cases()
    check(cases, 2 * len(cases))
    for cs in cases[:2]:
        o, ops = oracle_of(cs)
        # one walk: 2 -> 4 -> 8 lanes and back to the strip it began in
        x, pos, widths = o.begin_b, o.begin_a, []
        for op in ops:
            w = width_of(strip_of_column(pos - x + BAND))
            if not widths or widths[-1] != w:
                widths.append(w)
            x += op != "B"
            pos += op != "A"
        assert widths == [2, 4, 8, 4, 2], widths


def test_two_tasks_of_a_wavefront_in_strips_of_different_widths():
    cases = mixed_cases()
    check(cases, 2 * len(cases))
    for k in range(0, len(cases), 2):
        wa, wb = ({width_of(q) for q in path_strips(cs, *oracle_of(cs))} for cs in cases[k:k + 2])
        assert wa != wb and {2} in (wa, wb), (k, wa, wb)


def test_a_centred_path_is_served_by_the_narrow_strips():
    """Two centred, indel-free 6 kb pairs: the oracle's path stays on column `band`, so every call is on the 2-lane strip there and serves
    32 groups of 4 blocks.  The packed range starts with block 8 (behind the ramp) and ends with the last group: G whole groups, at most
    ceil(G / 32) + 1 calls per task (the + 1: the walk's first call starts at the group of the end cell, wherever it lies in the range).
    Uniform 4-lane strips (16 groups per call) need ceil(G / 16)."""
    rng = random.Random(51220)
    n = 6000
    cases = [displaced(rng, BAND, n, 0) for _ in range(2)]
    for cs in cases:
        o, ops = oracle_of(cs)
        assert o.status == O.OK and set(ops) <= {"M", "X"} and o.begin_a == 0 and o.begin_b == 0 and o.length >= n - 64
    res = run_cases(cases, want_ops=False)
    info = ctx().launch_info()
    assert [r["kernel"] for r in info] == ["k_align_p<17,4>"] and info[0]["units_dirfree"] == 1, info
    for cs, r in zip(cases, res):
        assert r.key() == oracle_of(cs)[0].key()
    groups = (n + 63 + 15) // 16 // 4 - 2          # blocks of 16 row-times over n rows + 63 lanes, in groups of 4, less blocks 0 .. 7
    per_task = info[0]["strips"] / len(cases)
    print("strip calls per task: %.1f over %d groups (bound %d, uniform 4-lane strips %d)" % (per_task, groups, -(-groups // 32) + 1, -(-groups // 16)))
    assert -(-groups // 32) + 1 < -(-groups // 16)
    assert per_task <= -(-groups // 32) + 1, info


def test_both_walk_modes():
    """everything above once more with GAMDP_SIDE_WALK_ROUNDS=0: no launch walks its two tasks side by side -- the one-task walk of the
    long launches (finish_walk) asks for the strips"""
    if os.environ.get("GAMDP_TEST_STRIP_WIDTHS_CHILD"):
        return
    env = dict(os.environ, GAMDP_SIDE_WALK_ROUNDS="0", GAMDP_TEST_STRIP_WIDTHS_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__)],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2500:] + r.stderr[-2000:]
