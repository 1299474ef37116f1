"""What the walk-skip GPU tests share (test_gpu_walk_skip.py, _pair.py, _i32.py, _backoff.py, _pieces.py): the kernel families, the
context of a child process, the off-and-on runner and the SHORT scan.

A family is a kernel reached one way: the property that switches its walks' diagonal test on (gamdp_ctx_set_walk_skip, _pair, _i32),
the kernels whose launches that property's statistics count, the environment that takes a small batch to the kernel.  A child process
is about one family: setup(name) chooses it, F reads it."""
import functools
import os
import random
import subprocess
import sys

import _cases
import _oracle as O
import gam_ngs_amd as gam
from gam_ngs_amd import lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DIAG_LIB = os.path.join(ROOT, "gam_ngs_amd", "libgamdp_diag.so")
# what a child's environment must not inherit (each child then gets its family's own switches)
SWITCHES = ("GAMDP_QUAD_MIN", "GAMDP_NO_PAIR", "GAMDP_NO_MERGE_N", "GAMDP_WALK_SKIP", "GAMDP_WALK_SKIP_PAIR", "GAMDP_WALK_SKIP_I32",
            "GAMDP_WALK_SKIP_BACKOFF", "GAMDP_LIB", "GAMDP_SIDE_WALK_ROUNDS", "GAMDP_NO_PACKED_TOP", "GAMDP_NO_PACKED_TOP_MIXED",
            "GAMDP_OCTO_MIN_ROWS", "GAMDP_NO_AUX_LAUNCH")
COUNTERS = ("tests", "groups_tested", "groups_skipped", "rows_skipped")
O19, P17 = "k_align_o<19,15>", "k_align_p<17,4>"
# the six int32 direction-free kernels by their cell of tests/_views.py
I32 = {"c17": "k_align<17,4,false>", "c17n": "k_align<17,4,true>", "q19": "k_align_q<19,15,false>", "q19n": "k_align_q<19,15,true>",
       "gen9": "k_align<9,-1,true>", "gen17": "k_align<17,-1,true>"}
SIX = set(I32.values())


def side_by_side():
    return int(os.environ["GAMDP_SIDE_WALK_ROUNDS"]) > 0


def check_path(st, info):
    """the walk path of the call's two-task launches is the one this child's environment asks for"""
    n = sum(1 for r in info if r["kernel"] == P17)
    assert n > 0, info
    assert (st["launches_side_by_side"], st["launches_one_by_one"]) == ((n, 0) if side_by_side() else (0, n)), (st, info)


def check_launches(st, info):
    assert st["launches"] == sum(1 for r in info if r["kernel"] in SIX) > 0, (st, info)


class Family:
    """name; prop: the property (Context.set_<prop>, Context.<prop>_stats); held: its field of the backoff statistics; kernel: the one
    under test; kernels: those the property's statistics count; band; C: columns per lane; lpt: lanes per task; need_n: False no N /
    True an N needed / None either; env: the child's switches; K: groups one test looks at, at most (a number or a function of the
    child's environment); scan: where SHORT is looked for, seed: of its pairs, short_calls: identical pairs per scan step (one
    wavefront's); fits: lengths rounded up by fit(); check: what else holds for the statistics of every call (st, info)."""

    def __init__(self, name, prop, held, kernel, band, C, lpt, K, scan, seed, env, kernels=None, need_n=None, short_calls=1, fits=False,
                 check=None):
        self.name, self.prop, self.held, self.kernel, self.band, self.C, self.lpt, self.K = name, prop, held, kernel, band, C, lpt, K
        self.scan, self.seed, self.env, self.kernels, self.need_n = scan, seed, env, kernels or {kernel}, need_n
        self.short_calls, self.fits, self.check = short_calls, fits, check
        self.cell = name             # (the int32 families are named after their cell of tests/_views.py)
        self.LE, self.lc = 2 * band // C, band // C   # the lanes (within the task) of the band's last and of its centre column

    def set(self, c, mode):
        getattr(c, "set_" + self.prop)(mode)

    def stats(self, c):
        return getattr(c, self.prop + "_stats")()


def _i32(cell, band, C, lpt, need_n, env):
    return Family(cell, "walk_skip_i32", "held_i32", I32[cell], band, C, lpt, 64, (192, 2049, 64), 64512, env, kernels=SIX, need_n=need_n,
                  fits=True, check=check_launches)


def _p17(name, rounds):   # SHORT: the range begins with block 8 (behind the ramp of 61 lanes)
    return Family(name, "walk_skip_pair", "held_pair", P17, 512, 17, 64, lambda: 8 if side_by_side() else 64, (192, 1601, 64), 64512,
                  {"GAMDP_SIDE_WALK_ROUNDS": rounds}, short_calls=2, check=check_path)


FAMILIES = {f.name: f for f in (
    # SHORT: by the block plan it lies near 35 blocks of 16 rows
    Family("o19", "walk_skip", "held", O19, 150, 19, 16, 8, (448, 1217, 16), 64150, {"GAMDP_QUAD_MIN": "1"}),
    _p17("p17_one", "0"),
    _p17("p17_side", "1000000"),
    _i32("c17", 512, 17, 64, False, {"GAMDP_NO_PAIR": "1"}),
    _i32("c17n", 512, 17, 64, True, {}),
    _i32("q19", 150, 19, 16, False, {"GAMDP_NO_PAIR": "1", "GAMDP_QUAD_MIN": "1"}),
    _i32("q19n", 150, 19, 16, True, {"GAMDP_QUAD_MIN": "1"}),
    _i32("gen9", 200, 9, 64, None, {}),
    _i32("gen17", 300, 17, 64, None, {}),
)}


# ---- in the child ------------------------------------------------------------------------------------------------------------------

_family = [None]


def setup(name):
    _family[0] = FAMILIES[name]


class _Current:
    """the family this child is about (setup())"""

    def __getattr__(self, k):
        assert _family[0] is not None, "setup(family) first"
        return getattr(_family[0], k)


F = _Current()


@functools.lru_cache(maxsize=1)
def ctx():
    return gam.Context(0)


def fit(n):
    """families that round lengths (test_gpu_walk_skip_i32.py): the shortest length >= n whose last block is the last block of a group"""
    return n + (-(n + F.LE)) % 64 if F.fits else n


def trimmed(a, b):
    """the pair without the last few bases of both (an unchanged stretch): rows + LE a multiple of 64, as fit() makes it for equal lengths"""
    if not F.fits:
        return a, b
    t = (len(b) + F.LE) % 64
    assert len(b) - t <= len(a) - t + F.band
    return a[:len(a) - t], b[:len(b) - t]


def route(a, b, same=False):
    """the pair as the kernel under test takes it: an N for the kernels that only N-holding calls reach"""
    if F.need_n and "N" not in a + b:
        a = a[:5] + "N" + a[6:]
        if same:
            b = a
    assert not (F.need_n is False and "N" in a + b)
    return a, b


def case(a, b, begin_a=0, end_a=None, begin_b=0, end_b=None, fs=False, fe=False, same=False):
    a, b = route(a, b, same)
    return dict(a=a.encode(), b=b.encode(), band=F.band, begin_a=begin_a, end_a=len(a) - 1 if end_a is None else end_a, begin_b=begin_b,
                end_b=len(b) - 1 if end_b is None else end_b, fs=fs, fe=fe)


def run(cases, want_ops):
    import _gpu
    _gpu.ctx = ctx          # (run_cases on this module's context)
    return _gpu.run_cases(cases, want_ops=want_ops)


def oracle_all(cases):
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(16) as ex:   # (the oracle's C code runs outside the GIL)
        return list(ex.map(lambda cs: O.oracle_align(O.encode(cs["a"]), O.encode(cs["b"]), cs["band"], cs["begin_a"], cs["end_a"], cs["begin_b"],
                                                     cs["end_b"], cs["fs"], cs["fe"], want_ops=True), cases))


def mine(info):
    return [r for r in info if r["kernel"] == F.kernel]


def family_rows(info):
    """the launches the family's statistics count"""
    return [r for r in info if r["kernel"] in F.kernels]


def family_strips(info):
    return sum(r["strips"] for r in family_rows(info))


def check_stats(st, info, mode):
    """the invariants of every call"""
    assert st["mode"] == mode, st
    if F.check:
        F.check(st, info)
    assert st["strips"] == family_strips(info), (st, info)
    K = F.K() if callable(F.K) else F.K
    assert st["groups_skipped"] <= st["groups_tested"] <= K * st["tests"], st
    assert 64 * st["groups_skipped"] - 63 * st["tests"] <= st["rows_skipped"] <= 64 * st["groups_skipped"], st
    if mode == L.WALK_STRIPS:
        assert st["tests"] == st["groups_tested"] == st["groups_skipped"] == st["rows_skipped"] == 0, st


def check_results(cases, res, want, flags, what):
    for k, (cs, r, (o, ops), f) in enumerate(zip(cases, res, want, flags)):
        assert r.status != L.ST_DIAG_RANGE, (k, "a packed value left the exact range")
        assert r.key() == o.key(), (F.name, what, k, len(cs["a"]), len(cs["b"]), r.key(), o.key())
        assert r.ops == (ops if f else None), (F.name, what, k, "edit string")


def check_equal(res0, res1):
    for k, (r0, r1) in enumerate(zip(res0, res1)):
        assert r0.key() == r1.key() and r0.ops == r1.ops and r0.cells == r1.cells, (k, r0.key(), r1.key())


def both(cases, want_ops=False, want=None, only=True):
    """The batch with the property off, then on, on one context.  Every result equals the oracle's and the other mode's.
    -> (oracle answers, launch info off, launch info on, stats off, stats on)"""
    c = ctx()
    want = want or oracle_all(cases)
    flags = list(want_ops) if isinstance(want_ops, (list, tuple)) else [bool(want_ops)] * len(cases)
    out = {}
    for mode in (L.WALK_STRIPS, L.WALK_SKIP_DIAG):
        F.set(c, mode)
        try:
            res = run(cases, want_ops)
        finally:
            F.set(c, L.WALK_STRIPS)
        info, st = c.launch_info(), F.stats(c)
        assert mine(info), (F.kernel, info)
        if only:
            assert {r["kernel"] for r in info} == {F.kernel}, info
        check_stats(st, info, mode)
        check_results(cases, res, want, flags, mode)
        out[mode] = (res, info, st)
    check_equal(out[0][0], out[1][0])
    st0, st1 = out[0][2], out[1][2]
    print("  %s %d calls: strips off %d on %d, tests %d, groups tested %d skipped %d, rows skipped %d" %
          (F.name, len(cases), st0["strips"], st1["strips"], st1["tests"], st1["groups_tested"], st1["groups_skipped"], st1["rows_skipped"]))
    return want, out[0][1], out[1][1], st0, st1


def gap_free(ops):
    return set(ops) <= {"M", "X"}


@functools.lru_cache(maxsize=None)
def _short_length(name):
    c = ctx()
    rng = random.Random(F.seed)
    lo, hi, step = F.scan
    scan = range(fit(lo), hi, step)
    t = F.short_calls
    seen = []
    F.set(c, L.WALK_SKIP_DIAG)
    try:
        for n in scan:
            a = _cases.rand_seq(rng, n)
            run([case(a, a, same=True) for _ in range(t)], False)
            info, st = c.launch_info(), F.stats(c)
            assert [r["kernel"] for r in info] == [F.kernel], info
            seen.append((n, info[0]["units_dirfree"], st["groups_skipped"] // t))
            if info[0]["units_dirfree"] > 0 and st["groups_skipped"] >= t * 3:
                break
    finally:
        F.set(c, L.WALK_STRIPS)
    n, df, groups = seen[-1]
    assert df > 0 and groups >= 3, seen
    assert all(not (d > 0 and g >= 3) for _, d, g in seen[:-1])
    assert n > scan[0], ("the scan must begin below the shortest length", seen)
    print("  %s SHORT = %d (%s)" % (F.name, n, seen[-3:]))
    return n


def short_length():
    """The shortest length of the family's scan at which an identical pair has a direction-free range of 3 groups or more: with the
    property on an identical pair's walk jumps over every group of the range below its end cell, so groups_skipped counts them (per
    task: the scan of the two-task kernel runs two)."""
    return _short_length(F.name)


def sizes():
    s = short_length()
    return (s, fit(2 * s + 21), fit(3000), fit(4700), fit(6000))


def substituted(rng, a, rate):
    return _cases.mutate(rng, a, rate, 0.0, 0.0)


def one_indel(rng, n, row, kind):
    a = _cases.rand_seq(rng, n)
    if kind == "ins":     # a base only b has
        b = a[:row] + {"A": "C", "C": "G", "G": "T", "T": "A"}[a[row]] + a[row:]
    else:                 # a base only a has
        b = a[:row] + a[row + 1:]
    return case(*trimmed(a, b))


# ---- in the parent: a fresh child (never exec) -------------------------------------------------------------------------------------

def run_child(module, name, family=None, diag=False, extra=None, timeout=600):
    """CHILDREN[name]() of test module `module` in a fresh process: the environment without SWITCHES, then the family's own switches,
    the diagnostics library if asked for, then `extra` -> the child's output"""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import _walkskip as W\nif %r: W.setup(%r)\nimport %s as T\nT.CHILDREN[%r]()\nprint('CHILD_OK')\n") % (ROOT, HERE, family, family, module, name)
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES and not k.startswith("GAMDP_DIAG_")}
    if family:
        env.update(FAMILIES[family].env)
    if diag:
        env["GAMDP_LIB"] = DIAG_LIB
    env.update(extra or {})
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=timeout)
    print("%s %s\n%s" % (family, sorted(FAMILIES[family].env.items()) if family else "", r.stdout[-4000:]))
    assert r.returncode == 0 and "CHILD_OK" in r.stdout, (name, family, diag, r.stdout[-3000:] + r.stderr[-3000:])
    return r.stdout
