"""gamdp_ctx_set_ops_walk (include/gamdp.h): in GAMDP_OPS_WALK_RUNS mode the walk of a call that wants an edit string writes it a
diagonal run at a time.  Nothing the library delivers may depend on the mode.

Per systolic kernel (the thirteen cells of tests/_views.py other than "wide", each in a child process with the environment that takes a
small batch to the kernel, at the smallest band that selects it; launch_info().kernel confirms it): a dozen calls of 300 - 3 000 bases --
pairs at 3 / 1 / 1 %, an identical pair, a pair with an indel every 2 - 5 bases, a pair whose indels cancel, the view cases of the kit
(windows whose begin_a and begin_b differ mod 16, rc and suffix views, force_start, force_end), runs of N for the N-aware kernels -- run
in STEPS and in RUNS mode on one context:
  * every field of every gamdp_result and every delivered byte equal between the modes and equal to the oracle's;
  * with capacities 1, 15, 16, 17, length - 1, length and length + 16 in a buffer pre-filled with 0xEE: the same bytes in both modes, the
    string where it fits, nothing behind a capacity touched (a clipped string is delivered as 0xFF bytes, include/gamdp.h);
  * with only every other call wanting a string (the tasks of one wavefront differ): the same;
  * gamdp_ctx_ops_walk_stats: all zero in STEPS mode; in RUNS mode ops_by_run and ops_by_step equal the split of tests/_opsrunmodel.py
    over the oracle's strings exactly, ops_by_run > 0, `tasks` = the calls that wanted a string, and `runs` lies between what runs of
    at most 256 steps need and one per step;
  * where the kernel has a walk-skip property: with it (and backoff) on, the RUNS walks make no test and ask for the same strips.
The oracle's strings of every cell hold an OK call of 200 ops or more, three runs of 17 steps or more and two gap ops: asserted, so
that no cell passes empty.

In one more child: gamdp_align_batch_fp in RUNS mode against gamdp_carry_ops_batch fingerprint by fingerprint, in three chunks or more,
its statistics summed over the chunks; two contexts of one gamdp_multi handle on one device, one per mode, deliver the same bytes."""
import ctypes as C
import os
import random
import re
import subprocess
import sys

import pytest

import _cases
import _fillonly as FO
import _opsrunmodel as M
import _oracle as O
import _views as V
import _walkskip as W
import gam_ngs_amd as gam
from gam_ngs_amd import lib as L

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CELLS = [c for c in V.CELLS if c != "wide"]
ZERO = dict(tasks=0, ops_by_run=0, ops_by_step=0, runs=0)
# the walk-skip property of a cell's kernel (tests/_walkskip.py FAMILIES), if it has one
SKIP_PROP = {"o19": "walk_skip", "p17": "walk_skip_pair", "c17": "walk_skip_i32", "c17n": "walk_skip_i32", "q19": "walk_skip_i32",
             "q19n": "walk_skip_i32", "gen9": "walk_skip_i32", "gen17": "walk_skip_i32"}


# ---- the batch of a cell -----------------------------------------------------------------------------------------------------------

def plain(a, b, band, begin_a=0, begin_b=0, fs=False, fe=False):
    return dict(a=a, b=b, stored_a=a, stored_b=b, va=(False, 0), vb=(False, 0), band=band, begin_a=begin_a, end_a=len(a) - 1, begin_b=begin_b,
                end_b=len(b) - 1, fs=fs, fe=fe)


def sprinkle_n(rng, s, runs):
    s = bytearray(s)
    for _ in range(runs):
        p = rng.randrange(20, len(s) - 20)
        for k in range(p, p + rng.randint(1, 7)):
            s[k] = 4
    return bytes(s)


def cell_cases(cell):
    name, bands, n_mode, env = V.CELLS[cell]
    band = bands[0]
    rng = random.Random(sum(cell.encode()) * 1000 + band)
    lo = max(300, 2 * band + 60)
    out = []
    for n in (lo, lo + 437, 3000):                       # 3 / 1 / 1 %
        a = V.rand_codes(rng, n)
        out.append(plain(a, V.mutate(rng, a, 0.03, 0.01, 0.01), band))
    a = V.rand_codes(rng, lo + 211)
    out.append(plain(a, a, band))                        # identical
    b = bytearray()                                      # an indel every 2 - 5 bases
    k = 0
    while k < len(a):
        step = rng.randint(2, 5)
        b += a[k:k + step]
        k += step
        if rng.random() < 0.5:
            b.append(rng.getrandbits(2))
        else:
            k += 1
    out.append(plain(a, bytes(b), band))
    a = V.rand_codes(rng, lo + 333)                      # indels that cancel: the path leaves the diagonal by one column and comes back
    b = bytearray(a)
    for p in range(len(a) - 40, 60, -97):
        del b[p]
        b.insert(p - 30, rng.getrandbits(2))
    out.append(plain(a, bytes(b), band))
    a = V.rand_codes(rng, lo + 100)                      # windows that begin at different residues mod 16, forced ends
    b = V.mutate(rng, a, 0.02, 0.0, 0.0)
    out.append(plain(a, b[5:], band, begin_a=min(band, 21), begin_b=16))
    out.append(plain(a, b, band, begin_a=3, begin_b=3, fs=True))
    out.append(plain(a, b, band, begin_a=0, begin_b=0, fe=True))
    # the kit's view cases of the cell: rc and suffix views, windows, force_start / force_end (tails)
    views = [cs for cs in V.matrix_cases() if cs["cell"] == cell and cs["band"] == band and len(cs["a"]) <= 3000 and not cs["tag"].get("long")]
    kinds = set()
    for cs in views:
        key = (cs["tag"]["kinds"], cs["tag"]["tail"])
        if cs["tag"]["kinds"] != ("none", "none") and len(kinds) < 4 and key not in kinds and cs["tag"]["kinds"] not in {k for k, _ in kinds}:
            kinds.add(key)
            out.append(cs)
    if n_mode is False:
        assert all(4 not in cs["stored_a"] and 4 not in cs["stored_b"] for cs in out), cell
    else:                                                # runs of N on either side (every call of an N-aware cell holds one)
        for cs in out:
            if "tag" in cs:
                continue
            if n_mode or rng.random() < 0.5:
                cs["a"] = cs["stored_a"] = sprinkle_n(rng, cs["a"], 3)
                cs["b"] = cs["stored_b"] = sprinkle_n(rng, cs["b"], 3)
    return name, band, out


def diagonal_runs(ops):
    return [len(m) for m in re.findall(r"[MX]+", ops)]


# ---- one call -------------------------------------------------------------------------------------------------------------------------

class Batch:
    def __init__(self, c, cases):
        self.c, self.cases, self.n = c, cases, len(cases)
        seqs = []
        for cs in cases:
            seqs += [cs["stored_a"], cs["stored_b"]]
        self.sset = gam.SequenceSet(c, seqs, ascii=False)
        self.tasks = (L.Task * self.n)()
        for i, cs in enumerate(cases):
            t = self.tasks[i]
            t.a_id, t.b_id, t.band = 2 * i, 2 * i + 1, cs["band"]
            (t.a_rc, t.a_off), (t.b_rc, t.b_off) = cs["va"], cs["vb"]
            t.begin_a, t.end_a, t.begin_b, t.end_b, t.force_start, t.force_end = cs["begin_a"], cs["end_a"], cs["begin_b"], cs["end_b"], cs["fs"], cs["fe"]

    def align(self, caps, handle=None, sset=None):
        """gamdp_align_batch with the given capacities (0: no string) -> (every field of every result, the buffer's bytes, the offsets)"""
        lib = self.c.lib
        offs, total = [], 0
        for cap in caps:
            offs.append(total)
            total += cap + 16                                # 16 bytes of 0xEE behind every room
        buf = C.create_string_buffer(bytes([M.UNTOUCHED]) * total, total)
        ops = L.Ops(C.cast(buf, C.c_void_p), (C.c_uint64 * self.n)(*offs), (C.c_uint64 * self.n)(*caps))
        out = (L.Result * self.n)()
        rc = lib.gamdp_align_batch(handle or self.c.handle, sset or self.sset.handle, sset or self.sset.handle, self.tasks, self.n, out, C.byref(ops))
        assert rc == 0, self.c.last_error()
        return [FO.whole(r) for r in out], buf.raw, offs


def expected_buffer(answers, caps):
    out = bytearray()
    for (o, ops), cap in zip(answers, caps):
        room = bytearray([M.UNTOUCHED]) * (cap + 16)
        if cap and o.status == O.OK:
            raw = bytes(O.OPS.index(ch) for ch in ops)
            room[:min(cap, len(raw))] = raw if len(raw) <= cap else b"\xff" * cap
        out += room
    return bytes(out)


def launched(c, cs):
    """the call is not settled by the pre-checks: it is a task of a launch"""
    return c.lib.gamdp_task_preflight(len(cs["a"]), len(cs["b"]), cs["band"], cs["begin_a"], cs["end_a"], cs["begin_b"], cs["end_b"], int(cs["fs"]),
                                      int(cs["fe"]), None) == L.ST_OK


def both_modes(bt, answers, caps, what, kernel):
    """the call in STEPS and in RUNS mode on one context -> the statistics of the RUNS call"""
    c = bt.c
    want = expected_buffer(answers, caps)
    seen = {}
    for mode in (L.OPS_WALK_STEPS, L.OPS_WALK_RUNS):
        c.set_ops_walk(mode)
        try:
            res, raw, _ = bt.align(caps)
        finally:
            c.set_ops_walk(L.OPS_WALK_STEPS)
        info, st = c.launch_info(), c.ops_walk_stats()
        assert {r["kernel"] for r in info} == {kernel}, (what, info)
        assert st["mode"] == mode, st
        assert raw == want, (what, mode, [i for i in range(len(raw)) if raw[i] != want[i]][:8])
        for i, (r, (o, _)) in enumerate(zip(res, answers)):
            key = tuple(r[FO.FIELDS.index(f)] for f in ("status", "begin_a", "begin_b", "score", "n_match", "length", "first_a", "first_b", "first_found",
                                                        "last_a", "last_b", "last_found", "homology"))
            assert key == tuple(o.key()) and r[FO.FIELDS.index("cells")] == o.cells, (what, mode, i, key, o.key())
        seen[mode] = (res, raw, st, info)
    assert seen[0][0] == seen[1][0] and seen[0][1] == seen[1][1], what
    st0, st1 = seen[0][2], seen[1][2]
    assert {k: st0[k] for k in ZERO} == ZERO, st0
    wanted = [(cs, o, ops) for cs, (o, ops), cap in zip(bt.cases, answers, caps) if cap and launched(c, cs)]
    splits = [M.split(ops, o.begin_a, o.begin_b, cs["begin_b"]) for cs, o, ops in wanted if o.status == O.OK]
    by_run, by_step = sum(s[0] for s in splits), sum(s[1] for s in splits)
    assert (st1["ops_by_run"], st1["ops_by_step"]) == (by_run, by_step) and by_run > 0, (what, st1, by_run, by_step)
    assert by_run + by_step == sum(o.length for _, o, _ in wanted if o.status == O.OK)
    assert st1["tasks"] == len(wanted), (what, st1, len(wanted))
    least = sum(-(-n // 256) for cs, o, ops in wanted if o.status == O.OK for n in diagonal_runs(ops[1:]))   # (a string's first op is a step from row 0 or pos == 0)
    assert least <= st1["runs"] <= by_run, (what, st1, least)
    print("  %s %s: %d calls, %d strings; RUNS: %s" % (kernel, what, bt.n, len(wanted), st1))
    return seen


def child_cell():
    cell = os.environ["OPS_WALK_CELL"]
    kernel, band, cases = cell_cases(cell)
    assert 12 <= len(cases) <= 16, len(cases)
    c = W.ctx()
    answers = FO.oracle_answers(cases)
    # the coverage condition, on the oracle's strings
    good = [ops for o, ops in answers if o.status == O.OK and o.length >= 200 and sum(1 for n in diagonal_runs(ops) if n >= 17) >= 3 and
            ops.count("A") + ops.count("B") >= 2]
    assert good, (cell, [(o.status, o.length) for o, _ in answers])
    assert sum(1 for o, _ in answers if o.status == O.OK) >= 10, [(o.status, o.length) for o, _ in answers]
    bt = Batch(c, cases)
    lens = [o.length if o.status == O.OK else 40 for o, _ in answers]
    full = [n + 16 for n in lens]
    seen = both_modes(bt, answers, full, "whole strings", kernel)
    named = lambda n, k: max(1, (1, 15, 16, 17, n - 1, n, n + 16)[k % 7])
    both_modes(bt, answers, [named(n, i) for i, n in enumerate(lens)], "capacities", kernel)
    both_modes(bt, answers, [named(n, i + 3) for i, n in enumerate(lens)], "capacities, shifted", kernel)
    both_modes(bt, answers, [cap if i % 2 else 0 for i, cap in enumerate(full)], "every other call", kernel)
    both_modes(bt, answers, [0 if i % 3 == 1 else cap for i, cap in enumerate(full)], "two of three calls", kernel)
    prop = SKIP_PROP.get(cell)
    if prop:   # the diagonal test stays away from a walk that writes a string
        strips = sum(r["strips"] for r in seen[1][3])
        getattr(c, "set_" + prop)(L.WALK_SKIP_DIAG)
        c.set_walk_skip_backoff(L.WALK_BACKOFF_ON)
        c.set_ops_walk(L.OPS_WALK_RUNS)
        try:
            res, raw, _ = bt.align(full)
        finally:
            getattr(c, "set_" + prop)(L.WALK_STRIPS)
            c.set_walk_skip_backoff(L.WALK_BACKOFF_OFF)
            c.set_ops_walk(L.OPS_WALK_STEPS)
        sk, info = getattr(c, prop + "_stats")(), c.launch_info()
        assert sk["mode"] == L.WALK_SKIP_DIAG and sk["tests"] == sk["groups_tested"] == sk["groups_skipped"] == 0, sk
        assert c.walk_skip_backoff_stats()[{"walk_skip": "held", "walk_skip_pair": "held_pair", "walk_skip_i32": "held_i32"}[prop]] == 0
        assert sum(r["strips"] for r in info) == strips and (res, raw) == (seen[1][0], seen[1][1])
        assert c.ops_walk_stats() == seen[1][2]
        print("  %s with %s on: no test, %d strips" % (kernel, prop, strips))


def child_fp_and_multi():
    c = W.ctx()
    rng = random.Random(77)
    cases = []
    for k in range(24):
        a = V.rand_codes(rng, rng.randint(300, 1500))
        cases.append(plain(a, V.mutate(rng, a, 0.03, 0.01, 0.01) if k % 5 else a, (150, 40, 512)[k % 3]))
    answers = FO.oracle_answers(cases)
    bt = Batch(c, cases)
    out, fp = (L.Result * bt.n)(), (C.c_uint32 * bt.n)()
    assert c.lib.gamdp_carry_ops_batch(c.handle, bt.sset.handle, bt.sset.handle, bt.tasks, bt.n, out, fp) == 0, c.last_error()
    want = [(FO.whole(r), f) for r, f in zip(out, fp)]
    assert all(f == (FO.fp_of(ops) if o.status == O.OK else 0) for f, (o, ops) in zip(fp, answers))
    rooms = sum(c.lib.gamdp_task_ops_cap(len(cs["a"]), len(cs["b"]), cs["band"], cs["begin_a"], cs["end_a"], cs["begin_b"], cs["end_b"], 0, 0) for cs in cases)
    seen = {}
    c.set_ops_chunk_bytes(rooms // 4)
    try:
        for mode in (L.OPS_WALK_STEPS, L.OPS_WALK_RUNS):
            c.set_ops_walk(mode)
            out2, fp2 = (L.Result * bt.n)(), (C.c_uint32 * bt.n)()
            assert c.lib.gamdp_align_batch_fp(c.handle, bt.sset.handle, bt.sset.handle, bt.tasks, bt.n, out2, fp2) == 0, c.last_error()
            assert [(FO.whole(r), f) for r, f in zip(out2, fp2)] == want, mode
            assert c.ops_fp_info()["chunks"] >= 3, c.ops_fp_info()
            seen[mode] = c.ops_walk_stats()
    finally:
        c.set_ops_walk(L.OPS_WALK_STEPS)
        c.set_ops_chunk_bytes(0)
    assert seen[0] == dict(ZERO, mode=0), seen[0]
    splits = [M.split(ops, o.begin_a, o.begin_b, cs["begin_b"]) for cs, (o, ops) in zip(cases, answers) if o.status == O.OK]
    st = seen[1]
    assert (st["tasks"], st["ops_by_run"], st["ops_by_step"], st["mode"]) == (bt.n, sum(s[0] for s in splits), sum(s[1] for s in splits), 1), st
    print("  fingerprints in %d chunks: %s" % (c.ops_fp_info()["chunks"], st))
    # two contexts of one handle on one device, one per mode
    m = gam.MultiContext([0, 0])
    m.set_ops_walk(L.OPS_WALK_RUNS, which=1)
    seqs = []
    for cs in cases:
        seqs += [cs["stored_a"], cs["stored_b"]]
    ms = gam.MultiSequenceSet(m, seqs, ascii=False)
    full = [(o.length if o.status == O.OK else 40) + 16 for o, _ in answers]
    got = []
    for i in range(2):
        h, s = C.c_void_p(c.lib.gamdp_multi_ctx(m.handle, i)), C.c_void_p(c.lib.gamdp_multi_seqset_on(ms.handle, i))
        got.append(bt.align(full, handle=h, sset=s)[:2])
    sts = m.ops_walk_stats()
    assert got[0] == got[1] and got[0][1] == expected_buffer(answers, full)
    assert [s["mode"] for s in sts] == [0, 1] and {k: sts[0][k] for k in ZERO} == ZERO and sts[1]["ops_by_run"] == st["ops_by_run"], sts
    # ... and gamdp_multi_align_batch runs each context in its own mode: the results do not differ from one context's
    out3 = (L.Result * bt.n)()
    assert c.lib.gamdp_multi_align_batch(m.handle, ms.handle, ms.handle, bt.tasks, bt.n, out3) == 0, m.last_error()
    assert [FO.whole(r) for r in out3] == [w for w, _ in want]
    print("  two contexts of one handle: the same bytes")


CHILDREN = {"cell": child_cell, "fp_and_multi": child_fp_and_multi}


def run_child(name, cell=None):
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_ops_walk as T\nT.CHILDREN[%r]()\nprint('CHILD_OK')\n") % (ROOT, HERE, name)
    env = {k: v for k, v in os.environ.items() if k not in W.SWITCHES + ("GAMDP_OPS_WALK_RUNS",) and not k.startswith("GAMDP_DIAG_")}
    if cell:
        env.update(V.CELLS[cell][3])
        env["OPS_WALK_CELL"] = cell
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and "CHILD_OK" in r.stdout, (name, cell, r.stdout[-3000:] + r.stderr[-3000:])


@pytest.mark.parametrize("cell", CELLS)
def test_both_modes_deliver_the_same(cell):
    run_child("cell", cell)


def test_fingerprints_in_chunks_and_two_contexts_of_one_handle():
    run_child("fp_and_multi")
