#!/usr/bin/env python3
"""A/B of the eight-task kernel's walk modes (gamdp_ctx_set_walk_skip): GAMDP_WALK_STRIPS against GAMDP_WALK_SKIP_DIAG and against
GAMDP_WALK_SKIP_DIAG with gamdp_ctx_set_walk_skip_backoff on, alternating call by call in ONE process on ONE context, at several
divergences.

Workloads (band 150): 100 000 x 5 kb, 16 384 x 50 kb, and the batch shaped like the merge-block driver's calls (tests/_mixed.py), each
at the divergences of DIVERGENCES (substitutions / insertions / deletions in per cent of the bases; the first is bench.py's config 5).
The pairs are made here, in numpy (gamdp_synth_pair's rates are fixed).  Per row: a warm-up call in either mode, then --reps calls per
mode, alternating; kernel time from gamdp_ctx_kernel_time; median and min - max per mode; every call's results are compared byte for
byte with the first call's; the device's counts (gamdp_ctx_walk_skip_stats, gamdp_ctx_launch_info) of a call in either mode.  With
--carry every row also runs gamdp_carry_batch once -- a kernel without any walk -- and compares whole results with it.
--piecewise adds two rows per pair workload: pairs whose divergence changes along the pair (tests/_piecewise.py), in both orders.

    python tools/walk_skip_ab.py [--reps 7] [--scale 1.0] [--workloads 5k,50k,mixed] [--piecewise] [--rows 0,2,5,6] [--carry] [--json]

--scale shrinks the pair counts (a quick look; the table of DESIGN.md section 6 is --scale 1).  No planner switch is needed at these
sizes (GAMDP_QUAD_MIN is for small batches)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gam_ngs_amd as gam  # noqa: E402
from gam_ngs_amd import lib as L  # noqa: E402
from srchash import source_hash  # noqa: E402

BAND = 150
DIVERGENCES = ((3.0, 1.0, 1.0), (2.0, 0.5, 0.5), (0.3, 0.1, 0.1), (0.05, 0.02, 0.02), (0.0, 0.0, 0.0))
KERNEL = "k_align_o<19,15>"
# the three columns: (gamdp_ctx_set_walk_skip, gamdp_ctx_set_walk_skip_backoff)
OFF, ON, BACKOFF = (L.WALK_STRIPS, L.WALK_BACKOFF_OFF), (L.WALK_SKIP_DIAG, L.WALK_BACKOFF_OFF), (L.WALK_SKIP_DIAG, L.WALK_BACKOFF_ON)
SETTINGS = (OFF, ON, BACKOFF)


def diverged(rng, A, n_pairs, length, sub, ins, dele):
    """B for the n_pairs sequences of `length` bases in A (one array): events drawn sparsely, applied in one pass.
    -> (B as one array, the lengths of its sequences)"""
    N = A.size
    B = A.copy()
    k = rng.binomial(N, sub)
    if k:
        p = rng.integers(0, N, k)
        B[p] = (A[p] + rng.integers(1, 4, k).astype(np.uint8)) & 3
    cnt = np.ones(N, np.uint8)
    k = rng.binomial(N, dele)
    if k:
        cnt[rng.integers(0, N, k)] = 0
    k = rng.binomial(N, ins)
    ins_at = np.unique(rng.integers(0, N, k)) if k else np.zeros(0, np.int64)
    cnt[ins_at] += 1
    lens = cnt.reshape(n_pairs, length).sum(axis=1, dtype=np.int64)
    out = np.repeat(B, cnt)
    if ins_at.size:   # the inserted base: the last copy of its source base
        ends = np.cumsum(cnt, dtype=np.int64)
        out[ends[ins_at] - 1] = rng.integers(0, 4, ins_at.size).astype(np.uint8)
    return out, lens


def pairs_workload(ctx, rng, n_pairs, length, div):
    sub, ins, dele = (v / 100.0 for v in div)
    seqs = []
    blens = []
    step = max(1, (32 << 20) // length)    # ~32 M bases at a time
    for first in range(0, n_pairs, step):
        n = min(step, n_pairs - first)
        A = rng.integers(0, 4, n * length, dtype=np.uint8)
        Bs, lens = diverged(rng, A, n, length, sub, ins, dele)
        at = 0
        for k in range(n):
            seqs.append(A[k * length:(k + 1) * length].tobytes())
            seqs.append(Bs[at:at + lens[k]].tobytes())
            at += int(lens[k])
            blens.append(int(lens[k]))
    sset = gam.SequenceSet(ctx, seqs, ascii=False)
    tasks = (L.Task * n_pairs)()
    for k in range(n_pairs):
        t = tasks[k]
        t.a_id, t.b_id, t.band = 2 * k, 2 * k + 1, BAND
        t.begin_a, t.end_a, t.begin_b, t.end_b = 0, length - 1, 0, max(blens[k], 1) - 1
    return sset, tasks, n_pairs


def piecewise_workload(ctx, rng, n_pairs, length, reverse, band=BAND):
    """pairs whose divergence changes along the pair (tests/_piecewise.py: thirds at 3/1/1 %, 0/0/0 and 0.3/0.1/0.1, or the other way round)"""
    import _piecewise
    seqs, blens = [], []
    step = max(1, (32 << 20) // length)
    for first in range(0, n_pairs, step):
        A, Bs = _piecewise.batch(rng, min(step, n_pairs - first), length, reverse=reverse)
        for a, b in zip(A, Bs):
            seqs.append(a.tobytes())
            seqs.append(b.tobytes())
            blens.append(len(b))
    sset = gam.SequenceSet(ctx, seqs, ascii=False)
    tasks = (L.Task * n_pairs)()
    for k in range(n_pairs):
        t = tasks[k]
        t.a_id, t.b_id, t.band = 2 * k, 2 * k + 1, band
        t.begin_a, t.end_a, t.begin_b, t.end_b = 0, length - 1, 0, max(blens[k], 1) - 1
    return sset, tasks


def mixed_workload(ctx, n_pairs, div):
    import _mixed
    sub, ins, dele = (v / 100.0 for v in div)
    plain = _mixed._mutate
    _mixed._mutate = lambda rng, a: plain(rng, a, sub, ins, dele)     # (mixed_batch mutates with its defaults)
    try:
        seqs, calls = _mixed.mixed_batch(20261004, n_pairs, 8)
    finally:
        _mixed._mutate = plain
    sset = gam.SequenceSet(ctx, seqs, ascii=False)
    tasks = (L.Task * len(calls))()
    _mixed.fill_tasks(tasks, calls)
    return sset, tasks, len(calls)


def one_row(ctx, name, sset, tasks, n, div, reps, carry):
    outs = {m: (L.Result * n)() for m in SETTINGS}
    first = None
    ms = {m: [] for m in SETTINGS}
    stats, strips, held, octo_tasks = {}, {}, 0, 0
    different = 0
    for rep in range(reps + 1):            # (rep 0 warms up)
        for mode in SETTINGS:
            ctx.set_walk_skip(mode[0])
            ctx.set_walk_skip_backoff(mode[1])
            ctx.kernel_time(reset=True)
            rc = ctx.lib.gamdp_align_batch(ctx.handle, sset.handle, sset.handle, tasks, n, outs[mode], None)
            assert rc == 0, (rc, ctx.last_error())
            if rep:
                ms[mode].append(ctx.kernel_time()[0])
            raw = C.string_at(outs[mode], C.sizeof(outs[mode]))
            if first is None:
                first = raw
            different += raw != first
            if rep == reps:
                stats[mode] = ctx.walk_skip_stats()
                info = ctx.launch_info()
                strips[mode] = sum(r["strips"] for r in info)
                octo_tasks = sum(r["tasks"] for r in info if r["kernel"] == KERNEL)
                held = ctx.walk_skip_backoff_stats()["held"]
    ctx.set_walk_skip(L.WALK_STRIPS)
    ctx.set_walk_skip_backoff(L.WALK_BACKOFF_OFF)
    rec = dict(workload=name, calls=n, eight_task_calls=octo_tasks, sub=div[0], ins=div[1], dele=div[2], results_differ=different,
               strips_off=strips[OFF], strips_on=strips[ON], strips_backoff=strips[BACKOFF], stats_on=stats[ON], stats_backoff=stats[BACKOFF], held=held)
    for mode, key in ((OFF, "off"), (ON, "on"), (BACKOFF, "backoff")):
        v = sorted(ms[mode])
        rec["ms_" + key] = dict(median=round(v[len(v) // 2], 2), min=round(v[0], 2), max=round(v[-1], 2))
    if carry:
        ca = (L.Result * n)()
        rc = ctx.lib.gamdp_carry_batch(ctx.handle, sset.handle, sset.handle, tasks, n, ca)
        assert rc == 0, (rc, ctx.last_error())
        whole = lambda r: r.key() + (r.cells,)  # noqa: E731
        rec["carry_mismatches"] = sum(1 for m in (ON, BACKOFF) for i in range(n) if whole(outs[m][i]) != whole(ca[i]))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--workloads", default="5k,50k,mixed")
    ap.add_argument("--piecewise", action="store_true", help="two more rows per pair workload: the divergence changes along the pair, both orders")
    ap.add_argument("--rows", default="", help="only these rows of every workload: indices into DIVERGENCES, the two piecewise rows behind them (e.g. 0,2,5,6)")
    ap.add_argument("--carry", action="store_true")
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    assert args.reps >= 1
    ctx = gam.Context(0)
    rows = []
    print("source %s, %d calls per mode after a warm-up, kernel ms: median (min - max)" % (source_hash(), args.reps), flush=True)
    print("%-16s %-15s %9s %9s %9s %12s %12s %9s  %-24s %-24s %-24s %s" % ("workload", "sub/ins/del %", "strips", "strips on", "strips bo", "grp skipped",
                                                                      "skipped bo", "held", "ms off", "ms on", "ms on + backoff", "on/off  bo/off"), flush=True)
    for w in args.workloads.split(","):
        rows_of = list(enumerate(DIVERGENCES)) + ([(len(DIVERGENCES), "piecewise"), (len(DIVERGENCES) + 1, "piecewise rev")] if args.piecewise and w != "mixed" else [])
        for di, div in rows_of:
            if args.rows and str(di) not in args.rows.split(","):
                continue
            rng = np.random.default_rng(20261019 + di)
            if isinstance(div, str):
                n, length = (max(8, int(100000 * args.scale)), 5000) if w == "5k" else (max(8, int(16384 * args.scale)), 50000)
                sset, tasks = piecewise_workload(ctx, rng, n, length, div.endswith("rev"))
                name = "%d x %d kb" % (n, length // 1000)
                div = (div, "", "")
            elif w == "5k":
                sset, tasks, n = pairs_workload(ctx, rng, max(8, int(100000 * args.scale)), 5000, div)
                name = "%d x 5 kb" % n
            elif w == "50k":
                sset, tasks, n = pairs_workload(ctx, rng, max(8, int(16384 * args.scale)), 50000, div)
                name = "%d x 50 kb" % n
            else:
                sset, tasks, n = mixed_workload(ctx, max(8, int(12500 * args.scale)), div)
                name = "mixed150 %d" % n
            rec = one_row(ctx, name, sset, tasks, n, div, args.reps, args.carry)
            sset.close()
            rows.append(rec)
            f = lambda d: "%.2f (%.2f - %.2f)" % (d["median"], d["min"], d["max"])  # noqa: E731
            print("%-16s %-15s %9d %9d %9d %12d %12d %9d  %-24s %-24s %-24s %.3f  %.3f%s%s" % (
                name, div[0] if isinstance(div[0], str) else "%g/%g/%g" % div, rec["strips_off"], rec["strips_on"], rec["strips_backoff"],
                rec["stats_on"]["groups_skipped"], rec["stats_backoff"]["groups_skipped"], rec["held"],
                f(rec["ms_off"]), f(rec["ms_on"]), f(rec["ms_backoff"]), rec["ms_on"]["median"] / rec["ms_off"]["median"],
                rec["ms_backoff"]["median"] / rec["ms_off"]["median"],
                "  RESULTS DIFFER in %d calls" % rec["results_differ"] if rec["results_differ"] else "",
                ("  carry mismatches %d" % rec["carry_mismatches"]) if args.carry else ""), flush=True)
    if args.json:
        print(json.dumps(dict(source=source_hash(), reps=args.reps, rows=rows)))
    bad = sum(r["results_differ"] for r in rows) + sum(r.get("carry_mismatches", 0) for r in rows)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
