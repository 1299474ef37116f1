#!/usr/bin/env python3
"""A/B of the two-task band-512 kernel's walk modes (gamdp_ctx_set_walk_skip_pair): GAMDP_WALK_STRIPS against GAMDP_WALK_SKIP_DIAG,
alternating on ONE context, one batch per row.

Rows: 50 kb and 5 kb band-512 pairs, identical, at 0.04 % indels, at 0.2 % indels and at config 5's 3 % substitutions + 1 % + 1 %
indels, each as a long launch (more than two rounds: the walks run one task after the other, finish_walk) and as a launch of at most
two rounds (the two tasks side by side, walk_many) -- which path a row took is read from gamdp_ctx_walk_skip_pair_stats and printed.
Per row: kernel time of the call (gamdp_ctx_kernel_time) in either mode, median and range; whether the results of the two modes are
the same bytes; the device's counts; with --carry the results of the `on` mode against gamdp_carry_batch.
A third column runs GAMDP_WALK_SKIP_DIAG with gamdp_ctx_set_walk_skip_backoff on; --piecewise adds two rows per length: pairs whose
divergence changes along the pair (tests/_piecewise.py), in both orders; --rows picks rows by index.

    python tools/walk_skip_pair_ab.py [--reps 5] [--scale 1.0] [--lengths 50k,5k] [--piecewise] [--rows 0,3,4,5] [--carry] [--json]

--scale shrinks the pair counts (a quick look; a scaled-down `long` row may no longer be a long launch: the path column says)."""
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
from walk_skip_ab import BACKOFF, OFF, ON, SETTINGS, diverged, piecewise_workload  # noqa: E402

BAND = 512
DIVERGENCES = ((0.0, 0.0, 0.0), (0.0, 0.02, 0.02), (0.0, 0.1, 0.1), (3.0, 1.0, 1.0))
KERNEL = "k_align_p<17,4>"
# pairs per row: (long launch, launch of at most two rounds) -- a round is one unit (two calls) per slot, 4 096 slots on 256 CUs
PAIRS = {"50k": (50000, 20480, 8192), "5k": (5000, 131072, 8192)}


def workload(ctx, rng, n_pairs, length, div):
    sub, ins, dele = (v / 100.0 for v in div)
    seqs, blens = [], []
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
    return sset, tasks


def one_row(ctx, name, sset, tasks, n, div, reps, carry):
    modes = SETTINGS                       # STRIPS, DIAG, DIAG + gamdp_ctx_set_walk_skip_backoff
    outs = {m: (L.Result * n)() for m in modes}
    first = None
    ms = {m: [] for m in modes}
    stats, different, held = {}, 0, 0
    for rep in range(reps + 1):            # (rep 0 warms up)
        for mode in modes:
            ctx.set_walk_skip_pair(mode[0])
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
                stats[mode] = ctx.walk_skip_pair_stats()
                held = ctx.walk_skip_backoff_stats()["held_pair"]
                pair_tasks = sum(r["tasks"] for r in ctx.launch_info() if r["kernel"] == KERNEL)
    ctx.set_walk_skip_pair(L.WALK_STRIPS)
    ctx.set_walk_skip_backoff(L.WALK_BACKOFF_OFF)
    on, bo = stats[ON], stats[BACKOFF]
    path = "+".join(p for p, k in (("one by one", "launches_one_by_one"), ("side by side", "launches_side_by_side")) if on[k])
    rec = dict(workload=name, calls=n, two_task_calls=pair_tasks, path=path, sub=div[0], ins=div[1], dele=div[2], results_differ=different,
               strips_off=stats[OFF]["strips"], strips_on=on["strips"], strips_backoff=bo["strips"], stats_on=on, stats_backoff=bo, held=held)
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--lengths", default="50k,5k")
    ap.add_argument("--piecewise", action="store_true", help="two more rows per length: the divergence changes along the pair (tests/_piecewise.py), both orders")
    ap.add_argument("--rows", default="", help="only these rows of every workload: indices into DIVERGENCES, the two piecewise rows behind them (e.g. 0,2,5,6)")
    ap.add_argument("--carry", action="store_true")
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    assert args.reps >= 1
    ctx = gam.Context(0)
    rows = []
    print("source %s, %d calls per mode after a warm-up, kernel ms: median (min - max)" % (source_hash(), args.reps), flush=True)
    print("%-16s %-13s %-12s %8s %9s %9s %11s %11s %8s  %-24s %-24s %-24s %s" % ("workload", "sub/ins/del %", "walks", "strips", "strips on", "strips bo",
          "grp skipped", "skipped bo", "held", "ms off", "ms on", "ms on + backoff", "on/off  bo/off"), flush=True)
    divs = list(enumerate(DIVERGENCES)) + ([(len(DIVERGENCES), "piecewise"), (len(DIVERGENCES) + 1, "piecewise rev")] if args.piecewise else [])
    for w in args.lengths.split(","):
        length, n_long, n_short = PAIRS[w]
        for n_full in (n_long, n_short):
            n = max(8, int(n_full * args.scale)) & ~1
            for di, div in divs:
                if args.rows and str(di) not in args.rows.split(","):
                    continue
                rng = np.random.default_rng(20261020 + di)
                if isinstance(div, str):
                    sset, tasks = piecewise_workload(ctx, rng, n, length, div.endswith("rev"), BAND)
                    div = (div, "", "")
                else:
                    sset, tasks = workload(ctx, rng, n, length, div)
                name = "%d x %s" % (n, w.replace("k", " kb"))
                rec = one_row(ctx, name, sset, tasks, n, div, args.reps, args.carry)
                sset.close()
                rows.append(rec)
                f = lambda d: "%.2f (%.2f - %.2f)" % (d["median"], d["min"], d["max"])  # noqa: E731
                print("%-16s %-13s %-12s %8d %9d %9d %11d %11d %8d  %-24s %-24s %-24s %.3f  %.3f%s%s" % (
                    name, div[0] if isinstance(div[0], str) else "%g/%g/%g" % div, rec["path"], rec["strips_off"], rec["strips_on"], rec["strips_backoff"],
                    rec["stats_on"]["groups_skipped"], rec["stats_backoff"]["groups_skipped"], rec["held"], f(rec["ms_off"]), f(rec["ms_on"]),
                    f(rec["ms_backoff"]), rec["ms_on"]["median"] / rec["ms_off"]["median"], rec["ms_backoff"]["median"] / rec["ms_off"]["median"],
                    "  RESULTS DIFFER in %d calls" % rec["results_differ"] if rec["results_differ"] else "",
                    ("  carry mismatches %d" % rec["carry_mismatches"]) if args.carry else ""), flush=True)
    if args.json:
        print(json.dumps(dict(source=source_hash(), reps=args.reps, rows=rows)))
    bad = sum(r["results_differ"] for r in rows) + sum(r.get("carry_mismatches", 0) for r in rows)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
