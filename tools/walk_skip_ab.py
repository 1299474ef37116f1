#!/usr/bin/env python3
"""A/B of the walk modes of a kernel family (gamdp_ctx_set_walk_skip, _pair, _i32): GAMDP_WALK_STRIPS against GAMDP_WALK_SKIP_DIAG and
against GAMDP_WALK_SKIP_DIAG with gamdp_ctx_set_walk_skip_backoff on, alternating call by call in ONE process on ONE context, one
batch per row.

    --family o19   the eight-task kernel k_align_o<19,15>, band 150: 100 000 x 5 kb, 16 384 x 50 kb and the batch shaped like the
                   merge-block driver's calls (tests/_mixed.py), at 3/1/1, 2/0.5/0.5, 0.3/0.1/0.1, 0.05/0.02/0.02 and 0/0/0 per cent
                   substitutions / insertions / deletions (the first is bench.py's config 5).  No planner switch is needed at these
                   sizes (GAMDP_QUAD_MIN is for small batches).
    --family p17   the two-task kernel k_align_p<17,4>, band 512: 50 kb and 5 kb pairs, identical, at 0.04 % indels, at 0.2 % indels
                   and at config 5's divergence, each as a long launch (more than two rounds: the walks run one task after the other,
                   finish_walk) and as a launch of at most two rounds (the two tasks side by side, walk_many) -- which path a row took
                   is read from gamdp_ctx_walk_skip_pair_stats and printed (a scaled-down `long` row may no longer be a long launch).
    --family i32   the int32 direction-free kernels, the same rows once, one kernel per process (the planner's switches are read once
                   per process); the tool says which environment a cell needs and stops when a row's launches are not that kernel's:
        --cell c17     k_align<17,4,false>      band 512   GAMDP_NO_PAIR=1
        --cell c17n    k_align<17,4,true>       band 512   (every pair holds an N)
        --cell q19     k_align_q<19,15,false>   band 150   GAMDP_NO_PAIR=1 GAMDP_QUAD_MIN=1
        --cell q19n    k_align_q<19,15,true>    band 150   GAMDP_QUAD_MIN=1 (every pair holds an N)
        --cell gen9    k_align<9,-1,true>       band 200
        --cell gen17   k_align<17,-1,true>      band 300

The pairs are made here, in numpy (gamdp_synth_pair's rates are fixed).  Per row: a warm-up call in every mode, then --reps calls per
mode, alternating; kernel time from gamdp_ctx_kernel_time; median and min - max per mode; every call's results are compared byte for
byte with the first call's; the device's counts (the family's gamdp_ctx_walk_skip*_stats, gamdp_ctx_walk_skip_backoff_stats,
gamdp_ctx_launch_info) of a call in every mode.  With --carry every row also runs gamdp_carry_batch once -- a kernel without any walk
-- and compares whole results with it.  --piecewise adds two rows per pair workload: pairs whose divergence changes along the pair
(tests/_piecewise.py), in both orders; --rows picks rows by index.

    python tools/walk_skip_ab.py --family o19 [--reps 7] [--scale 1.0] [--workloads 5k,50k,mixed] [--piecewise] [--rows 0,2,5,6] [--carry] [--json]
    python tools/walk_skip_ab.py --family p17 [--reps 5] [--scale 1.0] [--lengths 50k,5k] [--piecewise] [--rows 0,3,4,5] [--carry] [--json]
    python tools/walk_skip_ab.py --family i32 --cell gen9 [--reps 5] [--scale 1.0] [--lengths 50k,5k] [--piecewise] [--rows 0,3,4,5] [--carry] [--json]

--scale shrinks the pair counts (a quick look; the tables of DESIGN.md section 6 are --scale 1)."""
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

# the three columns: (the family's property, gamdp_ctx_set_walk_skip_backoff)
OFF, ON, BACKOFF = (L.WALK_STRIPS, L.WALK_BACKOFF_OFF), (L.WALK_SKIP_DIAG, L.WALK_BACKOFF_OFF), (L.WALK_SKIP_DIAG, L.WALK_BACKOFF_ON)
SETTINGS = (OFF, ON, BACKOFF)
INDELS = ((0.0, 0.0, 0.0), (0.0, 0.02, 0.02), (0.0, 0.1, 0.1), (3.0, 1.0, 1.0))
# i32: cell -> (kernel, band, every pair holds an N, environment)
CELLS = {
    "c17":   ("k_align<17,4,false>", 512, False, {"GAMDP_NO_PAIR": "1"}),
    "c17n":  ("k_align<17,4,true>", 512, True, {}),
    "q19":   ("k_align_q<19,15,false>", 150, False, {"GAMDP_NO_PAIR": "1", "GAMDP_QUAD_MIN": "1"}),
    "q19n":  ("k_align_q<19,15,true>", 150, True, {"GAMDP_QUAD_MIN": "1"}),
    "gen9":  ("k_align<9,-1,true>", 200, False, {}),
    "gen17": ("k_align<17,-1,true>", 300, False, {}),
}
# prop: Context.set_<prop> / Context.<prop>_stats; held: its field of the backoff statistics; pairs: workload -> (length, pairs per row:
# p17 has a long launch and one of at most two rounds -- a round is one unit (two calls) per slot, 4 096 slots on 256 CUs); mixed: calls
# of the driver-shaped workload; even: pair counts are rounded down to a multiple of it; tasks_key: the record's count of the kernel's
# tasks; launch_strips: the strips columns count every launch of the call (the mixed workload has other kernels), not the family's alone
FAMILIES = {
    "o19": dict(prop="walk_skip", held="held", kernel="k_align_o<19,15>", band=150, seed=20261019, reps=7, workloads="5k,50k,mixed",
                divergences=((3.0, 1.0, 1.0), (2.0, 0.5, 0.5), (0.3, 0.1, 0.1), (0.05, 0.02, 0.02), (0.0, 0.0, 0.0)),
                pairs={"5k": (5000, (100000,)), "50k": (50000, (16384,))}, mixed=12500, even=1, tasks_key="eight_task_calls", launch_strips=True),
    "p17": dict(prop="walk_skip_pair", held="held_pair", kernel="k_align_p<17,4>", band=512, seed=20261020, reps=5, workloads="50k,5k",
                divergences=INDELS, pairs={"50k": (50000, (20480, 8192)), "5k": (5000, (131072, 8192))}, even=2, tasks_key="two_task_calls",
                path=True),
    "i32": dict(prop="walk_skip_i32", held="held_i32", seed=20261020, reps=5, workloads="50k,5k", divergences=INDELS,
                pairs={"50k": (50000, (4096,)), "5k": (5000, (32768,))}, even=4, alone=True),
}


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


def workload(ctx, rng, n_pairs, length, div, band, with_n=False):
    sub, ins, dele = (v / 100.0 for v in div)
    seqs, blens = [], []
    step = max(1, (32 << 20) // length)    # ~32 M bases at a time
    for first in range(0, n_pairs, step):
        n = min(step, n_pairs - first)
        A = rng.integers(0, 4, n * length, dtype=np.uint8)
        Bs, lens = diverged(rng, A, n, length, sub, ins, dele)
        if with_n:                         # one N in the middle of every a: the call goes to the N-aware kernel, the path crosses an N-base pair
            A[length // 2::length] = 4
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
        t.a_id, t.b_id, t.band = 2 * k, 2 * k + 1, band
        t.begin_a, t.end_a, t.begin_b, t.end_b = 0, length - 1, 0, max(blens[k], 1) - 1
    return sset, tasks


def piecewise_workload(ctx, rng, n_pairs, length, reverse, band):
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


def one_row(ctx, fam, name, sset, tasks, n, div, reps, carry):
    setter, getter = getattr(ctx, "set_" + fam["prop"]), getattr(ctx, fam["prop"] + "_stats")
    outs = {m: (L.Result * n)() for m in SETTINGS}
    first = None
    ms = {m: [] for m in SETTINGS}
    stats, strips, different, held = {}, {}, 0, 0
    for rep in range(reps + 1):            # (rep 0 warms up)
        for mode in SETTINGS:
            setter(mode[0])
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
                stats[mode] = getter()
                info = ctx.launch_info()
                strips[mode] = sum(r["strips"] for r in info) if fam.get("launch_strips") else stats[mode]["strips"]
                held = ctx.walk_skip_backoff_stats()[fam["held"]]
    setter(L.WALK_STRIPS)
    ctx.set_walk_skip_backoff(L.WALK_BACKOFF_OFF)
    kernels = sorted({r["kernel"] for r in info})
    if fam.get("alone") and kernels != [fam["kernel"]]:
        sys.exit("the row ran %s, not %s alone: set the cell's environment (see --help)" % (kernels, fam["kernel"]))
    on, bo = stats[ON], stats[BACKOFF]
    rec = dict(workload=name, calls=n)
    if "tasks_key" in fam:
        rec[fam["tasks_key"]] = sum(r["tasks"] for r in info if r["kernel"] == fam["kernel"])
    if fam.get("path"):
        rec["path"] = "+".join(p for p, k in (("one by one", "launches_one_by_one"), ("side by side", "launches_side_by_side")) if on[k])
    if fam.get("alone"):
        rec["kernel"] = fam["kernel"]
    rec.update(sub=div[0], ins=div[1], dele=div[2], results_differ=different, strips_off=strips[OFF], strips_on=strips[ON],
               strips_backoff=strips[BACKOFF], stats_on=on, stats_backoff=bo, held=held)
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


def print_row(fam, rec, div, carry):
    """one line of the table (rec None: its header); the family's extra column is the walk path of the two-task kernel"""
    extra = [("%-12s", "walks", rec and rec["path"])] if fam.get("path") else []
    f = lambda d: "%.2f (%.2f - %.2f)" % (d["median"], d["min"], d["max"])  # noqa: E731
    cols = [("%-16s", "workload", rec and rec["workload"]), ("%-15s", "sub/ins/del %", rec and (div[0] if isinstance(div[0], str) else "%g/%g/%g" % div))] + extra + [
        ("%9s", "strips", rec and rec["strips_off"]), ("%9s", "strips on", rec and rec["strips_on"]), ("%9s", "strips bo", rec and rec["strips_backoff"]),
        ("%12s", "grp skipped", rec and rec["stats_on"]["groups_skipped"]), ("%12s", "skipped bo", rec and rec["stats_backoff"]["groups_skipped"]),
        ("%9s ", "held", rec and rec["held"]), ("%-24s", "ms off", rec and f(rec["ms_off"])), ("%-24s", "ms on", rec and f(rec["ms_on"])),
        ("%-24s", "ms on + backoff", rec and f(rec["ms_backoff"]))]
    line = " ".join(fmt % (head if rec is None else val) for fmt, head, val in cols)
    if rec is None:
        line += " on/off  bo/off"
    else:
        line += " %.3f  %.3f" % (rec["ms_on"]["median"] / rec["ms_off"]["median"], rec["ms_backoff"]["median"] / rec["ms_off"]["median"])
        line += "  RESULTS DIFFER in %d calls" % rec["results_differ"] if rec["results_differ"] else ""
        line += ("  carry mismatches %d" % rec["carry_mismatches"]) if carry else ""
    print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", required=True, choices=sorted(FAMILIES))
    ap.add_argument("--cell", choices=sorted(CELLS), help="--family i32: the kernel")
    ap.add_argument("--reps", type=int, default=0, help="calls per mode (default: 7 for o19, 5 otherwise)")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--workloads", "--lengths", dest="workloads", default="", help="default: 5k,50k,mixed for o19, 50k,5k otherwise")
    ap.add_argument("--piecewise", action="store_true", help="two more rows per pair workload: the divergence changes along the pair (tests/_piecewise.py), both orders")
    ap.add_argument("--rows", default="", help="only these rows of every workload: indices into the family's divergences, the two piecewise rows behind them (e.g. 0,2,5,6)")
    ap.add_argument("--carry", action="store_true")
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    fam = dict(FAMILIES[args.family])
    reps = args.reps or fam["reps"]
    assert reps >= 1
    with_n, top = False, {}
    if args.family == "i32":
        if not args.cell:
            ap.error("--family i32 needs --cell")
        fam["kernel"], fam["band"], with_n, env = CELLS[args.cell]
        missing = {k: v for k, v in env.items() if os.environ.get(k) != v}
        if missing:
            sys.exit("--cell %s needs %s in the environment" % (args.cell, " ".join("%s=%s" % kv for kv in sorted(missing.items()))))
        top = dict(cell=args.cell, kernel=fam["kernel"], band=fam["band"])
    ctx = gam.Context(0)
    rows = []
    print("source %s, %s band %d, %d calls per mode after a warm-up, kernel ms: median (min - max)" % (source_hash(), fam["kernel"], fam["band"], reps), flush=True)
    print_row(fam, None, None, args.carry)
    divergences = fam["divergences"]
    piecewise = [(len(divergences), "piecewise"), (len(divergences) + 1, "piecewise rev")] if args.piecewise and not with_n else []
    for w in (args.workloads or fam["workloads"]).split(","):
        length, counts = fam["pairs"].get(w, (0, (fam.get("mixed"),)))
        for n_full in counts:
            n = max(8, int(n_full * args.scale)) // fam["even"] * fam["even"]
            for di, div in list(enumerate(divergences)) + (piecewise if length else []):
                if args.rows and str(di) not in args.rows.split(","):
                    continue
                rng = np.random.default_rng(fam["seed"] + di)
                if not length:
                    sset, tasks, n_calls = mixed_workload(ctx, n, div)
                    name = "mixed150 %d" % n_calls
                elif isinstance(div, str):
                    sset, tasks = piecewise_workload(ctx, rng, n, length, div.endswith("rev"), fam["band"])
                    div = (div, "", "")
                else:
                    sset, tasks = workload(ctx, rng, n, length, div, fam["band"], with_n)
                if length:
                    n_calls, name = n, "%d x %s" % (n, w.replace("k", " kb"))
                rec = one_row(ctx, fam, name, sset, tasks, n_calls, div, reps, args.carry)
                sset.close()
                rows.append(rec)
                print_row(fam, rec, div, args.carry)
    if args.json:
        print(json.dumps(dict(source=source_hash(), **top, reps=reps, rows=rows)))
    bad = sum(r["results_differ"] for r in rows) + sum(r.get("carry_mismatches", 0) for r in rows)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
