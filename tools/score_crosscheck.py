"""Cross-checks gamdp_align_batch against gamdp_score_batch on the device both ran on, and times them.

gamdp_score_batch (gam_ngs_amd/csrc/gamdp_score.hip) computes score, status and cells of every call with a second kernel, in int32,
that shares no code with the alignment kernels -- the packed-f16 ones included, whose exactness rests on a range argument only the
diagnostics build asserts.  This tool runs both calls on one workload in one process, asserts that score,
status and cells agree for every task, and prints one JSON line: the task count, the mismatches (must be 0), the kernels
gamdp_align_batch launched, and each call's kernel time (gamdp_ctx_kernel_time) over --reps alternating repetitions.  It reads
nothing but the package and tests/_mixed.py.

With --carry a third call, gamdp_carry_batch (gam_ngs_amd/csrc/gamdp_carry.hip: the whole result from a fill in which every cell
carries the summary of the traceback that would start in it), checks the other half: every field of every gamdp_result -- begin,
score, n_match, length, first and last match, homology, status -- and cells must equal gamdp_align_batch's; the line then also holds
carry_mismatches, carry_kernels, carry_kernel_ms and carry_gcups.  Without the flag the output is what it was.
--carry --walk-skip-pair / --walk-skip-i32: gamdp_align_batch runs with that walk-skip property on (gamdp_ctx_set_walk_skip_pair,
gamdp_ctx_set_walk_skip_i32), so every field of its results is checked against a kernel that has no walk at all; the line then
also holds the property's statistics of the last call.  --walk-skip does the same for the eight-task kernel (gamdp_ctx_set_walk_skip), and
--walk-skip-backoff switches gamdp_ctx_set_walk_skip_backoff on beside whichever of the three is given (walk_skip_backoff: its statistics).

With --ops the edit strings are checked too.  gamdp_align_batch runs once more with edit strings (one buffer of |a| + |b| + 2 band +
64 bytes per call, on the device and on the host: what limits the batch), the host fingerprints the bytes it returned
(gamdp_ops_fingerprint), and gamdp_carry_ops_batch (gam_ngs_amd/csrc/gamdp_carry_ops.hip: the carry kernel with the fingerprint of
the edit string as a sixth field of a cell's summary) gives the fingerprint of the string the reference would return: both must
agree call by call, as must every field of the two results.  The line then also holds ops_mismatches, ops_first_mismatch (the call
and both values), ops_kernels, ops_kernel_ms (k_carry_f), align_ops_kernel_ms (gamdp_align_batch with edit strings; align_kernel_ms
is the same call without), ops_bytes and ops_gcups.

With --ops --device-fp the align side's fingerprints come from gamdp_align_batch_fp instead: the edit strings stay on the device, in
rooms of gamdp_task_ops_cap bytes, k_ops_fp (gam_ngs_amd/csrc/gamdp_ops_fp.hip) folds them there and 4 bytes per call come back, the
batch in chunks of the context's ops budget (--ops-chunk-bytes; 1 GiB by default) -- so no buffer of the batch's edit strings exists
anywhere and the batch may be of any size.  The line then also holds device_fp_mismatches (against gamdp_carry_ops_batch, as
ops_mismatches), align_fp_kernel_ms (all launches of the call), ops_fp_kernel_ms (k_ops_fp alone), ops_fp_info (gamdp_ctx_ops_fp_info
of the last repetition), align_fp_wall_ms (the whole call) and align_fp_bytes_to_host.  --host-fp-too runs the download path of plain
--ops beside it in every repetition, the two alternating (align_ops_wall_ms: the call, the reversal inside it and the host's
fingerprints; align_ops_bytes_to_host), for measurements of one against the other in one process.

With --ops --ops-walk-runs every call that returns or fingerprints edit strings runs twice in each repetition, alternating on the one
context: in GAMDP_OPS_WALK_STEPS and in GAMDP_OPS_WALK_RUNS mode (gamdp_ctx_set_ops_walk: the walks write the strings a diagonal run at
a time).  Both modes are compared with gamdp_carry_ops_batch (the mismatch counts cover both); the usual keys hold the STEPS figures, and
ops_walk_runs holds the RUNS ones -- the same kernel-time lists, align_fp_launch_ms (the alignment launches alone: the call without
k_ops_fp; align_fp_launch_ms at the top level is STEPS's, align_kernel_ms the same launches without strings) and
gamdp_ctx_ops_walk_stats of the last call.

Workloads:  --pairs N --len L --band B   N synthetic pairs of L bases (SequenceSet.synthetic), whole-sequence windows
            --mixed N                    N calls shaped like the merge-block driver's (tests/_mixed.py), band --band (default 150)

The planner switches of DESIGN.md section 6 apply to gamdp_align_batch as always (read once per process): with
GAMDP_NO_PAIR=1 GAMDP_QUAD_MIN=1000000000 in the environment it stays on the one-task int32 kernels.

Usage: python tools/score_crosscheck.py --pairs 4096 --len 50000 --band 150 [--carry] [--ops [--device-fp [--host-fp-too]]] [--reps 5] [--first-pair K]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gam_ngs_amd as gam  # noqa: E402
from gam_ngs_amd import lib as L  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=0)
    ap.add_argument("--len", type=int, default=50000)
    ap.add_argument("--band", type=int, default=150)
    ap.add_argument("--mixed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--first-pair", type=int, default=0)
    ap.add_argument("--seed", type=int, default=20261019)
    ap.add_argument("--carry", action="store_true", help="also run gamdp_carry_batch and compare whole results")
    ap.add_argument("--walk-skip", action="store_true", help="with --carry: gamdp_align_batch runs with gamdp_ctx_set_walk_skip(GAMDP_WALK_SKIP_DIAG)")
    ap.add_argument("--walk-skip-backoff", action="store_true", help="with one of --walk-skip, --walk-skip-pair, --walk-skip-i32: gamdp_ctx_set_walk_skip_backoff(GAMDP_WALK_BACKOFF_ON)")
    ap.add_argument("--walk-skip-pair", action="store_true", help="with --carry: gamdp_align_batch runs with gamdp_ctx_set_walk_skip_pair(GAMDP_WALK_SKIP_DIAG)")
    ap.add_argument("--walk-skip-i32", action="store_true", help="with --carry: gamdp_align_batch runs with gamdp_ctx_set_walk_skip_i32(GAMDP_WALK_SKIP_DIAG)")
    ap.add_argument("--ops", action="store_true", help="also run gamdp_carry_ops_batch and compare the fingerprints of gamdp_align_batch's edit strings")
    ap.add_argument("--device-fp", action="store_true", help="with --ops: the align side's fingerprints from gamdp_align_batch_fp (the strings stay on the device)")
    ap.add_argument("--host-fp-too", action="store_true", help="with --ops --device-fp: also the download path of plain --ops, alternating with it")
    ap.add_argument("--ops-walk-runs", action="store_true", help="with --ops: every edit-string call in GAMDP_OPS_WALK_STEPS and GAMDP_OPS_WALK_RUNS mode, alternating")
    ap.add_argument("--ops-chunk-bytes", type=int, default=0, help="gamdp_ctx_set_ops_chunk_bytes (0: the default, 1 GiB)")
    args = ap.parse_args()
    if (args.device_fp and not args.ops) or (args.host_fp_too and not args.device_fp):
        ap.error("--device-fp goes with --ops, --host-fp-too with --device-fp")
    if args.ops_walk_runs and not args.ops:
        ap.error("--ops-walk-runs goes with --ops")
    if bool(args.pairs) == bool(args.mixed):
        ap.error("one of --pairs N or --mixed N")
    if args.walk_skip_pair and not args.carry:
        ap.error("--walk-skip-pair goes with --carry")
    if args.walk_skip_i32 and not args.carry:
        ap.error("--walk-skip-i32 goes with --carry")
    if args.walk_skip and not args.carry:
        ap.error("--walk-skip goes with --carry")
    if args.walk_skip_backoff and not (args.walk_skip or args.walk_skip_pair or args.walk_skip_i32):
        ap.error("--walk-skip-backoff goes with --walk-skip, --walk-skip-pair or --walk-skip-i32")
    ctx = gam.Context(0)
    skip_octo = skip_backoff = None
    if args.walk_skip:        # the eight-task kernel's walks jump over indel-free groups
        ctx.set_walk_skip(L.WALK_SKIP_DIAG)
    if args.walk_skip_backoff:   # ... and the walks of whichever kernels test back off after failures
        ctx.set_walk_skip_backoff(L.WALK_BACKOFF_ON)
    skip_pair = None
    if args.walk_skip_pair:   # the two-task kernel's walks jump over indel-free groups: checked call by call against gamdp_carry_batch
        ctx.set_walk_skip_pair(L.WALK_SKIP_DIAG)
    skip_i32 = None
    if args.walk_skip_i32:    # ... and those of the int32 direction-free kernels
        ctx.set_walk_skip_i32(L.WALK_SKIP_DIAG)
    if args.mixed:
        import _mixed
        seqs, calls = _mixed.mixed_batch(args.seed, max(1, args.mixed // 8), 8, band=args.band)
        n = len(calls)
        sset = gam.SequenceSet(ctx, seqs, ascii=False)
        tasks = (L.Task * n)()
        _mixed.fill_tasks(tasks, calls)
        workload = dict(workload="mixed", calls=n, band=args.band, seed=args.seed)
    else:
        n = args.pairs
        sset = gam.SequenceSet.synthetic(ctx, args.first_pair, n, args.len)
        tasks = (L.Task * n)()
        for k in range(n):
            t = tasks[k]
            t.a_id, t.b_id, t.band = 2 * k, 2 * k + 1, args.band
            t.begin_a, t.end_a, t.begin_b, t.end_b = 0, args.len - 1, 0, sset.lengths[2 * k + 1] - 1
        workload = dict(workload="pairs", pairs=n, len=args.len, band=args.band)
    res, sc = (L.Result * n)(), (L.ScoreResult * n)()
    ca = (L.Result * n)() if args.carry else None
    align_ms, score_ms, carry_ms = [], [], []
    host_fp_path = args.ops and (not args.device_fp or args.host_fp_too)
    if args.ops:
        res_o, res_f, fp = (L.Result * n)(), (L.Result * n)(), (C.c_uint32 * n)()
        ops_bytes = 0
    if args.device_fp:
        res_d, fp_d = (L.Result * n)(), (C.c_uint32 * n)()
        ctx.set_ops_chunk_bytes(args.ops_chunk_bytes)
    # (--ops-walk-runs: the lists of the second mode, RUNS, are the ones with index 1)
    walk_modes = (L.OPS_WALK_STEPS, L.OPS_WALK_RUNS) if args.ops_walk_runs else (None,)
    per_mode = lambda: tuple([] for _ in walk_modes)  # noqa: E731
    dev_ms_m, dev_fp_ms_m, dev_wall_ms_m, host_wall_ms_m, align_ops_ms_m = per_mode(), per_mode(), per_mode(), per_mode(), per_mode()
    walk_stats = None
    dev_mismatches, dev_first_bad, fp_info = 0, None, None
    if host_fp_path:
        caps = [sset.lengths[t.a_id] + sset.lengths[t.b_id] + 2 * t.band + 64 for t in tasks]
        offs, ops_bytes = [], 0
        for cap in caps:
            offs.append(ops_bytes)
            ops_bytes += cap
        buf = C.create_string_buffer(max(1, ops_bytes))
        buf_addr = C.addressof(buf)
        ops_struct = L.Ops(C.cast(buf, C.c_void_p), (C.c_uint64 * n)(*offs), (C.c_uint64 * n)(*caps))
    ops_ms = []
    ops_mismatches, ops_first_bad = 0, None
    mismatches, first_bad = 0, None
    carry_mismatches, carry_first_bad = 0, None
    whole = lambda r: r.key() + (r.cells,)  # noqa: E731
    for rep in range(args.reps + 1):   # (the first pass warms up: buffers, reverse complements, code objects)
        ctx.kernel_time(reset=True)
        rc = ctx.lib.gamdp_align_batch(ctx.handle, sset.handle, sset.handle, tasks, n, res, None)
        assert rc == 0, ("gamdp_align_batch", rc, ctx.last_error())
        a_ms = ctx.kernel_time(reset=True)[0]
        if args.walk_skip:
            skip_octo = ctx.walk_skip_stats()
        if args.walk_skip_backoff:
            skip_backoff = ctx.walk_skip_backoff_stats()
        if args.walk_skip_pair:
            skip_pair = ctx.walk_skip_pair_stats()
        if args.walk_skip_i32:
            skip_i32 = ctx.walk_skip_i32_stats()
        rc = ctx.lib.gamdp_score_batch(ctx.handle, sset.handle, sset.handle, tasks, n, sc)
        assert rc == 0, ("gamdp_score_batch", rc, ctx.last_error())
        s_ms = ctx.kernel_time(reset=True)[0]
        if args.carry:
            rc = ctx.lib.gamdp_carry_batch(ctx.handle, sset.handle, sset.handle, tasks, n, ca)
            assert rc == 0, ("gamdp_carry_batch", rc, ctx.last_error())
            c_ms = ctx.kernel_time(reset=True)[0]
        if args.ops:
            rc = ctx.lib.gamdp_carry_ops_batch(ctx.handle, sset.handle, sset.handle, tasks, n, res_f, fp)
            assert rc == 0, ("gamdp_carry_ops_batch", rc, ctx.last_error())
            f_ms = ctx.kernel_time(reset=True)[0]
            if rep:
                ops_ms.append(f_ms)
        for m, mode in enumerate(walk_modes if host_fp_path else ()):
            if mode is not None:
                ctx.set_ops_walk(mode)
            t0 = time.perf_counter()
            rc = ctx.lib.gamdp_align_batch(ctx.handle, sset.handle, sset.handle, tasks, n, res_o, C.byref(ops_struct))
            assert rc == 0, ("gamdp_align_batch with edit strings", rc, ctx.last_error())
            host_fps = [ctx.lib.gamdp_ops_fingerprint(C.c_char_p(buf_addr + offs[i]), res_o[i].length) if res_o[i].status == 0 else 0 for i in range(n)]
            wall = (time.perf_counter() - t0) * 1e3
            ao_ms = ctx.kernel_time(reset=True)[0]
            if mode == L.OPS_WALK_RUNS:
                walk_stats = ctx.ops_walk_stats()
            if rep:
                align_ops_ms_m[m].append(ao_ms)
                host_wall_ms_m[m].append(wall)
            for i in range(n):   # (a status other than OK has no edit string: fingerprint 0 on both sides)
                if host_fps[i] != fp[i] or whole(res_o[i]) != whole(res_f[i]):
                    ops_mismatches += 1
                    if ops_first_bad is None:
                        ops_first_bad = dict(task=i, align_fp=host_fps[i], carry_fp=fp[i], align=whole(res_o[i]), carry=whole(res_f[i]))
        for m, mode in enumerate(walk_modes if args.device_fp else ()):
            if mode is not None:
                ctx.set_ops_walk(mode)
            t0 = time.perf_counter()
            rc = ctx.lib.gamdp_align_batch_fp(ctx.handle, sset.handle, sset.handle, tasks, n, res_d, fp_d)
            wall = (time.perf_counter() - t0) * 1e3
            assert rc == 0, ("gamdp_align_batch_fp", rc, ctx.last_error())
            d_ms = ctx.kernel_time(reset=True)[0]
            fp_info = ctx.ops_fp_info()
            if mode == L.OPS_WALK_RUNS:
                walk_stats = ctx.ops_walk_stats()
            if rep:
                dev_ms_m[m].append(d_ms)
                dev_fp_ms_m[m].append(fp_info["kernel_ms"])
                dev_wall_ms_m[m].append(wall)
            for i in range(n):
                if fp_d[i] != fp[i] or whole(res_d[i]) != whole(res_f[i]):
                    dev_mismatches += 1
                    if dev_first_bad is None:
                        dev_first_bad = dict(task=i, align_fp=fp_d[i], carry_fp=fp[i], align=whole(res_d[i]), carry=whole(res_f[i]))
        if args.ops_walk_runs:
            ctx.set_ops_walk(L.OPS_WALK_STEPS)
        if rep:
            align_ms.append(a_ms)
            score_ms.append(s_ms)
            if args.carry:
                carry_ms.append(c_ms)
        for i in range(n):
            if (res[i].score, res[i].status, res[i].cells) != (sc[i].score, sc[i].status, sc[i].cells):
                mismatches += 1
                if first_bad is None:
                    first_bad = dict(task=i, align=(res[i].score, res[i].status, res[i].cells), score=(sc[i].score, sc[i].status, sc[i].cells))
            if args.carry and whole(res[i]) != whole(ca[i]):
                carry_mismatches += 1
                if carry_first_bad is None:
                    carry_first_bad = dict(task=i, align=whole(res[i]), carry=whole(ca[i]))
    cells = sum(r.cells for r in res)
    dev_ms, dev_fp_ms, dev_wall_ms, host_wall_ms, align_ops_ms = dev_ms_m[0], dev_fp_ms_m[0], dev_wall_ms_m[0], host_wall_ms_m[0], align_ops_ms_m[0]
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    rec = dict(workload, tasks=n, mismatches=mismatches, first_mismatch=first_bad, ok=sum(1 for r in res if r.status == 0), cells=cells,
               align_kernels=sorted({r["kernel"] for r in ctx.launch_info()}), score_kernels=[r["kernel"] for r in ctx.score_info()],
               align_kernel_ms=[round(v, 3) for v in align_ms], score_kernel_ms=[round(v, 3) for v in score_ms],
               align_gcups=round(cells / med(align_ms) / 1e6, 1), score_gcups=round(cells / med(score_ms) / 1e6, 1))
    if args.carry:
        rec.update(carry_mismatches=carry_mismatches, carry_first_mismatch=carry_first_bad, carry_kernels=[r["kernel"] for r in ctx.carry_info()],
                   carry_kernel_ms=[round(v, 3) for v in carry_ms], carry_gcups=round(cells / med(carry_ms) / 1e6, 1))
    if args.walk_skip:
        rec.update(walk_skip=skip_octo)
    if args.walk_skip_backoff:
        rec.update(walk_skip_backoff=skip_backoff)
    if args.walk_skip_pair:
        rec.update(walk_skip_pair=skip_pair)
    if args.walk_skip_i32:
        rec.update(walk_skip_i32=skip_i32)
    if args.ops:
        rec.update(ops_mismatches=ops_mismatches, ops_first_mismatch=ops_first_bad, ops_kernels=[r["kernel"] for r in ctx.carry_ops_info()],
                   ops_kernel_ms=[round(v, 3) for v in ops_ms], align_ops_kernel_ms=[round(v, 3) for v in align_ops_ms],
                   ops_bytes=ops_bytes, ops_gcups=round(cells / med(ops_ms) / 1e6, 1))
    if host_fp_path and args.device_fp:
        rec.update(align_ops_wall_ms=[round(v, 2) for v in host_wall_ms], align_ops_bytes_to_host=ops_bytes + 40 * n)
    if args.device_fp:
        gbs = fp_info["bytes"] / (med(dev_fp_ms) * 1e6) if med(dev_fp_ms) > 0 else None
        rec.update(device_fp_mismatches=dev_mismatches, device_fp_first_mismatch=dev_first_bad, align_fp_kernel_ms=[round(v, 3) for v in dev_ms],
                   ops_fp_kernel_ms=[round(v, 4) for v in dev_fp_ms], ops_fp_info=fp_info, ops_fp_gb_per_s=round(gbs, 1) if gbs else None,
                   align_fp_wall_ms=[round(v, 2) for v in dev_wall_ms], align_fp_bytes_to_host=44 * n)
    launch_ms = lambda call, fold: [round(a - b, 3) for a, b in zip(call, fold)]  # noqa: E731
    if args.device_fp:
        rec.update(align_fp_launch_ms=launch_ms(dev_ms, dev_fp_ms))
    if args.ops_walk_runs:
        runs = dict(stats=walk_stats)
        if host_fp_path:
            runs.update(align_ops_kernel_ms=[round(v, 3) for v in align_ops_ms_m[1]], align_ops_wall_ms=[round(v, 2) for v in host_wall_ms_m[1]])
        if args.device_fp:
            runs.update(align_fp_kernel_ms=[round(v, 3) for v in dev_ms_m[1]], ops_fp_kernel_ms=[round(v, 4) for v in dev_fp_ms_m[1]],
                        align_fp_launch_ms=launch_ms(dev_ms_m[1], dev_fp_ms_m[1]), align_fp_wall_ms=[round(v, 2) for v in dev_wall_ms_m[1]])
        rec.update(ops_walk_runs=runs)
    print(json.dumps(rec), flush=True)
    sset.close()
    sys.exit(0 if mismatches == 0 and carry_mismatches == 0 and ops_mismatches == 0 and dev_mismatches == 0 else 1)


if __name__ == "__main__":
    main()
