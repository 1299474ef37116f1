#!/usr/bin/env python3
"""A/B of the merge-block driver's findHits mode (gamdp_ctx_set_l1_hits): gamdp_align_merge_blocks on the GAGE-shaped workloads
of tests/_gage.py (2.9 Mb and 30 Mb genomes) with the tail alignments seeded on the host and on the device.  The two modes
alternate in ONE process, on one context and the same resident sequence sets; per mode the median over the repeats of wall_ms,
host_pending_ms, gpu_busy_ms (gamdp_ctx_l1_stats) and the hits statistics (gamdp_ctx_l1_hits_stats).  The outputs of the two
modes (gamdp_mb_out and the audit arrays) must be identical byte for byte.

    python tools/l1_hits_ab.py [--genomes 2900000,30000000] [--repeats 7] [--json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

AUDIT = 8   # audit records kept per merge block for the comparison (the tail calls are the last of a trail)


def run(ctx, genome, repeats, seed=1, band=150):
    import _gage
    import bench_l1
    import gam_ngs_amd as gam
    from gam_ngs_amd import lib as L
    pb = _gage.problem(seed, genome_len=genome)
    flat, _ = _gage.merge_blocks(pb)
    masters = gam.SequenceSet(ctx, [bytes(c["seq"]) for c in pb["master"]], ascii=False)
    slaves = gam.SequenceSet(ctx, [bytes(c["seq"]) for c in pb["slave"]], ascii=False)
    ins, keep = bench_l1.marshal(flat)
    n = len(flat)
    modes = (("host", L.L1_HITS_HOST), ("device", L.L1_HITS_DEVICE))
    rows = {name: [] for name, _ in modes}
    outputs = {}
    st = L.L1Stats()
    for rep in range(repeats + 1):   # (the first pass of each mode warms buffers and reverse complements up: not counted)
        for name, mode in modes:
            ctx.set_l1_hits(mode)
            outs, aud = (L.MbOut * n)(), (L.Result * (n * AUDIT))()
            rc = ctx.lib.gamdp_align_merge_blocks(ctx.handle, masters.handle, slaves.handle, ins, n, band, outs, aud, AUDIT)
            if rc != 0:
                raise SystemExit("gamdp_align_merge_blocks (%s hits) failed: %d %s" % (name, rc, ctx.last_error()))
            ctx.lib.gamdp_ctx_l1_stats(ctx.handle, C.byref(st))
            h = ctx.l1_hits_stats()
            if rep:
                rows[name].append(dict(h, wall_ms=st.wall_ms, host_pending_ms=st.host_pending_ms, gpu_busy_ms=st.gpu_busy_ms,
                                       kernel_sum_ms=st.kernel_sum_ms, launches=st.launches, rounds=st.rounds, cohorts=st.cohorts))
            got = (bytes(outs), bytes(aud))
            if outputs.setdefault("first", got) != got:
                raise SystemExit("%s hits, repeat %d: the outputs differ from the first call's" % (name, rep))
    ctx.set_l1_hits(L.L1_HITS_HOST)
    masters.close()
    slaves.close()
    rec = {"genome": genome, "merge_blocks": n, "repeats": repeats, "outputs_identical": True}
    for name, _ in modes:
        rec[name] = {k: statistics.median(r[k] for r in rows[name]) for k in rows[name][0]}
        rec[name]["wall_ms_min"] = min(r["wall_ms"] for r in rows[name])
    return rec


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", default="2900000,30000000")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    import gam_ngs_amd as gam
    ctx = gam.Context(0)
    for g in a.genomes.split(","):
        rec = run(ctx, int(g), a.repeats)
        if a.json:
            print(json.dumps(rec))
            continue
        print("%.1f Mb genome, %d merge blocks, median of %d calls per mode (outputs identical):" % (rec["genome"] / 1e6, rec["merge_blocks"], rec["repeats"]))
        print("  %-7s %9s %9s %16s %12s %8s %8s %8s %9s %9s %14s %12s" % ("hits", "wall_ms", "(min)", "host_pending_ms", "gpu_busy_ms", "launches", "queries",
                                                                  "device", "trivial", "fallback", "hits_kernel_ms", "host_hits_ms"))
        for name in ("host", "device"):
            r = rec[name]
            print("  %-7s %9.2f %9.2f %16.2f %12.2f %8d %8d %8d %9d %9d %14.2f %12.2f" % (
                name, r["wall_ms"], r["wall_ms_min"], r["host_pending_ms"], r["gpu_busy_ms"], r["launches"], r["tail_queries"], r["device_queries"],
                r["trivial_queries"], r["host_fallback"], r["hits_kernel_ms"], r["host_hits_ms"]))
