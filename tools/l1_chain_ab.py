#!/usr/bin/env python3
"""A/B of the merge-block driver's chain modes (gamdp_ctx_set_l1_chain, gamdp_ctx_set_l1_walk_bands): gamdp_align_merge_blocks on the
GAGE-shaped workloads of tests/_gage.py (2.9 Mb and 30 Mb genomes) with the main chains in three modes: "walk" (WALK, a chain kernel
at band 150 only: the default), "carry" (CARRY: k_chain_c) and "walk-any" (WALK with GAMDP_L1_WALK_ANY_BAND: k_chain2 at band 150,
k_chain2g<C> elsewhere).  At band 150 that is kernel against kernel (walk and walk-any are the same launch); at any other band "walk"
means the round loop (one launch and one host round trip per link of every chain), so bands 100 and 300 compare the round loop
with the two chain launches.  The three modes alternate in ONE process, on one context and the same resident sequence sets; per
mode the median and the min-max over the repeats of wall_ms, gpu_busy_ms, rounds, launches (gamdp_ctx_l1_stats) and chain_ms
(gamdp_ctx_l1_chain_stats).  The outputs of the three modes (gamdp_mb_out and the audit arrays) must be identical byte for byte.

    python tools/l1_chain_ab.py [--genomes 2900000,30000000] [--bands 150,100,300] [--repeats 7] [--json]
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

AUDIT = 8   # audit records kept per merge block for the comparison
KEYS = ("wall_ms", "gpu_busy_ms", "chain_ms", "rounds", "launches")


def run(ctx, genome, bands, repeats, seed=1):
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
    modes = (("walk", (L.L1_CHAIN_WALK, L.L1_WALK_BAND_150)), ("carry", (L.L1_CHAIN_CARRY, L.L1_WALK_BAND_150)),
             ("walk-any", (L.L1_CHAIN_WALK, L.L1_WALK_ANY_BAND)))
    recs = []
    st = L.L1Stats()
    for band in bands:
        rows = {name: [] for name, _ in modes}
        last = {}
        first = None
        for rep in range(repeats + 1):   # (the first pass of each mode warms buffers and reverse complements up: not counted)
            for name, (mode, walk_bands) in modes:
                ctx.set_l1_chain(mode)
                ctx.set_l1_walk_bands(walk_bands)
                outs, aud = (L.MbOut * n)(), (L.Result * (n * AUDIT))()
                rc = ctx.lib.gamdp_align_merge_blocks(ctx.handle, masters.handle, slaves.handle, ins, n, band, outs, aud, AUDIT)
                if rc != 0:
                    raise SystemExit("gamdp_align_merge_blocks (band %d, %s chains) failed: %d %s" % (band, name, rc, ctx.last_error()))
                ctx.lib.gamdp_ctx_l1_stats(ctx.handle, C.byref(st))
                ch = ctx.l1_chain_stats()
                if rep:
                    rows[name].append(dict(wall_ms=st.wall_ms, gpu_busy_ms=st.gpu_busy_ms, chain_ms=ch["chain_ms"], rounds=st.rounds, launches=st.launches))
                last[name] = ch
                got = (bytes(outs), bytes(aud))
                if first is None:
                    first = got
                elif first != got:
                    raise SystemExit("band %d, %s chains, repeat %d: the outputs differ from the first call's" % (band, name, rep))
        rec = {"genome": genome, "band": band, "merge_blocks": n, "repeats": repeats, "outputs_identical": True}
        for name, _ in modes:
            r = rec[name] = {}
            for k in KEYS:
                v = [x[k] for x in rows[name]]
                r[k] = statistics.median(v)
                r[k + "_min"], r[k + "_max"] = min(v), max(v)
            for k in ("kernel", "chains", "chain_calls", "round_loop_mbs", "scratch_bytes", "twins", "cols"):
                r[k] = last[name][k]
        recs.append(rec)
    ctx.set_l1_chain(L.L1_CHAIN_WALK)
    ctx.set_l1_walk_bands(L.L1_WALK_BAND_150)
    masters.close()
    slaves.close()
    return recs


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", default="2900000,30000000")
    ap.add_argument("--bands", default="150,100,300")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    if a.repeats < 1:
        raise SystemExit("--repeats must be at least 1")
    import gam_ngs_amd as gam
    ctx = gam.Context(0)
    for g in a.genomes.split(","):
        for rec in run(ctx, int(g), [int(b) for b in a.bands.split(",")], a.repeats):
            if a.json:
                print(json.dumps(rec), flush=True)
                continue
            print("%.1f Mb genome, band %d, %d merge blocks, median (min-max) of %d calls per mode (outputs identical):" % (
                rec["genome"] / 1e6, rec["band"], rec["merge_blocks"], rec["repeats"]))
            print("  %-8s %-16s %7s %26s %26s %24s %7s %9s" % ("chains", "kernel", "chains", "wall_ms", "gpu_busy_ms", "chain_ms", "rounds", "launches"))
            for name in ("walk", "carry", "walk-any"):
                r = rec[name]
                span = lambda k: "%8.2f (%.2f-%.2f)" % (r[k], r[k + "_min"], r[k + "_max"])
                print("  %-8s %-16s %7d %26s %26s %24s %7d %9d" % (name, r["kernel"] or "(round loop)", r["chains"], span("wall_ms"), span("gpu_busy_ms"),
                                                                  span("chain_ms"), r["rounds"], r["launches"]), flush=True)
