"""Times gamdp_find_hits_batch (ABlast::findHits on the GPU) against the host gamdp_find_hits on 16 threads, and checks
every device result against the host's, on three workloads:

  tails    the left / right tail windows of the 2.9 Mb and 30 Mb GAGE-shaped problems (tests/_gage.py), shaped as the
           merge-block driver builds them (gamdp_l1.cpp; tests/_hitsq.py)
  long     1 000 queries of 100 kb x 100 kb (synthetic pairs: master against its diverged slave)
  repeats  500 queries of 5 kb x 5 kb over tandem repeats (units of 1 - 12 bases, some interrupted by random stretches)
  small    the first 1, 4, 16 and 64 tail queries of the 2.9 Mb problem: where a batch call's fixed cost decides

device_kernel_ms is the kernels' time (gamdp_ctx_kernel_time); device_call_ms the whole ABlast.find_hits_many call with the
hit lists, summary_call_ms the call for the summaries alone (hits_buf == NULL); host16_ms the host findHits on 16 threads.
Each is the median of --reps runs after a warm-up call.

One JSON line per workload.  Usage: python tools/find_hits_batch.py [--reps R] [--only tails,long,repeats,small]
"""
import argparse
import ctypes as C
import json
import os
import random
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _gage  # noqa: E402
import _hitsq as H  # noqa: E402
import gam_ngs_amd as gam  # noqa: E402
from gam_ngs_amd import api, lib  # noqa: E402

M64 = (1 << 64) - 1


def host_all(codes, queries, threads=16):
    """host gamdp_find_hits over all queries on `threads` threads: (hit lists, ms)"""
    l = lib.load_library()
    views = {}
    for q in queries:
        for key in ((q[0], q[1], q[2]), (q[5], q[6], q[7])):
            if key not in views:
                views[key] = H.view(codes[key[0]], key[1], key[2])

    def one(q):
        a, b = views[(q[0], q[1], q[2])], views[(q[5], q[6], q[7])]
        cap = len(a) + 1
        buf = (C.c_uint32 * cap)()
        n = l.gamdp_find_hits(a, len(a), q[3] & M64, q[4] & M64, b, len(b), q[8] & M64, q[9] & M64, q[10], buf, cap)
        return list(buf[:n])

    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        out = list(ex.map(one, queries, chunksize=max(1, len(queries) // (8 * threads))))
    return out, (time.perf_counter() - t0) * 1e3


def device_all(ctx, sset, queries, reps):
    ab = gam.ABlast()
    calls = [(sset.contig(q[0], q[1], q[2]), q[3], q[4], sset.contig(q[5], q[6], q[7]), q[8], q[9]) for q in queries]
    words = [q[10] for q in queries]
    hits = ab.find_hits_many(ctx, calls, words=words)   # warm-up, and the lists that are checked
    kms, walls, sums = [], [], []
    for _ in range(reps):
        ctx.kernel_time(reset=True)
        t0 = time.perf_counter()
        ab.find_hits_many(ctx, calls, want_hits=True, words=words)
        walls.append((time.perf_counter() - t0) * 1e3)
        kms.append(ctx.kernel_time()[0])
        t0 = time.perf_counter()
        ab.find_hits_many(ctx, calls, want_hits=False, words=words)
        sums.append((time.perf_counter() - t0) * 1e3)
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    return hits, med(kms), med(walls), med(sums)


def report(name, ctx, codes, queries, reps, sset=None, **extra):
    own = sset is None
    if own:
        sset = gam.SequenceSet(ctx, codes, ascii=False)
    dev, kms, wall, wall_sum = device_all(ctx, sset, queries, reps)
    host, hms = host_all(codes, queries)
    same = dev == host
    bad = next((i for i, (x, y) in enumerate(zip(dev, host)) if x != y), None)
    a_kmers = sum(min(q[4], len(H.view(codes[q[0]], q[1], q[2])) - 1) - q[3] + 1 for q in queries)
    rec = dict(workload=name, queries=len(queries), a_bases=a_kmers, seeded=sum(1 for h in host if h),
               device_kernel_ms=round(kms, 3), device_call_ms=round(wall, 3), summary_call_ms=round(wall_sum, 3),
               host16_ms=round(hms, 3),
               device_queries_per_s=round(len(queries) / (kms / 1e3), 1) if kms else None,
               call_queries_per_s=round(len(queries) / (wall / 1e3), 1),
               host16_queries_per_s=round(len(queries) / (hms / 1e3), 1), identical=same, first_mismatch=bad, **extra)
    print(json.dumps(rec), flush=True)
    if own:
        sset.close()
    return same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="tails,long,repeats")
    args = ap.parse_args()
    todo = args.only.split(",")
    ctx = gam.Context(0)
    ok = True
    if "tails" in todo:
        for label, glen in (("tails_2.9Mb", 2_900_000), ("tails_30Mb", 30_000_000)):
            codes, queries = H.tail_queries(_gage.problem(3, genome_len=glen))
            ok &= report(label, ctx, codes, queries, args.reps)
    if "long" in todo:
        n, L = 1000, 100_000
        syn = gam.SequenceSet.synthetic(ctx, 0, n, L)
        codes = []
        for k in range(n):
            m, s = api.synth_pair(k, L)
            codes += [m, s]
        queries = [(2 * k + 1, False, 0, 0, M64, 2 * k, False, 0, 0, M64, 20) for k in range(n)]
        ok &= report("long_100kb", ctx, codes, queries, args.reps, sset=syn)
        syn.close()
    if "repeats" in todo:
        rng = random.Random(12)
        codes, queries = [], []
        for k in range(500):
            unit = "".join(rng.choice("ACGT") for _ in range(rng.randint(1, 12)))
            a = (unit * (5000 // len(unit) + 1))[:5000]
            if rng.random() < 0.5:   # interrupted by random stretches
                a = "".join(ch if (i // 400) % 3 else rng.choice("ACGT") for i, ch in enumerate(a))
            b = a[rng.randint(0, 100):]
            codes += [api.encode(a), api.encode(b)]
            queries.append((2 * k, False, 0, 0, M64, 2 * k + 1, False, 0, 0, M64, 20))
        ok &= report("repeats_5kb", ctx, codes, queries, max(1, args.reps // 2))
    if "small" in todo:
        codes, queries = H.tail_queries(_gage.problem(3))
        sset = gam.SequenceSet(ctx, codes, ascii=False)
        for k in (1, 4, 16, 64):
            ok &= report("tails_2.9Mb_first%d" % k, ctx, codes, queries[:k], args.reps, sset=sset)
        sset.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
