"""Helpers of tests/test_gpu_l1_device_hits.py: one gamdp_align_merge_blocks call over a group of tests/test_l1_oracle_vs_ref.py
with the raw output arrays kept, the comparison with the stored reference answers, the number of tail calls an audit trail
holds, the scratch a tail's findHits query needs -- and, run as a script, the same in a fresh process (the environment
switches are read once per process):

    python tests/_l1hits.py GROUP[,GROUP...]|seed-case setter|env   ->  one JSON line
"""
import ctypes as C
import json
import sys

import _l1ref as R
import test_l1_oracle_vs_ref as T

WORD = 20   # ABlast's word size in PctgBuilder.cc:1544, 1584


def raw_call(c, cases):
    """(bytes of the gamdp_mb_out array, bytes of the audit array, answers) of ONE call over `cases` on context c (a Context, or
    a MultiContext).  An answer is (outcome dict, trail keys, seeds): seeds = [(right, begin_a)] of the merge block's tail calls as
    gamdp_ctx_l1_tail_calls reports them (None on a MultiContext, whose contexts number their own shares)."""
    import gam_ngs_amd as gam
    from gam_ngs_amd import lib as L
    multi = isinstance(c, gam.MultiContext)
    Set = gam.MultiSequenceSet if multi else gam.SequenceSet
    masters = Set(c, [sc["master"].encode() for sc in cases])
    slaves = Set(c, [sc["slave"].encode() for sc in cases])
    n, cap = len(cases), T.AUDIT_CAP
    ins, keep = (L.MbIn * n)(), []
    for i, sc in enumerate(cases):
        arr = (L.BlockC * max(1, len(sc["blocks"])))()
        for k, b in enumerate(sc["blocks"]):
            arr[k].m_begin, arr[k].m_end, arr[k].s_begin, arr[k].s_end = b[0], b[1], b[2], b[3]
            arr[k].m_strand, arr[k].s_strand, arr[k].n_reads = b[4].encode(), b[5].encode(), b[6]
        keep.append(arr)
        x = ins[i]
        x.m_id = x.s_id = i
        x.m_ltail, x.m_rtail, x.s_ltail, x.s_rtail = [int(t) for t in sc["tails"]]
        x.n_blocks, x.blocks = len(sc["blocks"]), C.cast(arr, C.POINTER(L.BlockC))
    outs, aud = (L.MbOut * n)(), (L.Result * (n * cap))()
    if multi:
        rc = c.lib.gamdp_multi_align_merge_blocks(c.handle, masters.handle, slaves.handle, ins, n, 150, outs, aud, cap)
        assert rc == 0, c.last_error()
    else:
        rc = c.lib.gamdp_align_merge_blocks(c.handle, masters.handle, slaves.handle, ins, n, 150, outs, aud, cap)
        assert rc == 0, c.last_error()
    seeds = None
    if not multi:
        seeds = [[] for _ in range(n)]
        for mb, right, begin_a, _ in c.l1_tail_calls():
            seeds[mb].append((right, begin_a))
    answers = []
    for i in range(n):
        o = outs[i]
        assert o.n_dp <= cap
        keys = [aud[i * cap + k].key() for k in range(o.n_dp)]
        answers.append((dict(thrown=o.status == 2, align_ok=bool(o.align_ok), coords_set=bool(o.coords_set),
                             align_rev=bool(o.align_rev) if o.coords_set else False, m_start=o.m_start, m_end=o.m_end,
                             s_start=o.s_start, s_end=o.s_end, n_dp=o.n_dp, cells=o.cells, trail_crc=R.trail_crc(keys)), keys,
                        seeds[i] if seeds is not None else None))
    raw = (bytes(outs), bytes(aud))
    masters.close()
    slaves.close()
    return raw[0], raw[1], answers


def tail_calls(sc, keys):
    """How many of a merge block's DP calls (keys: its audit trail) are tail alignments -- each is seeded by one findHits call.
    The main chain is replayed as alignBlocks / findBestAlignment run it (PctgBuilder.cc:1617-1708, 1420-1512): up to two attempts
    of one call per block, an attempt is good when every call has homology >= 95 and the lengths add up to 0.7 of the shortest
    frame (is_good, :1711-1724); the tails follow a good attempt only."""
    n = len(sc["blocks"])
    flen = lambda b, e: 0 if e < b else e - b + 1   # noqa: E731
    thr = int(0.7 * min(min(flen(b[0], b[1]), flen(b[2], b[3])) for b in sc["blocks"])) if n else 0
    used = 0
    for _ in range(2):
        att = keys[used:used + n]
        used += len(att)
        if len(att) < n or any(k[0] in (2, 3) for k in att):
            return 0   # a call threw: the merge block ends there
        if all(k[12] >= 95.0 for k in att) and sum(k[5] for k in att) >= thr:
            return len(keys) - used
    return 0


def query_words(a_len, b_lo, b_hi):
    """Scratch words of the findHits query of a tail call whose `a` window is [0, a_len - 1] of its view and whose `b` window is
    [b_lo, b_hi]: words = 3 * cap + 2 + na + nf (cap: the power of two >= max(16, 2 * na)); 0 for a query with no work after
    the clamps of ablast.cc:47-53."""
    if a_len < WORD or b_hi + 1 < WORD + b_lo:
        return 0
    na, nf, cap = a_len - WORD + 1, a_len, 16
    while cap < 2 * na:
        cap *= 2
    return 3 * cap + 2 + na + nf


def golden_tail_words(answers):
    """query_words of every tail call in the stored full trails (a tail call forces its start or its end; its window on `a` ends
    where the query's does: PctgBuilder.cc:1544-1551, 1584-1591)"""
    out = []
    for a in answers:
        for t in (a or {}).get("trail", ()):
            if t[8] or t[9]:
                out.append(query_words(t[5] + 1, t[6], t[7]))
    return out


def seed_case():
    """A merge block whose left tail alignment depends on its seed: the slave lacks 400 bases of the master 100 bases in front of
    the block, so most of the tail lies on diagonal 0 -- findHits returns [0] -- while the seed used when there are no hits
    (sa - sb, PctgBuilder.cc:1554-1561) is 400, further from it than the band is wide.  The call seeded with 0 ends empty, the
    one seeded with 400 aligns the last 100 bases."""
    import random
    import _cases
    rng = random.Random(2026)
    g = _cases.rand_seq(rng, 6000, 0)
    slave = _cases.mutate(rng, g[:1000], 0.01, 0, 0) + _cases.mutate(rng, g[1400:], 0.01, 0, 0)
    return dict(kind="seed-matters", master=g, slave=slave, blocks=[(1500, 4000, 1100, 3600, "+", "+", 10)],
                tails=(True, True, True, True))


def run_seed_case(c, stats_of):
    """seed_case() through context c against the oracle's driver: run_groups' tuple"""
    sc = seed_case()
    want, _ = T.oracle_answer(sc)
    _, _, got = raw_call(c, [sc])
    g, keys, _ = got[0]
    d = T.differences(g, want, keys)
    return 1, (["seed-matters: %s" % d] if d else []), tail_calls(sc, keys), dict(stats_of()[0]), l1_cohorts(c)


def run_groups(c, groups, stats_of):
    """every stored merge block of the groups through context c: (checked, differing cases, tail calls counted from the audit
    trails, the hits statistics summed over the calls, most cohorts a call used).  Where an answer is stored with its whole trail,
    the seed of every tail call (the begin_a of the window the reference called find_alignment with: trail[i][4]) is compared as
    well as the call's result; total["seeds"] counts them."""
    total = dict(seeds=0, tail_queries=0, device_queries=0, trivial_queries=0, host_fallback=0, host_queries=0, hits_launches=0)
    n = n_tail = cohorts = 0
    diffs = []
    for group in groups:
        cases = T.GROUPS[group]()
        answers = T.stored(group, cases)
        keep = [k for k, a in enumerate(answers) if a is not None]
        _, _, got = raw_call(c, [cases[k] for k in keep])
        for st in stats_of():
            for k in st:
                if k in total and k != "seeds":
                    total[k] += st[k]
            total["mode"] = st["mode"]
        cohorts = max(cohorts, l1_cohorts(c))
        for k, (g, keys, seeds) in zip(keep, got):
            d = T.differences(g, answers[k], keys)
            if seeds is not None and "trail" in answers[k]:
                want_seeds = [(bool(t[8]), t[4]) for t in answers[k]["trail"] if t[8] or t[9]]   # left forces its end, right its start
                total["seeds"] += len(want_seeds)
                if seeds != want_seeds:
                    d.append("seeds: device %s, reference %s" % (seeds, want_seeds))
            if d:
                diffs.append("%s %s #%d: %s" % (group, cases[k]["kind"], k, d))
            n_tail += tail_calls(cases[k], keys)
            n += 1
    return n, diffs, n_tail, total, cohorts


def l1_cohorts(c):
    import gam_ngs_amd as gam
    from gam_ngs_amd import lib as L
    if isinstance(c, gam.MultiContext):
        return 0
    st = L.L1Stats()
    c.lib.gamdp_ctx_l1_stats(c.handle, C.byref(st))
    return st.cohorts


def main(groups, how):
    import gam_ngs_amd as gam
    from gam_ngs_amd import lib as L
    c = gam.Context(0)
    if how == "setter":
        c.set_l1_hits(L.L1_HITS_DEVICE)
    if groups == "seed-case":
        n, diffs, n_tail, stats, cohorts = run_seed_case(c, lambda: [c.l1_hits_stats()])
    else:
        n, diffs, n_tail, stats, cohorts = run_groups(c, groups.split(","), lambda: [c.l1_hits_stats()])
    print(json.dumps(dict(n=n, diffs=diffs[:5], n_diffs=len(diffs), tail_calls=n_tail, stats=stats, cohorts=cohorts,
                          diag=bool(c.lib.gamdp_build_info() & 1))))


if __name__ == "__main__":
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    main(sys.argv[1], sys.argv[2])
