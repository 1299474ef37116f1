"""gamdp_find_hits_batch on the GPU against the host findHits (gamdp_find_hits), the CPU oracle and, where it is built, the
reference's own ABlast::findHits (oracle/_ref/libgamref.so).  Each group below is ONE batched call."""
import ctypes as C
import random

import numpy as np
import pytest

import _cases
import _gage
import _golden as G
import _gpu
import _hitsq as H
import _oracle as O
import gam_ngs_amd as gam
from gam_ngs_amd import api, lib

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1


def _calls(sset, queries):
    return [(sset.contig(q[0], q[1], q[2]), q[3], q[4], sset.contig(q[5], q[6], q[7]), q[8], q[9]) for q in queries]


def run_group(seqs, queries, ascii=False):
    """one batched call with hit lists and one with summaries only (hits_buf == NULL) over the same queries"""
    ctx = _gpu.ctx()
    sset = gam.SequenceSet(ctx, seqs, ascii=ascii)
    calls, words = _calls(sset, queries), [q[10] for q in queries]
    ab = gam.ABlast()
    hits = ab.find_hits_many(ctx, calls, words=words)
    sums = ab.find_hits_many(ctx, calls, want_hits=False, words=words)
    sset.close()
    return hits, sums


def host_hits(codes, q):
    a, b = H.view(codes[q[0]], q[1], q[2]), H.view(codes[q[5]], q[6], q[7])
    return a, b, gam.ABlast(q[10]).findHits(a, q[3], q[4], b, q[8], q[9])


def check_group(codes, queries, hits, sums, oracle=True, votes_for=0):
    """hits / summaries of the device call against the host; the oracle and the reference where asked for; the vote
    count against the Python statement for the first votes_for queries"""
    use_ref = oracle and O.ref() is not None
    for k, (q, h, s) in enumerate(zip(queries, hits, sums)):
        a, b, want = host_hits(codes, q)
        assert h == want, (k, q)
        assert s[:3] == (len(want), want[0] if want else 0, want[-1] if want else 0), (k, q)
        assert (s[3] > 0) == bool(want), (k, q)
        if oracle:
            assert O.oracle_find_hits(a, q[3] & M64, q[4] & M64, b, q[8] & M64, q[9] & M64, q[10]) == want, (k, q)
        if use_ref:
            assert O.ref_find_hits(api.decode(a).encode(), q[3] & M64, q[4] & M64, api.decode(b).encode(), q[8] & M64,
                                   q[9] & M64, q[10]) == want, (k, q)
        if k < votes_for:
            assert H.py_find_hits(a, q[3], q[4], b, q[8], q[9], q[10]) == (want, s[3]), (k, q)


def test_golden_cases():
    gold = G.load("findhits.json")
    seqs, queries = [], []
    for i, d in enumerate(gold):
        seqs += [api.encode(d["a"]), api.encode(d["b"])]
        queries.append((2 * i, False, 0, d["a_s"], d["a_e"], 2 * i + 1, False, 0, d["b_s"], d["b_e"], d["word"]))
    hits, sums = run_group(seqs, queries)
    for d, h in zip(gold, hits):
        assert h == d["hits"], d["name"]
    check_group(seqs, queries, hits, sums, votes_for=len(queries))


def _random_queries(seed, n):
    rng = random.Random(seed)
    seqs, queries = [], []
    for i in range(n):
        word = rng.choice((1, 2, 19, 20, 21, 31, 32, 33))
        la = rng.choice((0, 1, word - 1, word, rng.randint(0, 60), rng.randint(0, 400), rng.randint(0, 400)))
        la = max(0, la)
        a = _cases.rand_seq(rng, la, 0.05 if rng.random() < 0.3 else 0)
        off = rng.randint(0, max(0, la // 2))
        if rng.random() < 0.7 and la > off:
            b = _cases.mutate(rng, a[off:], 0.02, 0.005, 0.005)
        else:
            b = _cases.rand_seq(rng, rng.randint(0, 300), 0.05 if rng.random() < 0.2 else 0)
        seqs += [api.encode(a), api.encode(b)]

        def end(n_):
            u = rng.random()
            return rng.randint(0, n_ + 5) if u < 0.8 else (M64 if u < 0.9 else rng.randint(n_, n_ + 10 ** 6))

        queries.append((2 * i, False, 0, rng.randint(0, 20) if rng.random() < 0.8 else rng.randint(0, la + 30), end(la),
                        2 * i + 1, False, 0, rng.randint(0, 20) if rng.random() < 0.8 else rng.randint(0, len(b) + 30),
                        end(len(b)), word))
    return seqs, queries


def test_random_cases():
    seqs, queries = _random_queries(20261016, 3000)
    hits, sums = run_group(seqs, queries)
    check_group(seqs, queries, hits, sums, votes_for=300)
    assert sum(1 for h in hits if h) > 200


def test_n_windows_and_code_collision():
    rng = random.Random(5)
    seqs, queries = [], []

    def add(a, b, word, a_s=0, a_e=M64, b_s=0, b_e=M64):
        i = len(seqs) // 2
        seqs.extend([api.encode(a), api.encode(b)])
        queries.append((2 * i, False, 0, a_s, a_e, 2 * i + 1, False, 0, b_s, b_e, word))

    x = _cases.rand_seq(rng, 19, 0)
    # an N at the last place equals a digit one higher at the place before it and an A at the last: X+"AN" and X+"TA" have
    # equal codes (4*0 + 4 == 4*1 + 0), so the two different 21-mers vote
    add(_cases.rand_seq(rng, 7, 0) + x + "AN" + _cases.rand_seq(rng, 30, 0), x + "TA", 21)
    add("GGAN", "GTA", 2)
    add("CCCCAN", "TA", 2)
    for _ in range(40):
        a = _cases.rand_seq(rng, rng.randint(50, 500), 0.3)
        b = _cases.mutate(rng, a[rng.randint(0, 40):], 0.01, 0.0, 0.0)
        add(a, b, rng.choice((2, 5, 20, 32)))
    # poly-G 32-mers and longer: the code wraps to 2^64 - 1 (all ones)
    add(_cases.rand_seq(rng, 40, 0) + "G" * 90 + _cases.rand_seq(rng, 40, 0), "G" * 70, 32)
    add("G" * 120, "C" * 10 + "G" * 60, 33)
    add("NNNN" * 40, "NNNN" * 30, 20)
    hits, sums = run_group(seqs, queries)
    check_group(seqs, queries, hits, sums, votes_for=len(queries))
    assert hits[0] == [7] and sums[0][3] == 1           # the collision voted (diagonal 7 - 0)
    assert hits[1] and hits[2]
    assert hits[-3] and sums[-3][3] > 1 and hits[-2]


def test_reverse_complement_and_suffix_views():
    rng = random.Random(77)
    seqs = []
    for _ in range(60):
        a = _cases.rand_seq(rng, rng.randint(30, 3000), 0.01 if rng.random() < 0.3 else 0)
        seqs += [api.encode(a), api.encode(_cases.mutate(rng, a[rng.randint(0, 20):], 0.02, 0.005, 0.005))]
    queries = []
    for i in range(600):
        k = rng.randrange(30)
        a_id, b_id = (2 * k, 2 * k + 1) if rng.random() < 0.5 else (2 * k + 1, 2 * k)
        a_rc, b_rc = rng.random() < 0.5, rng.random() < 0.5
        la, lb = len(seqs[a_id]), len(seqs[b_id])
        a_off, b_off = rng.randint(0, la // 3), rng.randint(0, lb // 3)
        if rng.random() < 0.03:
            a_off = la   # an empty view
        queries.append((a_id, a_rc, a_off, rng.randint(0, 50), rng.choice((M64, rng.randint(0, la))), b_id, b_rc, b_off,
                        rng.randint(0, 50), rng.choice((M64, rng.randint(0, lb))), rng.choice((12, 20, 25))))
    hits, sums = run_group(seqs, queries)
    check_group(seqs, queries, hits, sums, votes_for=40)
    assert sum(1 for h in hits if h) > 100


def test_gage_tail_windows():
    pb = _gage.problem(3)
    seqs, queries = H.tail_queries(pb)
    assert len(queries) > 50
    hits, sums = run_group(seqs, queries)
    n_seeded = 0
    for q, h, s in zip(queries, hits, sums):
        a, b, want = host_hits(seqs, q)
        assert h == want, q
        # what the driver consumes: hitsList.back() for a left tail, .front() for a right one (PctgBuilder.cc:1544, 1584)
        assert (s[1], s[2]) == ((want[0], want[-1]) if want else (0, 0)), q
        n_seeded += bool(want)
    assert n_seeded > len(queries) // 4


def test_repeats():
    rng = random.Random(9)
    unit = "ACGTTGCAGT"
    seqs, queries = [], []

    def add(a, b, word=20):
        i = len(seqs) // 2
        seqs.extend([api.encode(a), api.encode(b)])
        queries.append((2 * i, False, 0, 0, M64, 2 * i + 1, False, 0, 0, M64, word))

    add("A" * 3000, "A" * 2000)
    add(unit * 400, unit * 250)
    add(_cases.rand_seq(rng, 500, 0) + "AC" * 1500 + _cases.rand_seq(rng, 500, 0), "CA" * 1200)
    add("ACGTA" * 700, _cases.rand_seq(rng, 100, 0) + "ACGTA" * 300, 7)
    hits, sums = run_group(seqs, queries)
    check_group(seqs, queries, hits, sums)
    assert len(hits[0]) > 500 and len(hits[1]) > 50   # many tied diagonals


def test_packed_only_synthetic_set():
    ctx = _gpu.ctx()
    n_pairs, length = 6, 20000
    syn = gam.SequenceSet.synthetic(ctx, 40, n_pairs, length)
    codes = []
    for k in range(n_pairs):
        m, s = api.synth_pair(40 + k, length)
        codes += [m, s]
    assert [len(c) for c in codes] == syn.lengths
    rng = random.Random(3)
    queries = []
    for k in range(n_pairs):
        for _ in range(8):
            # the master's window starts in front of the slave's (only idx_a >= idx_b votes)
            a_off = rng.choice((0, rng.randint(0, 5000)))
            a_s = rng.randint(0, 2000)
            b_s = a_off + a_s + rng.randint(0, 1000)
            queries.append((2 * k, False, a_off, a_s, a_s + rng.randint(300, 6000), 2 * k + 1, False, 0, b_s,
                            rng.choice((M64, b_s + rng.randint(300, 9000))), 20))
    ab = gam.ABlast()
    hits = ab.find_hits_many(ctx, _calls(syn, queries))
    check_group(codes, queries, hits, ab.find_hits_many(ctx, _calls(syn, queries), want_hits=False), oracle=False)
    assert sum(1 for h in hits if h) > len(queries) // 2
    # a reverse complement needs the host codes a packed-only set does not keep
    with pytest.raises(gam.GamdpError):
        ab.find_hits_many(ctx, [(syn.contig(0, True), 0, 100, syn.contig(1), 0, 100)])
    syn.close()


def _raw(ctx, sset, queries, caps=None):
    n = len(queries)
    tasks = (lib.HitsTask * n)()
    for t, q in zip(tasks, queries):
        t.a_id, t.a_rc, t.a_off, t.a_start, t.a_end = q[0], int(q[1]), q[2], q[3] & M64, q[4] & M64
        t.b_id, t.b_rc, t.b_off, t.b_start, t.b_end, t.word = q[5], int(q[6]), q[7], q[8] & M64, q[9] & M64, q[10]
    out = (lib.HitsResult * n)()
    if caps is None:
        return ctx.lib.gamdp_find_hits_batch(ctx.handle, sset.handle, sset.handle, tasks, n, out, None, None, None), out, None
    offs = np.cumsum([0] + list(caps))
    buf = (C.c_uint32 * max(1, int(offs[-1])))()
    rc = ctx.lib.gamdp_find_hits_batch(ctx.handle, sset.handle, sset.handle, tasks, n, out, buf,
                                       (C.c_uint64 * n)(*[int(x) for x in offs[:-1]]), (C.c_uint64 * n)(*caps))
    return rc, out, [list(buf[int(offs[i]):int(offs[i]) + min(out[i].n_hits, caps[i])]) for i in range(n)]


def test_cap_truncates_summary_stays_whole():
    ctx = _gpu.ctx()
    seqs = [api.encode("A" * 600), api.encode("A" * 400), api.encode("ACGT" * 100)]
    sset = gam.SequenceSet(ctx, seqs, ascii=False)
    queries = [(0, False, 0, 0, M64, 1, False, 0, 0, M64, 20), (2, False, 0, 0, M64, 2, False, 0, 0, M64, 20),
               (0, False, 0, 0, M64, 2, False, 0, 0, M64, 20), (0, False, 700, 0, M64, 1, False, 0, 0, M64, 20)]
    full = [host_hits(seqs, q)[2] for q in queries]
    caps = [3, 0, 5, 2]
    rc, out, got = _raw(ctx, sset, queries, caps)
    assert rc == 0
    rc0, out0, _ = _raw(ctx, sset, queries)
    assert rc0 == 0
    for i, want in enumerate(full):
        assert got[i] == want[:caps[i]]
        assert (out[i].n_hits, out[i].first, out[i].last) == (len(want), want[0] if want else 0, want[-1] if want else 0)
        assert (out[i].n_hits, out[i].votes, out[i].first, out[i].last) == (out0[i].n_hits, out0[i].votes, out0[i].first, out0[i].last)
    assert len(full[0]) > 3 and out[0].votes > 1
    assert [o.status for o in out] == [lib.ST_OK] * 3 + [lib.ST_INVALID]   # a view offset beyond the sequence
    sset.close()


def test_small_arena_splits_and_refuses_a_query_too_big():
    ctx = _gpu.ctx()
    rng = random.Random(21)
    seqs = []
    for _ in range(12):
        a = _cases.rand_seq(rng, 5000, 0)
        seqs += [api.encode(a), api.encode(_cases.mutate(rng, a[300:], 0.02, 0.005, 0.005))]
    seqs.append(api.encode(_cases.rand_seq(rng, 100000, 0)))
    sset = gam.SequenceSet(ctx, seqs, ascii=False)
    queries = [(2 * k, False, 0, 0, M64, 2 * k + 1, False, 0, 0, M64, 20) for k in range(12)]
    want = [host_hits(seqs, q)[2] for q in queries]
    assert all(want)
    caps = [5000] * len(queries)
    try:
        ctx.set_arena_bytes(1 << 20)   # one of these queries needs about 250 KB: the batch goes in several pieces
        rc, out, got = _raw(ctx, sset, queries, caps)
        assert rc == 0 and got == want
        big = queries[:3] + [(24, False, 0, 0, M64, 0, False, 0, 0, M64, 20)]   # 100 kb of a k-mers: about 4 MB
        rc, _, _ = _raw(ctx, sset, big, [100001] * 4)
        assert rc == lib.ENOMEM
        assert "query 3" in ctx.last_error()
    finally:
        ctx.set_arena_bytes(0)
    rc, out, got = _raw(ctx, sset, queries + [(24, False, 0, 0, M64, 0, False, 0, 0, M64, 20)], caps + [100001])
    assert rc == 0 and got[:-1] == want and got[-1] == host_hits(seqs, (24, False, 0, 0, M64, 0, False, 0, 0, M64, 20))[2]
    sset.close()


def test_launch_info_and_kernel_time():
    ctx = _gpu.ctx()
    rng = random.Random(4)
    a = _cases.rand_seq(rng, 3000, 0)
    b = _cases.mutate(rng, a[200:], 0.02, 0.005, 0.005)
    sset = gam.SequenceSet(ctx, [a.encode(), b.encode()])
    gam.BandedSmithWaterman(ctx).find_alignments([(sset.contig(0), 200, 2999, sset.contig(1), 0, len(b) - 1)] * 4)
    info = ctx.launch_info()
    assert info
    _, n0 = ctx.kernel_time()
    hits = gam.ABlast().find_hits_many(ctx, [(sset.contig(0), 0, 10 ** 9, sset.contig(1), 0, 10 ** 9)] * 3)
    assert hits[0] == gam.ABlast().findHits(api.encode(a), 0, 10 ** 9, api.encode(b), 0, 10 ** 9) and hits[0]
    assert ctx.launch_info() == info          # still the align call's record
    _, n1 = ctx.kernel_time()
    assert n1 > n0                            # the find_hits launches are counted
    sset.close()


def test_id_out_of_range_is_einval():
    ctx = _gpu.ctx()
    sset = gam.SequenceSet(ctx, [b"ACGTACGTACGTACGTACGTACGT", b"ACGTACGTACGTACGTACGTA"])
    q = (0, False, 0, 0, M64, 1, False, 0, 0, M64, 20)
    assert _raw(ctx, sset, [q, q[:5] + (2,) + q[6:]])[0] == lib.EINVAL
    assert _raw(ctx, sset, [(5,) + q[1:]])[0] == lib.EINVAL
    assert _raw(ctx, sset, [q])[0] == 0
    sset.close()
