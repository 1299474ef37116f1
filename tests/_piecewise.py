"""Pairs whose divergence changes along the pair: b is a copy of a mutated piece by piece, each piece at its own substitution /
insertion / deletion rates.  Seeded, in numpy, whole batches at a time.  The synthetic form of a contig pair with a repeat or a
misassembly in it: the workload on which a walk that has stopped testing can lose.

    batch(rng, n_pairs, length)  -> base codes (A 0, T 1, C 2, G 3), what tools/walk_skip*_ab.py --piecewise upload
    pair(seed, length)           -> one pair as ASCII strings, what the tests use"""
import numpy as np

# thirds: a divergent one, an identical one, a lightly divergent one (substitutions, insertions, deletions per base)
THIRDS = ((0.03, 0.01, 0.01), (0.0, 0.0, 0.0), (0.003, 0.001, 0.001))
LETTERS = np.frombuffer(b"ATCG", dtype=np.uint8)


def mutate_block(rng, A, sub, ins, dele):
    """A: (n_pairs, w) base codes -> (the mutated copies as one array, their lengths): events drawn sparsely, applied in one pass"""
    n_pairs, w = A.shape
    flat = np.ascontiguousarray(A).reshape(-1)
    N = flat.size
    B = flat.copy()
    k = rng.binomial(N, sub)
    if k:
        p = rng.integers(0, N, k)
        B[p] = (flat[p] + rng.integers(1, 4, k).astype(np.uint8)) & 3     # another base, never the same
    cnt = np.ones(N, np.uint8)
    k = rng.binomial(N, dele)
    if k:
        cnt[rng.integers(0, N, k)] = 0                                     # bases only a has
    k = rng.binomial(N, ins)
    ins_at = np.unique(rng.integers(0, N, k)) if k else np.zeros(0, np.int64)
    cnt[ins_at] += 1                                                       # bases only b has: behind their source base
    lens = cnt.reshape(n_pairs, w).sum(axis=1, dtype=np.int64)
    out = np.repeat(B, cnt)
    if ins_at.size:
        ends = np.cumsum(cnt, dtype=np.int64)
        out[ends[ins_at] - 1] = rng.integers(0, 4, ins_at.size).astype(np.uint8)
    return out, lens


def batch(rng, n_pairs, length, rates=THIRDS, reverse=False):
    """-> (A: (n_pairs, length) base codes, [b of pair 0, b of pair 1, ...]): b in len(rates) equal pieces; reverse: the pieces in the
    other order"""
    A = rng.integers(0, 4, (n_pairs, length), dtype=np.uint8)
    rates = tuple(reversed(rates)) if reverse else tuple(rates)
    cuts = [length * k // len(rates) for k in range(len(rates) + 1)]
    pieces = []
    for k, r in enumerate(rates):
        out, lens = mutate_block(rng, A[:, cuts[k]:cuts[k + 1]], *r)
        pieces.append((out, np.concatenate(([0], np.cumsum(lens)))))
    return A, [np.concatenate([out[at[i]:at[i + 1]] for out, at in pieces]) for i in range(n_pairs)]


def pair(seed, length, rates=THIRDS, reverse=False):
    """(a, b) as str"""
    A, B = batch(np.random.default_rng(seed), 1, length, rates, reverse)
    return LETTERS[A[0]].tobytes().decode(), LETTERS[B[0]].tobytes().decode()
