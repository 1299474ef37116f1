"""The lemma behind gamdp_ctx_set_walk_skip_i32 (gam_ngs_amd/csrc/kernel_finish.inc, finish_walk<..., SKIP> with int32 checkpoint
images), on the CPU, against the oracle's edit strings: tests/test_walk_skip_model.py's statement in the units the int32 kernels
store and with the reference's three-valued score.

The int32 fill keeps G4 = 4 (H + 16 x + 8 y) per cell.  A diagonal step (x + 1, same y) adds 4 (S + 16): 84 for equal codes (N
against N included), 64 when exactly one side is N, 48 for a mismatch (S = 5 / 0 / -4, oracle/gamdp_oracle.c:20-25).  So for a
walk on (x, y) and a span of s rows with e equal pairs and n1 pairs with exactly one N

    G4(x, y) - G4(x - s, y) = 4 (sw[x][y] - sw[x-s][y]) + 64 s == 48 s + 36 e + 16 n1   <=>   the next s ops are all M / X

and the span's MATCH ops (equal codes, or an N on either side: oracle/gamdp_oracle.c:228) number e + n1.

The fill is test_walk_skip_model.fill's with that score; the path is the oracle's edit string.  Spans of 16 and 64, bands 20 - 200,
N-free and N-holding pairs; every case set must hold spans where the equality holds and spans where it fails, spans with an N-N
pair and spans with exactly-one-N pairs -- counted here, on the CPU."""
import random

import _cases
import _oracle as O
import test_walk_skip_model as M

GAP = -8
SPANS = (16, 64)


def score(ca, cb):
    if ca == cb:
        return 5                      # N against N too
    return 0 if "N" in (ca, cb) else -4


def fill(a, b, band, begin_a, begin_b, end_b):
    """test_walk_skip_model.fill (banded_smith_waterman.cc:97-171, no force flags) with the three-valued score"""
    end_b = min(end_b, len(b) - 1)
    X = min(end_b - begin_b + 1, len(a) + band - begin_a)
    Y = 2 * band + 1
    sw = [[0] * Y for _ in range(X)]
    for j in range(Y):
        pos = begin_a - band + j
        if 0 <= pos < len(a):
            diag = score(a[pos], b[begin_b])
            sw[0][j] = max(diag, GAP, sw[0][j - 1]) if pos > 0 and j > 0 else max(GAP, diag)
    for i in range(1, X):
        row, prev = sw[i], sw[i - 1]
        cb = b[begin_b + i]
        for j in range(Y):
            pos = begin_a + i + j - band
            if pos < 0 or pos >= len(a):
                continue
            s = score(a[pos], cb)
            up = prev[j + 1] + GAP if j < Y - 1 else GAP
            if pos == 0:
                row[j] = max(s, up, GAP) if j < Y - 1 else max(s, GAP)
                continue
            diag = prev[j] + s
            left = row[j - 1] + GAP if j > 0 else GAP
            if 0 < j < Y - 1:
                row[j] = max(diag, up, left)
            elif j < Y - 1:
                row[j] = max(diag, up)
            elif j > 0:
                row[j] = max(diag, left)
            else:
                row[j] = diag
    return sw


def g4(sw, x, y):
    return 4 * (sw[x][y] + 16 * x + 8 * y)


class Seen:
    def __init__(self):
        self.holds = self.fails = self.with_nn = self.with_n1 = self.passing_with_n = 0

    def ok(self, n_holding):
        base = self.holds > 100 and self.fails > 0
        return base and (not n_holding or (self.with_nn > 0 and self.with_n1 > 0 and self.passing_with_n > 0))

    def __repr__(self):
        return repr(self.__dict__)


def check_case(seen, a, b, band, begin_a=0, begin_b=0):
    end_a, end_b = len(a) - 1, len(b) - 1
    o, ops = O.oracle_align(O.encode(a.encode()), O.encode(b.encode()), band, begin_a, end_a, begin_b, end_b, False, False, want_ops=True)
    assert o.status == O.OK and o.length == len(ops)
    sw = fill(a, b, band, begin_a, begin_b, end_b)
    cells = M.path_cells(o, ops, begin_b)
    x_end, pos_end = cells[-1]
    assert sw[x_end][pos_end - begin_a - x_end + band] == o.score          # the model's matrix is the oracle's
    assert sum(op == "M" for op in ops) == o.n_match
    for k, (x, pos) in enumerate(cells):
        if x < 65 or pos < 65:
            continue
        y = pos - begin_a - x + band
        for s in SPANS:
            pairs = [(a[pos - t], b[begin_b + x - t]) for t in range(s)]
            e = sum(ca == cb for ca, cb in pairs)
            nn = sum(ca == cb == "N" for ca, cb in pairs)
            n1 = sum((ca == "N") != (cb == "N") for ca, cb in pairs)
            assert 48 * s + 36 * e + 16 * n1 == sum(4 * (score(ca, cb) + 16) for ca, cb in pairs)
            equal = g4(sw, x, y) - g4(sw, x - s, y) == 48 * s + 36 * e + 16 * n1
            assert g4(sw, x, y) - g4(sw, x - s, y) == 4 * (sw[x][y] - sw[x - s][y]) + 64 * s
            assert k - s + 1 >= 0
            span_ops = ops[k - s + 1:k + 1]                                # the next s ops of the traceback: ops[k], ops[k-1], ...
            diagonal = all(op in "MX" for op in span_ops)
            assert equal == diagonal, (band, len(a), len(b), k, x, pos, s, span_ops)
            if equal:
                assert span_ops.count("M") == e + n1, (band, k, s, span_ops, e, n1)
            seen.holds += equal
            seen.fails += not equal
            seen.with_nn += nn > 0
            seen.with_n1 += n1 > 0
            seen.passing_with_n += equal and nn > 0 and n1 > 0
    return cells, ops


def sprinkle(rng, a, b, every=23):
    """N into both sequences of a pair whose bases line up at equal indices for the most part: N-N, N-base and base-N all occur"""
    a, b = list(a), list(b)
    for at in range(every, min(len(a), len(b)) - 1, every):
        kind = rng.randrange(3)
        if kind != 1:
            a[at] = "N"
        if kind != 0:
            b[at] = "N"
    return "".join(a), "".join(b)


def test_n_free_pairs():
    rng = random.Random(51)
    seen = Seen()
    for band, n in ((20, 330), (64, 300), (150, 260), (200, 300)):
        for div in (0.0, 0.3, 1.0):
            a, b = _cases.related_pair(rng, n, div=div)
            check_case(seen, a, b, band)
        a = _cases.rand_seq(rng, n + 30)
        check_case(seen, a, _cases.mutate(rng, a[17:], 0.02, 0.004, 0.004), band, begin_a=9, begin_b=3)
    assert seen.ok(False) and seen.fails > 100 and seen.with_nn == seen.with_n1 == 0, seen


def test_n_holding_pairs():
    rng = random.Random(52)
    seen = Seen()
    for band, n in ((20, 330), (64, 300), (150, 260), (200, 300)):
        a = _cases.rand_seq(rng, n)
        check_case(seen, *sprinkle(rng, a, a), band)                                       # gap-free: every span passes
        check_case(seen, *sprinkle(rng, a, _cases.mutate(rng, a, 0.03, 0.0, 0.0)), band)   # substitutions only
        row = n // 2 + 11
        check_case(seen, *sprinkle(rng, a, a[:row] + a[row + 1:]), band)                   # one deletion: the N pairs shift apart behind it
        b = _cases.mutate(rng, a, 0.02, 0.004, 0.004)
        check_case(seen, *sprinkle(rng, a, b, every=17), band)
        check_case(seen, *sprinkle(rng, a + "ACGT", b[9:], every=29), band, begin_a=5, begin_b=2)
    assert seen.ok(True) and seen.fails > 100, seen


def test_n_holding_tie_rich_pairs():
    """homopolymers and repeats with N in them: `up` and `left` tie with `diag` along the path, N-base pairs score 0 next to gaps"""
    rng = random.Random(53)
    seen = Seen()
    for band in (20, 150):
        for kind in ("homopolymer", "ac_shift1", "tandem19", "tandem17"):
            a, b = _cases.adversarial_pair(kind, 300, band)
            check_case(seen, *sprinkle(rng, a, b, every=19), band)
    for band in (20, 100):
        a = "".join(rng.choice("AC") for _ in range(280))
        check_case(seen, *sprinkle(rng, a, a[:130] + "A" + a[130:], every=13), band)
    assert seen.ok(True), seen
