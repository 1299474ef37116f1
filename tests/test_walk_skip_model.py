"""The lemma behind GAMDP_WALK_SKIP_DIAG (gam_ngs_amd/csrc/kernel_walk.inc), on the CPU, against the oracle's edit strings.

find_alignment's traceback (lib/src/alignment/banded_smith_waterman.cc:265-285) tests diag first: in the interior (pos >= 1, x >= 1) it
steps diagonally iff sw[x][y] == sw[x-1][y] + S(a[pos], b[begin_b + x]), and its fill (:158-168) makes sw[x][y] >= sw[x-1][y] + S in
every such cell.  So for a walk standing on (x, y):

    sw[x][y] - sw[x-s][y] == sum of S over the s base pairs below      <=>      the next s ops of the traceback are all M / X

(=>: the difference telescopes into s terms sw[x-k][y] - sw[x-k-1][y] - S >= 0 that add to zero; <=: a diagonal step is taken on
equality).  The kernel tests the left side on values the fill stored, 64 rows apart, and jumps.

The fill here is a plain-Python copy of :97-171 (no force flags) that keeps the whole matrix; the path is the oracle's edit string
(tests/test_oracle_vs_ref.py pins the oracle to the reference).  Spans of 16 and 64, bands 20 - 150, on random, tie-rich and
single-indel pairs; every case set must hold spans where the equality holds and spans where it fails."""
import random

import _cases
import _oracle as O

GAP = -8
SPANS = (16, 64)


def score(ca, cb):
    return 5 if ca == cb else -4      # N-free pairs only


def fill(a, b, band, begin_a, begin_b, end_b):
    """sw of banded_smith_waterman.cc:97-171 without force flags; a, b: strings over ACGT"""
    end_b = min(end_b, len(b) - 1)
    X = min(end_b - begin_b + 1, len(a) + band - begin_a)
    Y = 2 * band + 1
    sw = [[0] * Y for _ in range(X)]
    for j in range(Y):                                               # :112-132
        pos = begin_a - band + j
        if 0 <= pos < len(a):
            diag = score(a[pos], b[begin_b])
            if pos > 0 and j > 0:
                sw[0][j] = max(diag, GAP, sw[0][j - 1])
            else:
                sw[0][j] = max(GAP, diag)
    for i in range(1, X):                                            # :135-171
        row, prev = sw[i], sw[i - 1]
        cb = b[begin_b + i]
        for j in range(Y):
            pos = begin_a + i + j - band
            if pos < 0 or pos >= len(a):
                continue
            s = score(a[pos], cb)
            up = prev[j + 1] + GAP if j < Y - 1 else GAP
            if pos == 0:                                             # :143-150
                row[j] = max(s, up, GAP) if j < Y - 1 else max(s, GAP)
                continue
            diag = prev[j] + s                                       # :158-168
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


def path_cells(o, ops, begin_b):
    """(x, pos) of the cell every op of the edit string was taken from, in the edit string's order.  The traceback takes ops[k] in
    cell k and moves on to cell k - 1 (GAP_A: x--, GAP_B: pos--, else both), and ends one step beyond (begin_b - 1, begin_a - 1)."""
    x, pos = o.begin_b - begin_b - 1, o.begin_a - 1
    out = []
    for op in ops:
        if op == "A":
            x += 1
        elif op == "B":
            pos += 1
        else:
            x += 1
            pos += 1
        out.append((x, pos))
    return out


def check_case(a, b, band, begin_a=0, begin_b=0):
    """-> (spans where the equality holds, spans where it fails, the cells of the path with their ops) over the oracle's path"""
    end_a, end_b = len(a) - 1, len(b) - 1
    o, ops = O.oracle_align(O.encode(a.encode()), O.encode(b.encode()), band, begin_a, end_a, begin_b, end_b, False, False, want_ops=True)
    assert o.status == O.OK and o.length == len(ops)
    sw = fill(a, b, band, begin_a, begin_b, end_b)
    cells = path_cells(o, ops, begin_b)
    x_end, pos_end = cells[-1]
    assert sw[x_end][pos_end - begin_a - x_end + band] == o.score          # the model's matrix is the oracle's
    holds = fails = 0
    for k, (x, pos) in enumerate(cells):
        if x < 65 or pos < 65:
            continue
        y = pos - begin_a - x + band
        for s in SPANS:
            total = sum(score(a[pos - t], b[begin_b + x - t]) for t in range(s))
            equal = sw[x][y] - sw[x - s][y] == total
            diagonal = all(op in "MX" for op in ops[k - s + 1:k + 1])      # the next s ops of the traceback: ops[k], ops[k-1], ...
            assert k - s + 1 >= 0
            assert equal == diagonal, (band, len(a), len(b), k, x, pos, s, ops[k - s + 1:k + 1])
            holds += equal
            fails += not equal
    return holds, fails, cells, ops


def test_random_pairs():
    rng = random.Random(41)
    holds = fails = 0
    for band, n in ((20, 330), (64, 300), (150, 260), (150, 330)):
        for div in (0.0, 0.3, 1.0):
            a, b = _cases.related_pair(rng, n, div=div)
            h, f, _, _ = check_case(a, b, band)
            holds += h
            fails += f
        a = _cases.rand_seq(rng, n + 30)
        h, f, _, _ = check_case(a, _cases.mutate(rng, a[17:], 0.02, 0.004, 0.004), band, begin_a=9, begin_b=3)
        holds += h
        fails += f
    assert holds > 100 and fails > 100, (holds, fails)


def test_tie_rich_pairs():
    """homopolymers, dinucleotide and tandem repeats: `up` and `left` tie with `diag` all along the path, and diag wins"""
    holds = fails = 0
    for band in (20, 150):
        for kind in ("homopolymer", "ac_shift1", "tandem19", "tandem17"):
            a, b = _cases.adversarial_pair(kind, 300, band)
            h, f, _, _ = check_case(a, b, band)
            holds += h
            fails += f
    rng = random.Random(42)
    for band in (20, 100):
        a = "".join(rng.choice("AC") for _ in range(280))
        b = a[:130] + "A" + a[130:]
        h, f, _, _ = check_case(a, b, band)
        holds += h
        fails += f
    assert holds > 100 and fails > 0, (holds, fails)


def test_one_row_above_on_and_below_a_single_indel():
    rng = random.Random(43)
    seen = 0
    for band in (20, 150):
        for kind in ("ins", "del"):
            for row in (130, 191, 192, 193):
                a = _cases.rand_seq(rng, 300)
                b = a[:row] + {"A": "C", "C": "G", "G": "T", "T": "A"}[a[row]] + a[row:] if kind == "ins" else a[:row] + a[row + 1:]
                holds, fails, cells, ops = check_case(a, b, band)
                gaps = [k for k, op in enumerate(ops) if op in "AB"]
                assert len(gaps) == 1 and holds > 0 and fails > 0, (band, kind, row, gaps)
                kg = gaps[0]
                xg, pg = cells[kg]
                assert xg >= 65 and pg >= 65
                sw = fill(a, b, band, 0, 0, len(b) - 1)
                for s in SPANS:
                    for dk, want in ((-1, True), (0, False), (1, False), (s - 1, False), (s, True)):
                        # dk ops further along the path than the gap: the span of the cell BEFORE the gap (dk = -1) and of the cell s
                        # ops behind it do not reach it, the spans of the cells between do
                        x, pos = cells[kg + dk]
                        y = pos - x + band
                        total = sum(score(a[pos - t], b[x - t]) for t in range(s))
                        assert (sw[x][y] - sw[x - s][y] == total) == want, (band, kind, row, s, dk)
                        seen += 1
    assert seen == 2 * 2 * 4 * 2 * 5
