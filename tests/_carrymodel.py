"""A plain-Python model of find_alignment as a fill only: every cell carries the summary of the traceback that would start in it.

Written from BandedSmithWaterman::find_alignment, lib/src/alignment/banded_smith_waterman.cc (line numbers below are its), and from
first_match_pos / last_match_pos, lib/src/alignment/my_alignment.cc:167-193 / :228-262.  It shares nothing with the library or with
oracle/gamdp_oracle.c; tests/test_carry_model_cpu.py pins it to the reference's recorded output (tests/golden).

The traceback (:227-311) is a pointer chase: the step it takes from a cell (x, y), pos = begin_a + x + y - band, depends on that cell's
value and its three neighbours' values only, which the fill has in hand when it computes the cell.  So the summary T(x, y) of the
loop entered at (x, y) -- where it ends, how many ops, how many MATCH ops, the first and the last MATCH -- follows from the summary of
the cell the step leads to, and the end cell's summary is the whole result: no directions, no stored matrix, no walk.  (The model keeps
the two rows the recurrence reads, not the matrix.)
"""
OK, EMPTY, OUT_OF_RANGE, INVALID = 0, 1, 2, 3
GAP = -8             # GAP_SCORE, my_alignment.hpp:46
MAXGAP = 10          # FORCE_MAXGAP_LEN, banded_smith_waterman.hpp:37
MAX_ROWS = 500000    # BSW_MAX_ALIGNMENT
DIAG, UP, LEFT = 0, 1, 2   # MATCH or MISMATCH (x--), GAP_A (x--, y++), GAP_B (y--)
M64 = (1 << 64) - 1
NEG = -(1 << 62)     # std::numeric_limits<int64_t>::min() of :235 / :270: below every value

_CODE = {65: 0, 84: 1, 67: 2, 71: 3, 97: 0, 116: 1, 99: 2, 103: 3}   # A T C G -> 0 1 2 3, anything else is N (4)


def codes(s):
    """ASCII bases -> codes A0 T1 C2 G3 N4 (bytes of codes pass through)"""
    if isinstance(s, str):
        s = s.encode()
    if all(c <= 4 for c in s):
        return bytes(s)
    return bytes(_CODE.get(c, 4) for c in s)


def score(ca, cb):
    """SCORING_MATRIX (:80-88)"""
    if ca == 4 or cb == 4:
        return 5 if ca == cb else 0
    return 5 if ca == cb else -4


class Throws(Exception):
    """a.at(pos) / b.at(pos) beyond the sequence"""


def _at(s, i):
    if i < 0 or i >= len(s):
        raise Throws()
    return s[i]


def _signed(v):
    v &= M64
    return v - (1 << 64) if v >> 63 else v


def step(fs, Y, x, y, pos, v, d, u, l, ca, cb):
    """The op the traceback takes from (x, y) (:229-308).  v = sw[x][y]; d, u, l = sw[x-1][y], sw[x-1][y+1], sw[x][y-1] where they
    exist (None otherwise); ca, cb = the two bases.  Returns (op, is_match)."""
    s = score(ca, cb)
    is_match = ca == cb or ca == 4 or cb == 4                       # :239, :274
    if pos == 0:                                                    # :229-262
        left = NEG if (fs and x > MAXGAP) else GAP                  # :233-235
        if v == s:                                                  # :237
            return DIAG, is_match
        if y == Y - 1 or v == left:                                 # :251
            return LEFT, False
        return UP, False
    diag = (d if x > 0 else 0) + s                                  # :265
    up = u + GAP if (x > 0 and y < Y - 1) else GAP                  # :266
    if fs and x == 0:                                               # :269-270
        up = GAP if pos <= MAXGAP else NEG
    if v == diag:                                                   # :272
        return DIAG, is_match
    if 0 < y < Y - 1:                                               # :286-296
        return (UP, False) if v == up else (LEFT, False)
    if y < Y - 1:                                                   # :297, y == 0
        return UP, False
    return LEFT, False                                              # :303, y == y_size-1


def find_result(a, b, band, begin_a, end_a, begin_b, end_b, fs=False, fe=False):
    """-> (status, begin_a, begin_b, score, n_match, length, first_a, first_b, first_found, last_a, last_b, last_found, homology),
    the layout of tests/_golden.KEYS"""
    a, b = codes(a), codes(b)
    try:
        return _find(a, b, band, begin_a, end_a, begin_b, end_b, bool(fs), bool(fe))
    except Throws:
        return (OUT_OF_RANGE,) + (0,) * 11 + (0.0,)


def _empty():
    return (EMPTY,) + (0,) * 11 + (0.0,)


def _find(a, b, band, begin_a, end_a, begin_b, end_b, fs, fe):
    alen, blen = len(a), len(b)
    if end_b < begin_b:                                             # :90
        return _empty()
    if begin_b >= blen:
        # :91 sets end_b below begin_b and x_size wraps: the row-0 loop throws from b.at(begin_b) at the first column that qualifies
        # (:116, :125); with none the reference indexes a matrix it could not allocate
        lo, hi = max(begin_a - band, 0), begin_a + band
        any_col = lo < alen or (fs and lo <= min(hi, MAXGAP))
        return ((OUT_OF_RANGE if any_col else INVALID),) + (0,) * 11 + (0.0,)
    if end_b >= blen:                                               # :91
        end_b = blen - 1
    X = end_b - begin_b + 1                                         # :93-95, in unsigned arithmetic
    X = min(X, (alen + band - begin_a) & M64, MAX_ROWS)
    if X == 0:
        return (INVALID,) + (0,) * 11 + (0.0,)
    Y = 2 * band + 1                                                # :97
    A0 = begin_a - band

    # the end-cell search (:173-215) as a rank per candidate cell: last row by columns (:179-192), then the anti-diagonal
    # pos == end_a by rows (:197-212); `!found || value > max` keeps the first of equal values
    ge = end_a >= begin_a + band                                    # :197 (both sides unsigned)
    i0 = end_a - (begin_a + band) if ge else 0
    j0 = 2 * band if ge else _signed(2 * band - (begin_a + band - end_a))   # :198

    def candidate_rank(i, j, pos):
        ranks = []
        if not fe and i == X - 1 and 0 <= pos <= end_a:             # :183
            ranks.append(j)
        if i >= i0 and j >= 0 and i - i0 == j0 - j:                 # the cell the loop :199 visits in row i
            if not fe or (X - 1 - MAXGAP >= 0 and i >= X - 1 - MAXGAP):   # :201 (unsigned: x_size < 11 wraps, nothing passes)
                ranks.append(Y + (i - i0))
        return min(ranks) if ranks else None

    best = None   # (value, rank, summary or None, pos)
    prev_v, prev_t = [0] * Y, [None] * Y
    for i in range(X):
        cur_v, cur_t = [0] * Y, [None] * Y
        for j in range(Y):
            pos = A0 + i + j
            in_a = 0 <= pos < alen
            if i == 0:                                              # :112-132
                if (not fs and in_a) or (fs and 0 <= pos <= MAXGAP):
                    diag = score(_at(a, pos), _at(b, begin_b))
                    has_left = pos > 0 and j > 0
                    cur_v[j] = max(diag, GAP, cur_v[j - 1]) if has_left else max(GAP, diag)
                if fs and pos > MAXGAP and pos < alen:
                    diag = score(_at(a, pos), _at(b, begin_b))
                    has_left = pos > 0 and j > 0
                    cur_v[j] = max(diag, cur_v[j - 1]) if has_left else diag
            elif in_a:                                              # :141-168
                s = score(_at(a, pos), _at(b, begin_b + i))
                up = prev_v[j + 1] + GAP if j < Y - 1 else None
                if pos == 0 and (not fs or i <= MAXGAP):            # :143-150
                    cur_v[j] = max(s, up, GAP) if up is not None else max(s, GAP)
                elif pos == 0:                                      # :151-157
                    cur_v[j] = max(s, up) if up is not None else s
                else:                                               # :158-168
                    cands = [prev_v[j] + s]
                    if up is not None:
                        cands.append(up)
                    if j > 0:
                        cands.append(cur_v[j - 1] + GAP)
                    cur_v[j] = max(cands)
            if in_a:
                # the summary of the traceback entered here, from its predecessor's
                op, is_match = step(fs, Y, i, j, pos, cur_v[j], prev_v[j] if i > 0 else None, prev_v[j + 1] if (i > 0 and j < Y - 1) else None,
                                    cur_v[j - 1] if j > 0 else None, a[pos], b[begin_b + i])
                px, py = (i - 1, j) if op == DIAG else (i - 1, j + 1) if op == UP else (i, j - 1)
                ppos = A0 + px + py
                if px < 0 or py < 0 or ppos < 0:                    # the loop ends (:227); begin from :321
                    t = (ppos + 1, begin_b + px + 1, 0, 0, None, None)
                else:
                    t = prev_t[py] if px == i - 1 else cur_t[py]
                    assert t is not None and ppos < alen, "a predecessor inside the matrix lies inside a"
                ba, bb, length, n_match, first, last = t
                if is_match:
                    here = (pos, begin_b + i)
                    n_match, last, first = n_match + 1, here, (first if first is not None else here)
                cur_t[j] = (ba, bb, length + 1, n_match, first, last)
            rank = candidate_rank(i, j, pos)
            if rank is not None and (best is None or cur_v[j] > best[0] or (cur_v[j] == best[0] and rank < best[1])):
                best = (cur_v[j], rank, cur_t[j], pos)
        prev_v, prev_t = cur_v, cur_t

    if best is None:                                                # :215
        return _empty()
    value, _, t, pos = best
    if pos >= alen:                                                 # a.at(pos) of :231 / :265 (pos >= 0: every candidate has it)
        raise Throws()
    assert pos >= 0 and t is not None
    ba, bb, length, n_match, first, last = t
    # without a MATCH: first_match_pos ends behind the last op (my_alignment.cc:167-193), last_match_pos keeps the begin (:228-262)
    x_end = None
    if first is None:
        # the end cell is (x, y) with pos: its row is where the ops end
        x_end = _end_row(best, X, Y, i0)
        first_a, first_b, first_found = pos + 1, begin_b + x_end + 1, 0
        last_a, last_b, last_found = ba, bb, 0
    else:
        first_a, first_b, first_found = first[0], first[1], 1
        last_a, last_b, last_found = last[0], last[1], 1
    homology = float(n_match * 100) / float(length) if length else 0.0      # :319
    return (OK, ba, bb, value, n_match, length, first_a, first_b, first_found, last_a, last_b, last_found, homology)


def _end_row(best, X, Y, i0):
    rank = best[1]
    return X - 1 if rank < Y else i0 + (rank - Y)
