"""The walk of finish_walk<..., OPSRUN> (gam_ngs_amd/csrc/kernel_finish.inc; gamdp_ctx_set_ops_walk, GAMDP_OPS_WALK_RUNS) in plain
Python: from a forward edit string, its begin cell and the two coded sequences, the walk is replayed from the end cell, cut into single
steps and runs by the device's rule, and each run's bytes are produced as the 64 lanes produce them.  CPU only.

The rule.  The walk stands on cell (x, pos): x = row of the DP (b index - task begin_b), pos = a index.  Where x == 0 or pos == 0 it
takes one step of the edit string.  Everywhere else it takes a run: the n diagonal steps ahead of it, at most what the direction-word
cache holds (the block the walk stands in from its row r = (x + l) & 15 down, and the TB_DEPTH - 1 - k blocks below it, k = how deep in
the cache the walk already is) and at most min(x, pos); n == 0 is a gap step.  A run that ended at a gap whose cell still has x >= 1 and
pos >= 1 takes that gap step in the same iteration.  l = y // C is the lane that owns band column y = pos - begin_a - x + band.

The bytes of a run.  hi_a = a_base + pos, hi_b = b_base + begin_b + x are the bases of the run's first step.  Lane k of the wavefront
holds 2-bit word (w0 - k) of either sequence, w0 = ((hi - 15) >> 4) + 1 when a window is (re)filled; a window is kept while the run
fits it.  Chunk j = bases [hi - 16 j - 15, hi - 16 j]: lane da + j makes it from its own word and the one above, shifted by
((hi - 15) & 15) bases, da = w0_a - ((hi_a - 15) >> 4); b's chunk comes from lane lane + db - da.  Base p of the chunk is step
s = 16 j + 15 - p of the run; p0 = 16 j + 16 - n is the first base that belongs to it, lanes with j < 0 have none.  The op is MATCH where
the 2-bit codes are equal or either side is N, else MISMATCH; byte len + s is written iff len + s < cap.

Where a run is cut changes no byte (test_ops_walk_model_cpu.py runs every case at several cache depths); the device's cuts also depend
on which strips of direction-free blocks exist, which this model does not know -- so `runs` of the statistics is bounded, not equal,
in the GPU tests, and ops_by_run / ops_by_step, which do not depend on the cuts, are equal.
"""
GAP_A, GAP_B, MATCH, MISMATCH = 0, 1, 2, 3
OPS = "ABMX"
TB_DEPTH = 16
LANES = 64
UNTOUCHED = 0xEE


def _words2(codes, base):
    """the packed plane: 16 bases per 32-bit word, base i of the array = code i - base of the sequence (N packs as 0, zeros around)"""
    def word(w):
        v = 0
        for p in range(16):
            i = 16 * w + p - base
            if 0 <= i < len(codes) and codes[i] < 4:
                v |= codes[i] << (2 * p)
        return v
    return word


def _words_n(codes, base):
    """the N plane: 32 bases per word"""
    def word(w):
        v = 0
        for p in range(32):
            i = 32 * w + p - base
            if 0 <= i < len(codes) and codes[i] == 4:
                v |= 1 << p
        return v
    return word


def _alignbit(hi, lo, shift):
    return (((hi << 32) | lo) >> shift) & 0xFFFFFFFF


class _Window:
    """lane k holds word (w0 - k); refilled when the run does not fit it"""

    def __init__(self, word):
        self.word, self.w0, self.v = word, None, [0] * LANES

    def fit(self, w_top, w_bot):
        if self.w0 is None or w_top + 1 > self.w0 or w_bot < self.w0 - 63:
            self.w0 = w_top + 1
            self.v = [self.word(self.w0 - k) for k in range(LANES)]


def replay(ops_fwd, begin_a, begin_b, a, b, band, task_begin_a, task_begin_b, cap=None, C=17, a_base=0, b_base=0, depth=TB_DEPTH):
    """-> dict(bytes: the edit string in traceback order as the device leaves it in a buffer of max(cap, length) + 16 bytes pre-filled
    with UNTOUCHED, length, ops_by_run, ops_by_step, runs, run_lengths (of every run iteration with n > 0), gap_ops)"""
    rev = [OPS.index(ch) for ch in reversed(ops_fwd)]
    length = len(rev)
    cap = length if cap is None else cap
    n_diag = sum(1 for o in rev if o >= MATCH)
    pos = begin_a + n_diag + rev.count(GAP_B) - 1
    x = begin_b + n_diag + rev.count(GAP_A) - 1 - task_begin_b
    y = pos - task_begin_a - x + band
    out = bytearray([UNTOUCHED]) * (max(cap, length) + 16)
    wa_, wb_ = _Window(_words2(a, a_base)), _Window(_words2(b, b_base))
    na_, nb_ = _words_n(a, a_base), _words_n(b, b_base)
    code = lambda s, i: s[i] if 0 <= i < len(s) else 0
    ln = ops_by_run = ops_by_step = runs = 0
    run_lengths = []
    cblk0 = cl = cg = None

    def put(at, op):
        if at < cap:
            out[at] = op

    def gap(op):
        nonlocal x, y, pos, ln, ops_by_step
        put(ln, op)
        if op == GAP_A:
            x -= 1; y += 1
        else:
            y -= 1; pos -= 1
        ln += 1
        ops_by_step += 1

    while ln < length:
        assert x >= 0 and pos >= 0 and 0 <= y <= 2 * band, (x, pos, y)
        op = rev[ln]
        if x == 0 or pos == 0:
            if op >= MATCH:
                pa, pb = code(a, pos), code(b, task_begin_b + x)
                is_match = pa == pb or pa == 4 or pb == 4
                assert (op == MATCH) == is_match, (ln, pa, pb, op)
                put(ln, MATCH if is_match else MISMATCH)
                x -= 1; pos -= 1
                ln += 1
                ops_by_step += 1
            else:
                gap(op)
            continue
        l, c = divmod(y, C)
        tau = x + l
        blk, r = tau >> 4, tau & 15
        g = c >> 2
        k0 = None if cblk0 is None else cblk0 - blk
        if l != cl or g != cg or k0 is None or k0 < 0 or k0 >= depth:
            cblk0, cl, cg, k0 = blk, l, g, 0
        held = (r + 1) + 16 * min(depth - 1 - k0, blk)   # rows of this column in the cache, from the walk down (no block below 0)
        n_run = 0
        while ln + n_run < length and rev[ln + n_run] >= MATCH and n_run < held:
            n_run += 1
        stopped = n_run < held                           # the run ended at a gap whose direction word is in the cache
        n = min(n_run, x, pos)
        if n == 0:
            assert op < MATCH
            gap(op)
            continue
        hi_a, hi_b = a_base + pos, b_base + task_begin_b + x
        w_a, w_b = (hi_a - 15) >> 4, (hi_b - 15) >> 4
        wa_.fit(w_a, (hi_a - n - 15) >> 4)
        wb_.fit(w_b, (hi_b - n - 15) >> 4)
        da, db = wa_.w0 - w_a, wb_.w0 - w_b
        assert da >= 1 and db >= 1
        sh_a, sh_b = ((hi_a - 15) & 15) * 2, ((hi_b - 15) & 15) * 2
        a16 = [_alignbit(wa_.v[k - 1] if k else 0, wa_.v[k], sh_a) for k in range(LANES)]
        b16s = [_alignbit(wb_.v[k - 1] if k else 0, wb_.v[k], sh_b) for k in range(LANES)]
        for lane in range(LANES):
            j = lane - da
            p0 = 16 * j + 16 - n
            msk = 0x55555555 if p0 <= 0 else (0 if p0 >= 16 else (0x55555555 << (2 * p0)) & 0xFFFFFFFF)
            if j < 0:
                msk = 0
            if not msk:
                continue
            b16 = b16s[(lane + db - da) & 63]            # ds_bpermute: lane index modulo 64
            xr = a16[lane] ^ b16
            ne = (xr | (xr >> 1)) & 0x55555555
            lo_a, lo_b = hi_a - 15 - 16 * j, hi_b - 15 - 16 * j
            nn16 = (_alignbit(na_((lo_a >> 5) + 1), na_(lo_a >> 5), lo_a & 31) | _alignbit(nb_((lo_b >> 5) + 1), nb_(lo_b >> 5), lo_b & 31)) & 0xFFFF
            for p in range(16):
                if (nn16 >> p) & 1:
                    ne &= ~(1 << (2 * p))
            eq = ~ne & msk
            for p in range(16):
                if (msk >> (2 * p)) & 1:
                    s = 16 * j + 15 - p
                    opb = MATCH if (eq >> (2 * p)) & 1 else MISMATCH
                    assert rev[ln + s] == opb, (ln, s, lane, j, p, rev[ln + s], opb)
                    put(ln + s, opb)
        x -= n; pos -= n
        ln += n
        ops_by_run += n
        runs += 1
        run_lengths.append(n)
        if stopped and n == n_run and x >= 1 and pos >= 1 and ln < length:
            assert rev[ln] < MATCH
            gap(rev[ln])
    return dict(bytes=bytes(out), length=length, ops_by_run=ops_by_run, ops_by_step=ops_by_step, runs=runs, run_lengths=run_lengths,
                gap_ops=sum(1 for o in rev if o < MATCH))


def split(ops_fwd, begin_a, begin_b, task_begin_b):
    """(ops_by_run, ops_by_step) alone, which no cut of the runs changes: a diagonal step counts as a run's where the cell it is taken
    from has x >= 1 and pos >= 1"""
    n_diag = sum(1 for ch in ops_fwd if ch in "MX")
    pos = begin_a + n_diag + ops_fwd.count("B") - 1
    x = begin_b + n_diag + ops_fwd.count("A") - 1 - task_begin_b
    by_run = 0
    for ch in reversed(ops_fwd):
        if ch in "MX":
            by_run += x >= 1 and pos >= 1
            x -= 1; pos -= 1
        elif ch == "A":
            x -= 1
        else:
            pos -= 1
    return by_run, len(ops_fwd) - by_run


def expected_bytes(ops_fwd, cap):
    """what a buffer of max(cap, length) + 16 bytes holds after the walk, by definition: the string reversed, clipped at cap"""
    rev = bytes(OPS.index(ch) for ch in reversed(ops_fwd))
    n = max(cap, len(rev)) + 16
    return rev[:cap] + bytes([UNTOUCHED]) * (n - min(cap, len(rev)))
