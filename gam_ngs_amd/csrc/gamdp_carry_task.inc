// The DP of one find_alignment call as k_carry runs it (gamdp_carry.hip has the argument): a cell's summary, the wavefront's state and
// carry_task<C>, which takes one task from its descriptor to its DevResult.  Included inside namespace gamdp { namespace {, behind
// gamdp_score_common.inc, by gamdp_carry.hip (k_carry: a batch of tasks), gamdp_chain_carry.hip (k_chain_c: the calls of a merge
// block's main chain, one after the other) and gamdp_carry_ops.hip (k_carry_f: k_carry with the edit string's fingerprint as a sixth
// field of the summary, FP = true below; with FP = false nothing of it exists); nothing of the alignment kernels is used here.
constexpr int K_DEAD = -32;            // what a column beyond the band's last adds on its diagonal in the fast blocks
// The dead-column argument of k_score (gamdp_score.hip), here needed in its strict form: what comes back into the band's last column
// through `up` from the columns beyond it is at least 12 below that column's own diagonal candidate, so the last column's value never
// EQUALS its `up` and the fast step rule never takes an `up` the reference does not have there (:292, :303)
static_assert(-2 * S_GAP >= 16 && -(S_MAX_SCORE + K_DEAD) >= 16 && 16 + S_MIN_SCORE >= 12, "the band's last column could equal its dead `up`");
// What the kernel reads outside the sequences (the planes are padded by SEQ_PAD_BASES on either side).  In front of a: band bases
// (pos = begin_a - band + ...), fetched as whole words.  Behind a: lane 63 takes the base at begin_a - band + 63 (C-1) + C + tau with
// tau < X + LE, X <= |a| + band - begin_a (preflight_hd), LE <= 63; a fast block fetches the window of the block behind it, which
// begins at a row-time <= X - 1 (K_BLOCK row-times on from one that is fast); a fetch reads 64 bases on from its index (load_win) -- at
// C = 17 at most 63 * 16 + 17 + 63 + 64 bases behind |a|.  b: rows begin_b + tau, X <= |b| - begin_b.
constexpr int K_BLOCK = 32;            // row-times of a fast block: what one fetch of 32 bases feeds
static_assert(543 + 64 <= SEQ_PAD_BASES && 63 * 16 + 17 + 63 + 64 + 64 <= SEQ_PAD_BASES && K_BLOCK <= 32, "k_carry's fetches would leave the padded planes");
constexpr int K_XSHIFT = 2048;         // cell code x * 2048 + y
static_assert(543 * 2 + 2 < K_XSHIFT && (int64_t)500001 * K_XSHIFT + K_XSHIFT < (int64_t)1 << 31, "a cell code does not fit an int32");

enum : int { OP_DIAG = 0, OP_UP = 1, OP_LEFT = 2 };   // MATCH or MISMATCH (x--), GAP_A (x--, y++), GAP_B (y--)

// The summary of a cell.  FP: with the fingerprint of the forward edit string of the traceback that starts in the cell
// (gamdp_ops_fingerprint, include/gamdp.h: F(s . e) = F(s) * K_FP_MULT + e + 1 mod 2^32, F(empty) = 0).  The forward string of a cell
// is that of the cell its step leads to plus the step's op, so the field is updated as the others are: one step per cell.  Five
// initialisers leave it 0, the fingerprint of the empty string.
template <bool FP> struct SumT;
template <> struct SumT<false> { int B, ln, nm, F, Lc; };
template <> struct SumT<true> { int B, ln, nm, F, Lc; u32 fp; };
typedef SumT<false> Sum;
constexpr u32 K_FP_MULT = 0x9E3779B1u;   // GAMDP_OPS_FP_MULT
template <bool FP>
__device__ __forceinline__ SumT<FP> sum_from_lane_below(const SumT<FP>& s)
{
    SumT<FP> r = {from_lane_below(s.B), from_lane_below(s.ln), from_lane_below(s.nm), from_lane_below(s.F), from_lane_below(s.Lc)};
    if constexpr (FP) r.fp = (u32)from_lane_below((int)s.fp);
    return r;
}
template <bool FP>
__device__ __forceinline__ SumT<FP> sum_from_lane_above(const SumT<FP>& s)
{
    SumT<FP> r = {from_lane_above(s.B), from_lane_above(s.ln), from_lane_above(s.nm), from_lane_above(s.F), from_lane_above(s.Lc)};
    if constexpr (FP) r.fp = (u32)from_lane_above((int)s.fp);
    return r;
}
template <bool FP>
__device__ __forceinline__ SumT<FP> pick(const bool d, const SumT<FP>& sd, const bool u, const SumT<FP>& su, const SumT<FP>& sl)
{
    SumT<FP> r = {d ? sd.B : (u ? su.B : sl.B), d ? sd.ln : (u ? su.ln : sl.ln), d ? sd.nm : (u ? su.nm : sl.nm), d ? sd.F : (u ? su.F : sl.F), d ? sd.Lc : (u ? su.Lc : sl.Lc)};
    if constexpr (FP) r.fp = d ? sd.fp : (u ? su.fp : sl.fp);
    return r;
}
// one more op in front of the traceback t: `op` at the cell with code `cur`; `match`: it is a MATCH (:239, :274), which only an
// OP_DIAG is.  The fingerprint takes the op's public code + 1: GAP_A 0 (OP_UP), GAP_B 1 (OP_LEFT), MATCH 2, MISMATCH 3.
static_assert(OP_UP == 0 + 1 && OP_LEFT == 1 + 1, "a gap's OP_ is its GAMDP_OP_ code + 1");
template <bool FP>
__device__ __forceinline__ SumT<FP> step_on(SumT<FP> t, const bool match, const int cur, const int op)
{
    t.F = (match && t.nm == 0) ? cur : t.F;
    t.Lc = match ? cur : t.Lc;
    t.nm += match ? 1 : 0;
    t.ln += 1;
    if constexpr (FP) t.fp = t.fp * K_FP_MULT + (u32)(match ? 2 + 1 : (op == OP_DIAG ? 3 + 1 : op));
    return t;
}

// the wavefront's state: WaveBase (gamdp_score_common.inc) holds the values, this the summaries
template <int C, bool FP> struct FpCols { u32 sfp[C]; };   // the sixth field's register array ...
template <int C> struct FpCols<C, false> {};              // ... which a kernel without it does not have
template <int C, bool FP = false>
struct CWave : WaveBase<C, K_DEAD>, FpCols<C, FP> {
    typedef SumT<FP> Sum;
    using B = WaveBase<C, K_DEAD>;
    using B::h; using B::a5; using B::dead; using B::leftadd; using B::row;
    int sB[C], sln[C], snm[C], sF[C], sLc[C];   // the summaries of the cells h[], a register array per field
    Sum bs;                                     // the summary of the end-cell search's best candidate (bv, bk)

    __device__ __forceinline__ Sum sum(const int c) const
    {
        Sum r = {sB[c], sln[c], snm[c], sF[c], sLc[c]};
        if constexpr (FP) r.fp = this->sfp[c];
        return r;
    }
    __device__ __forceinline__ void set_sum(const int c, const Sum& t)
    {
        sB[c] = t.B; sln[c] = t.ln; snm[c] = t.nm; sF[c] = t.F; sLc[c] = t.Lc;
        if constexpr (FP) this->sfp[c] = t.fp;
    }

    // Row-time k of a fast block (every lane that holds band columns is at a row >= 1 below the last, every pos inside (0, |a|), no
    // candidate of the end-cell search goes by): every cell is sw[i][j] = max(sw[i-1][j] + S, sw[i-1][j+1] + gap, sw[i][j-1] + gap)
    // (:160-164), kept as sw[i][j] + 16 i + 8 j so that the gap terms add nothing and the diagonal adds the unsigned field S + 16.
    // The traceback's step from such a cell (:265-307, x > 0, pos > 0): diag if the value equals the diagonal candidate, else up if
    // 0 < y < Y-1 and it equals `up`, else left; y == 0: up; y == Y-1: left.  All three candidates carry the same offset, so the
    // comparisons are those of the reference.  Column 0 has no `left` candidate (S_NEG in lane 0), so "not diag" is "equals up" there;
    // the last column never equals its dead `up` (see K_DEAD).  The a window moves by one register per row-time (a5[c] <- a5[c+1]).
    __device__ __forceinline__ void fast_cell(const int c, const int uv, const Sum& su, const int lv, const Sum& sl, const int cur)
    {
        const int f = cell_score16(row, a5[c]);
        const int dv = h[c] + f + dead[c];
        const int v = max3i(dv, uv, lv);
        const bool isd = v == dv, isu = v == uv;
        set_sum(c, step_on(pick(isd, sum(c), isu, su, sl), isd && f != S_MIN_SCORE + 16, cur, isd ? OP_DIAG : (isu ? OP_UP : OP_LEFT)));
        h[c] = v;
    }
    __device__ __forceinline__ void fast_step(const SWin& wa, const SWin& wb, const int k, const int cur0)
    {
        this->take_row(wb, k);
        const int L = from_lane_below(h[C - 1]) + leftadd;
        const Sum Ls = sum_from_lane_below(sum(C - 1));
        fast_cell(0, h[1], sum(1), L, Ls, cur0);
        const int U = from_lane_above(h[0]);   // (lane 63 gets 0, for a column that is always dead: 2*band+1 is odd, 64*C even)
        const Sum Us = sum_from_lane_above(sum(0));
#pragma unroll
        for (int c = 1; c < C - 1; ++c) fast_cell(c, h[c + 1], sum(c + 1), h[c - 1], sum(c - 1), cur0 + c);
        fast_cell(C - 1, U, Us, h[C - 2], sum(C - 2), cur0 + C - 1);
        this->advance(wa, k);
    }

    // One row-time by the reference's rules, cell by cell: the value (:112-168), then the step the traceback takes from
    // the cell (:229-308) and the summary it leaves.  Lanes that are not at a row of the matrix, and cells outside a, compute along:
    // a traceback never enters them (pos does not grow along it, and a cell with x < 0, y < 0 or pos < 0 ends it).
    __device__ __forceinline__ void slow_step(const STask& t, const int tau, const int lane)
    {
        this->slow_take_row(t, tau);
        const int i = tau - lane;
        const int p0 = t.A0 + tau + (C - 1) * lane, j0 = C * lane;
        const bool row0 = i == 0;
        const int L = from_lane_below(h[C - 1]);   // (lane 0: unused, its column 0 has no left neighbour)
        const Sum Ls = sum_from_lane_below(sum(C - 1));
        int U = 0;
        Sum Us = {0, 0, 0, 0, 0};
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int pos = p0 + c, j = j0 + c;
            const int sc = cell_score16(row, a5[c]) - 16;
            const int leftv = c > 0 ? h[c > 0 ? c - 1 : 0] : L;
            const int upv = c < C - 1 ? h[c < C - 1 ? c + 1 : 0] : U;
            const Sum lefts = c > 0 ? sum(c > 0 ? c - 1 : 0) : Ls;
            const Sum ups = c < C - 1 ? sum(c < C - 1 ? c + 1 : 0) : Us;
            const int dold = h[c];
            // The value, by the rules of slow_value (gamdp_score_common.inc, where each is explained), in this kernel's own text: why
            // it is not the call is in that file's header.  row 0 (:112-132) ...
            const bool in_a = (u32)pos < (u32)t.alen;
            const bool has_left = pos > 0 && j > 0;
            const bool r0_gap = t.fs ? (u32)pos <= (u32)S_MAXGAP : in_a;                 // :116
            const bool r0_forced = t.fs && pos > S_MAXGAP && pos < t.alen;               // :125
            const int v_gap = has_left ? max3i(sc, S_GAP, leftv) : max(S_GAP, sc);
            const int v_forced = has_left ? max(sc, leftv) : sc;
            const int v0 = r0_gap ? v_gap : (r0_forced ? v_forced : 0);
            // ... rows >= 1 (:141-168)
            const int up = j < t.Y - 1 ? upv + S_GAP : S_NEG;
            const int left = pos == 0 ? ((t.fs && i > S_MAXGAP) ? S_NEG : S_GAP) : (j > 0 ? leftv + S_GAP : S_NEG);
            const int vn = in_a ? max3i(dold + sc, up, left) : 0;
            const int v = row0 ? v0 : vn;
            // the traceback's step from this cell.  pos == 0 (:229-262): diag is the score alone, left the gap score (nothing for a
            // forced start beyond FORCE_MAXGAP_LEN rows), and the last column goes left whatever it holds
            const int op_p0 = v == sc ? OP_DIAG : ((j == t.Y - 1 || v == ((t.fs && i > S_MAXGAP) ? S_NEG : S_GAP)) ? OP_LEFT : OP_UP);
            // pos > 0 (:263-308): row 0 has no cell above (diag from 0; up the gap score, or nothing for a forced start beyond
            // FORCE_MAXGAP_LEN, :269-270); columns 0 and Y-1 compare with the diagonal only
            const int t_diag = (row0 ? 0 : dold) + sc;
            const int t_up = row0 ? ((t.fs && pos > S_MAXGAP) ? S_NEG : S_GAP) : (j < t.Y - 1 ? upv + S_GAP : S_GAP);
            const int op_in = v == t_diag ? OP_DIAG : (j > 0 && j < t.Y - 1) ? (v == t_up ? OP_UP : OP_LEFT) : (j < t.Y - 1 ? OP_UP : OP_LEFT);
            const int op = pos == 0 ? op_p0 : op_in;
            // the cell the step leads to: outside (x < 0, y < 0 or pos < 0) the traceback ends and the summary begins (:227, :321)
            const bool ends = op == OP_DIAG ? (row0 || pos == 0) : op == OP_UP ? row0 : (j == 0 || pos == 0);
            const int bcode = op == OP_DIAG ? i * K_XSHIFT + j + 1 : op == OP_UP ? i * K_XSHIFT + j + 2 : (i + 1) * K_XSHIFT + j;
            Sum nt = pick(op == OP_DIAG, sum(c), op == OP_UP, ups, lefts);
            if (ends) nt = {bcode, 0, 0, 0, 0};
            set_sum(c, step_on(nt, op == OP_DIAG && sc != S_MIN_SCORE, i * K_XSHIFT + j, op));
            h[c] = v;
            if (c == 0) { U = from_lane_above(h[0]); Us = sum_from_lane_above(sum(0)); }
        }
        this->search_end_cell(t, i, p0, j0, [&](const int c) { bs = sum(c); });
        this->slow_advance();
    }
};

// One task.  Inlined into its kernel: a call would cost the callee-saved registers' stack slots, and the kernels are to use no private
// memory.  The result comes back wave-uniform (every field is made of scalars and of values read from one lane); the caller stores it.
// FP: *fp takes the fingerprint of the edit string, 0 unless the status is OK (also wave-uniform).
template <int C, bool FP = false>
__device__ __forceinline__ DevResult carry_task(const DevTask& dt, const int lane, u32* const fp = nullptr)
{
    typedef SumT<FP> Sum;
    const STask t = stask_of(dt);
    CWave<C, FP> w;
    if constexpr (FP) *fp = 0;
    w.seed(t, dt, lane);
#pragma unroll
    for (int c = 0; c < C; ++c) w.set_sum(c, {0, 0, 0, 0, 0});
    w.bs = {0, 0, 0, 0, 0};
    // The task's row-times: runs of fast blocks (the bases of a block are fetched while the block before it is computed) where
    // FastRange allows them, slow_step for all others.  Written out here and not shared: see gamdp_score_common.inc.
    constexpr int G = K_BLOCK;
    const int LE = (t.Y - 1) / C;
    const FastRange fast(t, C, G, LE);
    const int T = t.X + LE;   // lane LE is at the last row at row-time X - 1 + LE
    for (int tau = 0; tau < T;) {
        if (fast(tau)) {
            SWin wa = load_win_uniform(t.a2, t.an, w.aidx + tau), wb = load_win_uniform(t.b2, t.bn, w.bidx + tau);
            w.to_block(tau, lane);
            int cur = (tau - lane) * K_XSHIFT + C * lane;   // the code of the lane's column 0 at this row-time
            do {
                const SWin na = load_win(t.a2, t.an, w.aidx + tau + G), nb = load_win(t.b2, t.bn, w.bidx + tau + G);   // (all lanes the same words)
#pragma nounroll
                for (int k = 0; k < G; ++k) {
                    w.fast_step(wa, wb, k, cur);
                    cur += K_XSHIFT;
                }
                wa = win_uniform(na); wb = win_uniform(nb);
                tau += G;
            } while (fast(tau));
            w.from_block(tau, lane);
            w.sa = wa; w.sb = wb; w.used = 0;
        } else {
            w.slow_step(t, tau, lane);
            ++tau;
        }
    }

    // the winner of the end-cell search (best_of_wave and end_of_key of gamdp_score_common.inc in this kernel's own text, see that
    // file's header), and its summary from the lane that holds it (a scan position belongs to one cell, so to one lane)
    int bv = w.bv, bk = w.bk;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const int ov = __shfl_xor(bv, o, 64), ok = __shfl_xor(bk, o, 64);
        if (ov > bv || (ov == bv && ok < bk)) { bv = ov; bk = ok; }
    }
    bv = __builtin_amdgcn_readfirstlane(bv);
    bk = __builtin_amdgcn_readfirstlane(bk);
    DevResult res;
    res.begin_a = res.begin_b = res.score = 0;
    res.n_match = res.length = 0;
    res.first_a = res.first_b = res.last_a = res.last_b = 0;
    u32 status = S_ST_EMPTY;   // no end cell (:215)
    u32 found = 0;
    if (bk != S_KEY_NONE) {
        const int x = bk < t.Y ? t.X - 1 : t.iA + (bk - t.Y);
        const int pos = bk < t.Y ? t.A0 + x + bk : t.ea;
        if (pos >= t.alen) status = S_ST_OUT_OF_RANGE;   // the traceback's a.at(pos) throws
        else {
            status = S_ST_OK;
            const unsigned long long holders = __ballot(w.bk == bk);
            const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)holders) - 1);
            Sum e;
            e.B = __builtin_amdgcn_readlane(w.bs.B, src); e.ln = __builtin_amdgcn_readlane(w.bs.ln, src); e.nm = __builtin_amdgcn_readlane(w.bs.nm, src);
            e.F = __builtin_amdgcn_readlane(w.bs.F, src); e.Lc = __builtin_amdgcn_readlane(w.bs.Lc, src);
            if constexpr (FP) *fp = (u32)__builtin_amdgcn_readlane((int)w.bs.fp, src);
            const int xb = e.B / K_XSHIFT, yb = e.B % K_XSHIFT - 1;
            res.begin_a = t.A0 + xb + yb; res.begin_b = dt.begin_b + xb;   // :321
            res.score = bv;
            res.n_match = (u32)e.nm; res.length = (u32)e.ln;
            if (e.nm > 0) {
                res.first_a = t.A0 + e.F / K_XSHIFT + e.F % K_XSHIFT; res.first_b = dt.begin_b + e.F / K_XSHIFT;
                res.last_a = t.A0 + e.Lc / K_XSHIFT + e.Lc % K_XSHIFT; res.last_b = dt.begin_b + e.Lc / K_XSHIFT;
                found = 3;
            } else {
                res.first_a = pos + 1; res.first_b = dt.begin_b + x + 1;
                res.last_a = res.begin_a; res.last_b = res.begin_b;
            }
        }
    }
    res.flags = found | (status << 8) | ((u32)C << CARRY_COLS_SHIFT);   // (the instantiation, for gamdp_ctx_carry_info)
    return res;
}
