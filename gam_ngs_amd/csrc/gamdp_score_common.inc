// What k_score (gamdp_score.hip) and k_carry / k_chain_c (gamdp_carry_task.inc) share, each stated once: the constants of the
// reference, the sequence windows, the scoring-matrix rows, the lane shifts, what a wavefront knows of its task (STask, stask_of),
// the wavefront's state (WaveBase), the candidacy of a cell in the end-cell search (search_end_cell) and the fast-range rule
// (FastRange).  The two are one implementation of these rules, not two: what they check independently is the alignment kernels
// (gamdp_kernel.hip, kernel_*.inc, gamdp_wide.hip), of which nothing is used here or there.
// Three pieces are stated here and used by k_score alone, with carry_task keeping its own text of them: the value of a cell
// (slow_value), the wave reduction and the decoding of the winning key (best_of_wave, end_of_key).  A fourth, the loop over a
// task's row-times, is written out in score_task and in carry_task.  Shared, each compiled to the same instructions in another
// order and layout (how the prefetch loads are waited for, where the record stores sit in k_chain_c's call loop) and measured
// slower than the spread of the timings allows: DESIGN.md section 4, "What is stated once", has the figures.
// Included inside namespace gamdp { namespace { of either file.
constexpr int S_NEG = -(1 << 30);      // "no such neighbour": below every value a cell can take, and far from wrapping
constexpr int S_GAP = -8;              // GAP_SCORE, my_alignment.hpp:46
constexpr int S_MAXGAP = 10;           // FORCE_MAXGAP_LEN, banded_smith_waterman.hpp:37
constexpr int S_KEY_NONE = 0x7fffffff;
enum : u32 { S_ST_OK = 0, S_ST_EMPTY = 1, S_ST_OUT_OF_RANGE = 2 };   // GAMDP_ST_* (include/gamdp.h)
constexpr int S_MIN_SCORE = -4, S_MAX_SCORE = 5;   // of the scoring matrix (:80-88)
constexpr int S_POS_MAX = 0x7fff0000;  // above every position of a task (|a| < 2^31 - 2^20, rows + band columns beyond it < 2^19 + 2^11)

typedef const __attribute__((address_space(1))) u32* splane;

// 32 bases from base idx on (any alignment; idx may be negative or beyond the sequence: the planes are padded, gamdp_dev.h): base k's
// code at bits [2k, 2k+2) of hi:lo, its N flag at bit k of n
struct SWin { u32 lo, hi, n; };
__device__ __forceinline__ SWin load_win(splane p2, splane pn, const int64_t idx)
{
    const int64_t w = idx >> 4, wn = idx >> 5;
    const u32 sh = (u32)(idx & 15) * 2u;
    const u32 x0 = p2[w], x1 = p2[w + 1], x2 = p2[w + 2];
    SWin r;
    r.lo = __builtin_amdgcn_alignbit(x1, x0, sh);
    r.hi = __builtin_amdgcn_alignbit(x2, x1, sh);
    r.n = __builtin_amdgcn_alignbit(pn[wn + 1], pn[wn], (u32)(idx & 31));
    return r;
}
// a window all lanes fetched alike, into scalar registers, so that what is taken from its three words is scalar work
__device__ __forceinline__ SWin win_uniform(const SWin& w)
{
    return {(u32)__builtin_amdgcn_readfirstlane((int)w.lo), (u32)__builtin_amdgcn_readfirstlane((int)w.hi), (u32)__builtin_amdgcn_readfirstlane((int)w.n)};
}
// load_win at an index all lanes share
__device__ __forceinline__ SWin load_win_uniform(splane p2, splane pn, const int64_t idx) { return win_uniform(load_win(p2, pn, idx)); }
__device__ __forceinline__ u32 win_code(const SWin& w, const int k) { return ((k < 16 ? w.lo : w.hi) >> (2 * (k & 15))) & 3u; }
__device__ __forceinline__ bool win_isn(const SWin& w, const int k) { return ((w.n >> k) & 1u) != 0; }

// The scoring matrix (:80-88) as one word per b base: five 5-bit fields, field k = S[k][b] (5 equal, -4 different, 0 when exactly
// one is N), each + 16 so that it is unsigned (what the fast blocks add: see fast_step).  A cell's score is the field its a base
// selects: one v_bfe_u32 with the a base kept as the offset 5 * code.
constexpr u32 S_ROW16_ACGT = 12u | (12u << 5) | (12u << 10) | (12u << 15) | (16u << 20);   // -4 four times, 0 against N, + 16
constexpr u32 S_ROW16_N = 16u | (16u << 5) | (16u << 10) | (16u << 15) | (21u << 20);
__device__ __forceinline__ u32 score_row16(const u32 code2, const bool isn) { return isn ? S_ROW16_N : (S_ROW16_ACGT ^ (25u << (5u * code2))); }   // 12 ^ 25 = 21
__device__ __forceinline__ int a_field(const u32 code2, const bool isn) { return isn ? 20 : (int)(5u * code2); }
__device__ __forceinline__ int cell_score16(const u32 row, const int field) { return (int)__builtin_amdgcn_ubfe(row, (u32)field, 5u); }

__device__ __forceinline__ int from_lane_below(const int v) { return __builtin_amdgcn_update_dpp(0, v, 0x138, 0xf, 0xf, true); }   // lane l <- lane l-1 (wave_shr:1); lane 0 gets 0
__device__ __forceinline__ int from_lane_above(const int v) { return __builtin_amdgcn_update_dpp(0, v, 0x130, 0xf, 0xf, true); }   // lane l <- lane l+1 (wave_shl:1); lane 63 gets 0
// the same with the lane that has no neighbour taking `own` instead: where a sequence enters the wavefront
__device__ __forceinline__ int shift_in_from_below(const int own, const int v) { return __builtin_amdgcn_update_dpp(own, v, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ int shift_in_from_above(const int own, const int v) { return __builtin_amdgcn_update_dpp(own, v, 0x130, 0xf, 0xf, false); }
__device__ __forceinline__ int max3i(const int a, const int b, const int c) { return max(max(a, b), c); }

// what a task's wavefront knows of it: all wave-uniform
struct STask {
    splane a2, an, b2, bn;
    int A0;          // pos of (row 0, column 0): begin_a - band
    int alen, X, Y;
    int ea;          // end_a, clamped above every position
    int iA;          // first row of the anti-diagonal pos == end_a (:197)
    bool fs, fe;
};
__device__ __forceinline__ STask stask_of(const DevTask& dt)
{
    STask t;
    t.a2 = (splane)dt.a2; t.an = (splane)dt.an; t.b2 = (splane)dt.b2; t.bn = (splane)dt.bn;
    const int band = dt.band;
    t.A0 = dt.begin_a - band;
    t.alen = dt.alen; t.X = dt.X; t.Y = 2 * band + 1;
    t.ea = (int)min(dt.end_a, (int64_t)S_POS_MAX);
    const int64_t over = dt.end_a - ((int64_t)dt.begin_a + band);
    t.iA = over >= 0 ? (int)min(over, (int64_t)(1 << 30)) : 0;
    t.fs = (dt.flags & TF_FORCE_START) != 0; t.fe = (dt.flags & TF_FORCE_END) != 0;
    return t;
}

// The value of the cell at row i, band column j, position pos by the reference's rules: s is its score, diag / leftv / upv what
// sw[i-1][j], sw[i][j-1], sw[i-1][j+1] hold (anything where there is no such cell: the rules below do not read it then).  A cell
// outside a holds 0, as the reference's matrix does.
__device__ __forceinline__ int slow_value(const STask& t, const int i, const int j, const int pos, const int s, const int diag, const int leftv, const int upv)
{
    const bool in_a = (u32)pos < (u32)t.alen;
    // row 0 (:112-132): `left` is the neighbour itself, without a gap
    const bool has_left = pos > 0 && j > 0;
    const bool r0_gap = t.fs ? (u32)pos <= (u32)S_MAXGAP : in_a;                 // :116
    const bool r0_forced = t.fs && pos > S_MAXGAP && pos < t.alen;               // :125
    const int v_gap = has_left ? max3i(s, S_GAP, leftv) : max(S_GAP, s);
    const int v_forced = has_left ? max(s, leftv) : s;
    const int v0 = r0_gap ? v_gap : (r0_forced ? v_forced : 0);
    // rows >= 1 (:141-168).  At pos == 0 the cell above is outside a and holds 0, so `diag` is the plain form; `left` is the gap
    // score whatever the column (:147), or nothing once a forced start is more than FORCE_MAXGAP_LEN rows away (:151-156)
    const int up = j < t.Y - 1 ? upv + S_GAP : S_NEG;
    const int left = pos == 0 ? ((t.fs && i > S_MAXGAP) ? S_NEG : S_GAP) : (j > 0 ? leftv + S_GAP : S_NEG);
    const int vn = in_a ? max3i(diag + s, up, left) : 0;
    return i == 0 ? v0 : vn;
}

// The wavefront's state, DEAD being what the kernel's own static_assert allows for `dead`.  Lane l owns band columns [C*l, C*l + C)
// and is at row i = tau - l at row-time tau.
// The two sequences move through the wavefront one lane per row-time, so only its end lanes take new bases, and those are the
// same for all lanes (scalar work): lane l's row at row-time tau is lane l-1's of tau-1 (`row` comes up from the lane below,
// lane 0 takes b[begin_b + tau]), and the a base that enters lane l's window is the one lane l+1 has in column 1 (it comes down
// from the lane above, lane 63 takes a[A0 + tau + 63 (C-1) + C]).
template <int C, int DEAD>
struct WaveBase {
    int h[C];        // the lane's cells of the row it was at last
    int a5[C];       // 5 * code of the a bases its columns meet at this row-time (pos = A0 + tau + (C-1) * lane + c)
    int dead[C];     // fast blocks: 0, or DEAD for a column beyond the band's last (the lane holds C columns whatever the band)
    int leftadd;     // fast blocks: what column 0's `left` adds: 0, or S_NEG in lane 0 (no column left of it)
    u32 row;         // the scoring-matrix row (fields S + 16) of the lane's b base
    SWin sa, sb;     // the slow path's bases (wave-uniform): the a bases lane 63 takes and the b bases lane 0 takes, from row-time tau - used on
    int used;
    int64_t aidx, bidx;   // index of the a base lane 63 takes at row-time 0 / of the b base of row 0
    int bv, bk;           // best candidate of the end-cell search so far: value, scan position

    __device__ __forceinline__ void seed(const STask& t, const DevTask& dt, const int lane)
    {
        const int64_t ap = dt.a_base + t.A0 + (int64_t)(C - 1) * lane;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int64_t k = ap + c;
            h[c] = 0;
            a5[c] = a_field((t.a2[k >> 4] >> ((u32)(k & 15) * 2u)) & 3u, ((t.an[k >> 5] >> (u32)(k & 31)) & 1u) != 0);
            dead[c] = (C * lane + c >= t.Y) ? DEAD : 0;
        }
        leftadd = lane == 0 ? S_NEG : 0;
        aidx = dt.a_base + t.A0 + 63 * (C - 1) + C;
        bidx = dt.b_base + dt.begin_b;
        sa = load_win_uniform(t.a2, t.an, aidx);
        sb = load_win_uniform(t.b2, t.bn, bidx);
        used = 0;
        row = 0;
        bv = S_NEG; bk = S_KEY_NONE;
    }
    // into / out of the fast blocks' form (sw[i][j] + 16 i + 8 j, dead columns from S_NEG: see the kernels' fast_step) in front of
    // row-time tau: the lane's cells are those of row tau - 1 - lane
    __device__ __forceinline__ void to_block(const int tau, const int lane)
    {
#pragma unroll
        for (int c = 0; c < C; ++c) h[c] = dead[c] ? S_NEG : h[c] + 16 * (tau - 1 - lane) + 8 * (C * lane + c);
    }
    __device__ __forceinline__ void from_block(const int tau, const int lane)
    {
#pragma unroll
        for (int c = 0; c < C; ++c) h[c] -= 16 * (tau - 1 - lane) + 8 * (C * lane + c);
    }
    // a row-time begins: the row of base k of the b window comes in at lane 0 ...
    __device__ __forceinline__ void take_row(const SWin& wb, const int k) { row = (u32)shift_in_from_below((int)score_row16(win_code(wb, k), win_isn(wb, k)), (int)row); }
    // ... and ends: the a window moves on by one register, base k of the a window comes in at lane 63
    __device__ __forceinline__ void advance(const SWin& wa, const int k)
    {
        const int enters = shift_in_from_above(a_field(win_code(wa, k), win_isn(wa, k)), a5[1]);
#pragma unroll
        for (int c = 0; c < C - 1; ++c) a5[c] = a5[c + 1];
        a5[C - 1] = enters;
    }
    // the same for a row-time of the slow path, from its own windows: 32 bases, then the next fetch
    __device__ __forceinline__ void slow_take_row(const STask& t, const int tau)
    {
        if (used == 32) {
            sa = load_win_uniform(t.a2, t.an, aidx + tau);
            sb = load_win_uniform(t.b2, t.bn, bidx + tau);
            used = 0;
        }
        take_row(sb, used);
    }
    __device__ __forceinline__ void slow_advance() { advance(sa, used); ++used; }

    // The end-cell search (:174-212) over the cells h[] of a slow row-time (row i, positions from p0, columns from j0): last-row
    // cells with 0 <= pos <= end_a in column order, then the cells with pos == end_a by rows; `!found || value > max`, i.e. the
    // larger value, then the smaller scan position.  taken(c): column c is the best so far.
    template <class Taken>
    __device__ __forceinline__ void search_end_cell(const STask& t, const int i, const int p0, const int j0, Taken taken)
    {
        const bool active = i >= 0 && i < t.X;
        const bool last_row = active && !t.fe && i == t.X - 1;
        const bool on_diag = active && t.ea >= p0 && t.ea <= p0 + C - 1 &&
                             (!t.fe || (t.X >= S_MAXGAP + 1 && i >= t.X - 1 - S_MAXGAP));   // :201, an unsigned compare there
        if (__any(last_row || on_diag)) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int pos = p0 + c, j = j0 + c;
                const bool ok_row = last_row && j < t.Y && pos >= 0 && pos <= t.ea;
                const bool ok_diag = on_diag && j < t.Y && pos == t.ea;
                const int key = ok_row ? j : t.Y + (i - t.iA);
                const int v = h[c];
                if ((ok_row || ok_diag) && (v > bv || (v == bv && key < bk))) { bv = v; bk = key; taken(c); }
            }
        }
    }
};

// the search's winner over the wavefront, in scalar registers
__device__ __forceinline__ void best_of_wave(int& bv, int& bk)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const int ov = __shfl_xor(bv, o, 64), ok = __shfl_xor(bk, o, 64);
        if (ov > bv || (ov == bv && ok < bk)) { bv = ov; bk = ok; }
    }
    bv = __builtin_amdgcn_readfirstlane(bv);
    bk = __builtin_amdgcn_readfirstlane(bk);
}
// ... and the cell its scan position names: row x, position pos
struct SEnd { u32 status; int x, pos; };
__device__ __forceinline__ SEnd end_of_key(const STask& t, const int bk)
{
    if (bk == S_KEY_NONE) return {S_ST_EMPTY, 0, 0};   // no end cell (:215)
    const int x = bk < t.Y ? t.X - 1 : t.iA + (bk - t.Y);
    const int pos = bk < t.Y ? t.A0 + x + bk : t.ea;
    return {pos >= t.alen ? S_ST_OUT_OF_RANGE : S_ST_OK, x, pos};   // (out of range: the traceback's a.at(pos) throws)
}

// The G row-times from tau on are fast when, in lanes 0 .. LE (the lane that holds the band's last column): every row is >= 1 and
// every pos > 0 (lane 0, column 0 has the smallest); the highest row, lane 0's, is below the last; every pos < |a| (lane LE, column
// C-1 has the largest); and pos == end_a is in nobody's columns.  span = what the largest pos of the block is above the smallest of
// its first row-time.
struct FastRange {
    int f_lo, f_hi, d_lo, d_hi;
    __device__ __forceinline__ FastRange(const STask& t, const int C, const int G, const int LE)
    {
        const int span = G - 1 + (LE + 1) * (C - 1);
        f_lo = max(LE + 1, 1 - t.A0);
        f_hi = min(t.X - 1 - G, t.alen - t.A0 - span - 1);
        const int64_t d_hi64 = (int64_t)t.ea - t.A0;
        d_hi = (int)min(d_hi64, (int64_t)0x7fffffff);
        d_lo = (int)max(min(d_hi64 - span, (int64_t)0x7fffffff), (int64_t)-0x7fffffff);
    }
    __device__ __forceinline__ bool operator()(const int tau) const { return tau >= f_lo && tau <= f_hi && (tau < d_lo || tau > d_hi); }
};
