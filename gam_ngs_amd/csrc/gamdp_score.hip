// k_score: score and end cell of BandedSmithWaterman(band).find_alignment without the traceback (gamdp_score_batch, include/gamdp.h).
// A second implementation of the fill (banded_smith_waterman.cc:80-171) and of the end-cell search (:173-215), in plain int32, that
// shares no code with the alignment kernels (gamdp_kernel.hip, kernel_*.inc): its results are an independent check of theirs.
//
// One task per wavefront.  Lane l owns band columns [C*l, C*l + C) and is at row i = tau - l at row-time tau, so that what a cell
// needs of its neighbours is already there:
//   left  sw[i][j-1]    own column c-1 of this row-time; column 0 takes lane l-1's last column of row-time tau-1 (one lane shift);
//   diag  sw[i-1][j]    own column c of row-time tau-1;
//   up    sw[i-1][j+1]  own column c+1 of row-time tau-1; the last column takes lane l+1's column 0 of THIS row-time (its row is
//                       i-1), which every lane therefore computes first and hands down (the second lane shift).
// Nothing of the matrix goes to memory: a lane keeps the C cells of its row, and the end cell -- the maximum over the last row and
// over the anti-diagonal pos == end_a, first in scan order -- is searched while the cells go by, as a (value, key) pair per lane
// with key = scan position; one wave reduction at the end of the task.
//
// Most row-times of a long task touch nothing special: every lane is at a row >= 1, every position is inside (0, |a|), no candidate
// of the end-cell search goes by.  Those run a block of 9 to 17 at a time through fast_block (three instructions per cell in the source: bit-field extract, three-operand add, three-operand maximum); all others -- the first
// rows, positions <= 0 or >= |a|, the last row, the anti-diagonal -- go one by one through slow_step, which is the reference's rules
// written out cell by cell.
#include <hip/hip_runtime.h>

#include "gamdp_dev.h"

namespace gamdp {
namespace {

#include "gamdp_score_common.inc"   // constants, sequence windows, scoring rows, lane shifts, STask: shared with k_carry (gamdp_carry.hip)

constexpr int S_DEAD = -32;            // what a column beyond the band's last adds on its diagonal in the fast blocks (see fast_step)
// fast_step's argument: a value that leaves the band's last column through the columns beyond it comes back n rows lower having lost
// two gaps, and 16 or more for every further row (two more gaps, or a diagonal step of S + S_DEAD) -- more than the n diagonal steps
// of the last column itself can lose
static_assert(-2 * S_GAP > -S_MIN_SCORE && -2 * S_GAP >= 16 && -(S_MAX_SCORE + S_DEAD) >= 16 && 16 > -S_MIN_SCORE, "dead columns could win in the band's last column");
// What the kernel reads outside the sequences (the planes are padded by SEQ_PAD_BASES on either side).  In front of a: band bases
// (pos = begin_a - band + ...), a fetch of whole words.  Behind a: lane 63 takes the base at begin_a - band + 63 (C-1) + C + tau, tau <
// X + LE with X <= |a| + band - begin_a (preflight_hd) and LE <= 63, and a fetch reads 64 bases on from there (load_win: three 2-bit
// words, two N words) -- at C = 17 at most 63 * 16 + 17 + 63 + 64 bases behind |a|.  b: rows begin_b + tau, X <= |b| - begin_b.
static_assert(543 + 64 <= SEQ_PAD_BASES && 63 * 16 + 17 + 63 + 64 + 64 <= SEQ_PAD_BASES, "k_score's fetches would leave the padded planes");

// row-times a fast block takes: a multiple of C (the a window is back in natural order after it) that one fetch of 32 bases feeds
template <int C>
constexpr int S_BLOCK = C == 2 ? 16 : (C == 3 || C == 5) ? 15 : C;

template <int C>
struct SWave {
    int h[C];        // the lane's cells of the row it was at last
    int a5[C];       // 5 * code of the a bases its columns meet at this row-time (pos = A0 + tau + (C-1) * lane + c)
    int dead[C];     // fast blocks: 0, or -32 for a column beyond the band's last (the lane holds C columns whatever the band)
    int leftadd;     // fast blocks: what column 0's `left` adds: 0, or S_NEG in lane 0 (no column left of it)
    // The two sequences move through the wavefront one lane per row-time, so only its end lanes take new bases, and those are the
    // same for all lanes (scalar work): lane l's row at row-time tau is lane l-1's of tau-1 (`row` comes up from the lane below,
    // lane 0 takes b[begin_b + tau]), and the a base that enters lane l's window is the one lane l+1 has in column 1 (it comes down
    // from the lane above, lane 63 takes a[A0 + tau + 63 (C-1) + C]).
    u32 row;         // the scoring-matrix row (fields S + 16) of the lane's b base
    SWin sa, sb;     // slow_step's bases (wave-uniform): the a bases lane 63 takes and the b bases lane 0 takes, from row-time tau - used on
    int used;
    int64_t aidx, bidx;   // index of the a base lane 63 takes at row-time 0 / of the b base of row 0
    int bv, bk;           // best candidate of the end-cell search so far: value, scan position

    // Row-time K of a fast block: nothing special happens in any lane that holds band columns, so every cell is
    //     sw[i][j] = max(sw[i-1][j] + S, sw[i-1][j+1] + gap, sw[i][j-1] + gap)                              (:160-164)
    // and the block keeps sw[i][j] + 16 i + 8 j instead of sw[i][j] (to_block / from_block): the two gap terms then add nothing (16 - 8
    // and 8 cancel the gap score of -8) and the diagonal adds S + 16, which is what the unsigned field holds -- three instructions per
    // cell (v_bfe_u32, v_add3_u32, v_max3_i32), all int32, all exact (16 * 500 000 rows + 8 * 1 087 columns is far from 2^31).
    // The band's last column has no `up` (:165-166), but the lane computes the columns beyond it (`dead`) like any other.  They start
    // from S_NEG and add S_DEAD = -32 on their diagonal, so what they hold never wins in the last column: a value can only come back from them
    // through `up`, n >= 1 rows below where it left the last column and at least 16 n lower (8 to leave, 8 to return, 16 or more per
    // further row), while the last column's own diagonal loses 4 per row at the most.
    // K % C = row-times since the a window was in natural order: column c's base is a5[(c + K) % C], and the base that enters
    // replaces the one column 0 has just used.
    template <int K>
    __device__ __forceinline__ void fast_step(const SWin& wa, const SWin& wb)
    {
        row = (u32)shift_in_from_below((int)score_row16(win_code(wb, K), win_isn(wb, K)), (int)row);
        const int L = from_lane_below(h[C - 1]);
        h[0] = max3i(h[0] + cell_score16(row, a5[K % C]) + dead[0], h[1], L + leftadd);
        const int U = from_lane_above(h[0]);   // (lane 63 gets 0, for a column that is always dead: 2*band+1 is odd, 64*C even)
#pragma unroll
        for (int c = 1; c < C - 1; ++c) h[c] = max3i(h[c] + cell_score16(row, a5[(c + K) % C]) + dead[c], h[c + 1], h[c - 1]);
        h[C - 1] = max3i(h[C - 1] + cell_score16(row, a5[(C - 1 + K) % C]) + dead[C - 1], U, h[C - 2]);
        a5[K % C] = shift_in_from_above(a_field(win_code(wa, K), win_isn(wa, K)), a5[(1 + K) % C]);
    }
    // into / out of the fast blocks' form in front of row-time tau: the lane's cells are those of row tau - 1 - lane
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
    template <int K>
    __device__ __forceinline__ void fast_block(const SWin& wa, const SWin& wb)
    {
        if constexpr (K < S_BLOCK<C>) {
            fast_step<K>(wa, wb);
            fast_block<K + 1>(wa, wb);
        }
    }

    // One row-time by the reference's rules, cell by cell.  Lanes that are not at a row of the matrix compute along (nothing reads
    // what they make: see the header) and offer no candidates.  No branch depends on the lane except around the candidates: the
    // lane shifts need every lane.
    __device__ __forceinline__ void slow_step(const STask& t, const int tau, const int lane)
    {
        if (used == 32) {
            sa = load_win_uniform(t.a2, t.an, aidx + tau);
            sb = load_win_uniform(t.b2, t.bn, bidx + tau);
            used = 0;
        }
        row = (u32)shift_in_from_below((int)score_row16(win_code(sb, used), win_isn(sb, used)), (int)row);
        const int i = tau - lane;
        const int p0 = t.A0 + tau + (C - 1) * lane, j0 = C * lane;
        const bool row0 = i == 0;
        const int L = from_lane_below(h[C - 1]);   // (lane 0: unused, its column 0 has no left neighbour)
        int U = 0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int pos = p0 + c, j = j0 + c;
            const int s = cell_score16(row, a5[c]) - 16;
            const bool in_a = (u32)pos < (u32)t.alen;
            const int leftv = c > 0 ? h[c > 0 ? c - 1 : 0] : L;
            const int upv = c < C - 1 ? h[c < C - 1 ? c + 1 : 0] : U;
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
            const int vn = in_a ? max3i(h[c] + s, up, left) : 0;
            h[c] = row0 ? v0 : vn;
            if (c == 0) U = from_lane_above(h[0]);
        }
        // the end-cell search (:174-212): last-row cells with 0 <= pos <= end_a in column order, then the cells with pos == end_a by
        // rows; `!found || value > max`, i.e. the larger value, then the smaller scan position
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
                const int v = h[c];   // (a cell outside a holds 0, as the reference's matrix does)
                if ((ok_row || ok_diag) && (v > bv || (v == bv && key < bk))) { bv = v; bk = key; }
            }
        }
        // the window moves on by one base
        const int enters = shift_in_from_above(a_field(win_code(sa, used), win_isn(sa, used)), a5[1]);
#pragma unroll
        for (int c = 0; c < C - 1; ++c) a5[c] = a5[c + 1];
        a5[C - 1] = enters;
        ++used;
    }
};

// Out of line, like the phases of the alignment kernels (registers of the task allocated apart from the task loop's).  It also keeps
// the task's last statement (lane 0 stores the record) away from the loop's first (lane 0 takes the next task): see k_score.
template <int C>
__device__ __noinline__ void score_task(const DevTask& dt, ScoreRec* results, const int lane)
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
    const int LE = (t.Y - 1) / C;   // the lane that holds the band's last column

    SWave<C> w;
    const int64_t ap = dt.a_base + t.A0 + (int64_t)(C - 1) * lane;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int64_t k = ap + c;
        w.h[c] = 0;
        w.a5[c] = a_field((t.a2[k >> 4] >> ((u32)(k & 15) * 2u)) & 3u, ((t.an[k >> 5] >> (u32)(k & 31)) & 1u) != 0);
        w.dead[c] = (C * lane + c >= t.Y) ? S_DEAD : 0;
    }
    w.leftadd = lane == 0 ? S_NEG : 0;
    w.aidx = dt.a_base + t.A0 + 63 * (C - 1) + C;
    w.bidx = dt.b_base + dt.begin_b;
    w.sa = load_win_uniform(t.a2, t.an, w.aidx);
    w.sb = load_win_uniform(t.b2, t.bn, w.bidx);
    w.used = 0;
    w.row = 0;
    w.bv = S_NEG; w.bk = S_KEY_NONE;

    // The G row-times from tau on are fast when, in lanes 0 .. LE: every row is >= 1 and every pos > 0 (lane 0, column 0 has the
    // smallest); the highest row, lane 0's, is below the last; every pos < |a| (lane LE, column C-1 has the largest); and pos == end_a
    // is in nobody's columns.  span = what the largest pos of the block is above the smallest of its first row-time.
    constexpr int G = S_BLOCK<C>;
    const int span = G - 1 + (LE + 1) * (C - 1);
    const int f_lo = max(LE + 1, 1 - t.A0);
    const int f_hi = min(t.X - 1 - G, t.alen - t.A0 - span - 1);
    const int64_t d_hi64 = (int64_t)t.ea - t.A0;
    const int d_hi = (int)min(d_hi64, (int64_t)0x7fffffff), d_lo = (int)max(min(d_hi64 - span, (int64_t)0x7fffffff), (int64_t)-0x7fffffff);
    auto fast = [&](const int tau) { return tau >= f_lo && tau <= f_hi && (tau < d_lo || tau > d_hi); };
    const int T = t.X + LE;   // lane LE is at the last row at row-time X - 1 + LE
    for (int tau = 0; tau < T;) {
        if (fast(tau)) {
            // a run of fast blocks: the bases of a block are fetched while the block before it is computed
            SWin wa = load_win_uniform(t.a2, t.an, w.aidx + tau), wb = load_win_uniform(t.b2, t.bn, w.bidx + tau);
            w.to_block(tau, lane);
            do {
                const SWin na = load_win(t.a2, t.an, w.aidx + tau + G), nb = load_win(t.b2, t.bn, w.bidx + tau + G);   // (all lanes the same words)
                w.template fast_block<0>(wa, wb);
                wa.lo = (u32)__builtin_amdgcn_readfirstlane((int)na.lo); wa.hi = (u32)__builtin_amdgcn_readfirstlane((int)na.hi); wa.n = (u32)__builtin_amdgcn_readfirstlane((int)na.n);
                wb.lo = (u32)__builtin_amdgcn_readfirstlane((int)nb.lo); wb.hi = (u32)__builtin_amdgcn_readfirstlane((int)nb.hi); wb.n = (u32)__builtin_amdgcn_readfirstlane((int)nb.n);
                tau += G;
            } while (fast(tau));
            w.from_block(tau, lane);
            w.sa = wa; w.sb = wb; w.used = 0;
        } else {
            w.slow_step(t, tau, lane);
            ++tau;
        }
    }

    int bv = w.bv, bk = w.bk;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const int ov = __shfl_xor(bv, o, 64), ok = __shfl_xor(bk, o, 64);
        if (ov > bv || (ov == bv && ok < bk)) { bv = ov; bk = ok; }
    }
    bv = __builtin_amdgcn_readfirstlane(bv);
    bk = __builtin_amdgcn_readfirstlane(bk);
    u32 status = S_ST_EMPTY;   // no end cell (:215)
    int score = 0, end_a = 0, end_b = 0;
    if (bk != S_KEY_NONE) {
        const int x = bk < t.Y ? t.X - 1 : t.iA + (bk - t.Y);
        const int pos = bk < t.Y ? t.A0 + x + bk : t.ea;
        if (pos >= t.alen) status = S_ST_OUT_OF_RANGE;   // the traceback's a.at(pos) throws
        else { status = S_ST_OK; score = bv; end_a = pos; end_b = dt.begin_b + x; }
    }
    if (lane == 0) {
        typedef u32 u32x4 __attribute__((ext_vector_type(4)));
        const u32x4 rec = {(u32)score, (u32)end_a, (u32)end_b, status | ((u32)C << 8)};
        *reinterpret_cast<u32x4*>(&results[dt.res_idx]) = rec;
    }
}

// The task loop.  With score_task inlined and nothing between the two `if (lane == 0)` -- the record store that ends a task and the
// cursor fetch that begins the next -- the compiler (ROCm 7.2's clang 22, -O3) threaded lane 0 from the one into the other.  The gfx950
// code then took lane 0 out of EXEC after the first task and sent lanes 1 .. 63 back to the readfirstlane of `ti`, which for them is
// the 0 it was initialised with: they ran task 0 again, for ever (the kernel never ended on the device).  Two things now stand between
// the two statements, either of which is enough: score_task is a call, and every pass of the loop begins with a wave barrier, a
// convergent operation with side effects that no path may skip or duplicate.  What to look for in the assembly of k_score<C> after a
// compiler change: one loop, whose head restores EXEC to all lanes before v_readfirstlane_b32 of the fetched index.
// (register budget: five wavefronts per SIMD up to 5 columns per lane, four beyond)
template <int C>
__global__ __launch_bounds__(64, C <= 5 ? 5 : 4) void k_score(const ScoreParams p)
{
    const int lane = threadIdx.x;
    for (;;) {
        __builtin_amdgcn_wave_barrier();
        u32 ti = 0;
        if (lane == 0) ti = atomicAdd(p.cursor, 1u);
        ti = __builtin_amdgcn_readfirstlane(ti);
        if (ti >= p.n_tasks) break;
        score_task<C>(p.tasks[ti], p.results, lane);
    }
}

}  // namespace

const KernelFamily& score_family()
{
    static const KernelFamily f = {
        {(const void*)k_score<2>, (const void*)k_score<3>, (const void*)k_score<5>, (const void*)k_score<9>, (const void*)k_score<17>},
        {"k_score<2>", "k_score<3>", "k_score<5>", "k_score<9>", "k_score<17>"},
        64};
    return f;
}

}  // namespace gamdp
