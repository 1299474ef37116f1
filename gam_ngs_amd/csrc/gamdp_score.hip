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

#include "gamdp_score_common.inc"   // shared with k_carry / k_chain_c: windows, scoring rows, WaveBase, slow_value, the end-cell search, FastRange

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

// the wavefront's state (WaveBase, gamdp_score_common.inc) and the two kinds of row-time
template <int C>
struct SWave : WaveBase<C, S_DEAD> {
    using B = WaveBase<C, S_DEAD>;
    using B::h; using B::a5; using B::dead; using B::leftadd; using B::row;

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
        this->take_row(wb, K);
        const int L = from_lane_below(h[C - 1]);
        h[0] = max3i(h[0] + cell_score16(row, a5[K % C]) + dead[0], h[1], L + leftadd);
        const int U = from_lane_above(h[0]);   // (lane 63 gets 0, for a column that is always dead: 2*band+1 is odd, 64*C even)
#pragma unroll
        for (int c = 1; c < C - 1; ++c) h[c] = max3i(h[c] + cell_score16(row, a5[(c + K) % C]) + dead[c], h[c + 1], h[c - 1]);
        h[C - 1] = max3i(h[C - 1] + cell_score16(row, a5[(C - 1 + K) % C]) + dead[C - 1], U, h[C - 2]);
        a5[K % C] = shift_in_from_above(a_field(win_code(wa, K), win_isn(wa, K)), a5[(1 + K) % C]);
    }
    template <int K>
    __device__ __forceinline__ void fast_block(const SWin& wa, const SWin& wb)
    {
        if constexpr (K < S_BLOCK<C>) {
            fast_step<K>(wa, wb);
            fast_block<K + 1>(wa, wb);
        }
    }

    // One row-time by the reference's rules, cell by cell (slow_value).  Lanes that are not at a row of the matrix compute along
    // (nothing reads what they make: see the header) and offer no candidates.  No branch depends on the lane except around the
    // candidates: the lane shifts need every lane.
    __device__ __forceinline__ void slow_step(const STask& t, const int tau, const int lane)
    {
        this->slow_take_row(t, tau);
        const int i = tau - lane;
        const int p0 = t.A0 + tau + (C - 1) * lane, j0 = C * lane;
        const int L = from_lane_below(h[C - 1]);   // (lane 0: unused, its column 0 has no left neighbour)
        int U = 0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int leftv = c > 0 ? h[c > 0 ? c - 1 : 0] : L;
            const int upv = c < C - 1 ? h[c < C - 1 ? c + 1 : 0] : U;
            h[c] = slow_value(t, i, j0 + c, p0 + c, cell_score16(row, a5[c]) - 16, h[c], leftv, upv);
            if (c == 0) U = from_lane_above(h[0]);
        }
        this->search_end_cell(t, i, p0, j0, [](int) {});
        this->slow_advance();
    }
};

// Out of line, like the phases of the alignment kernels (registers of the task allocated apart from the task loop's).  It also keeps
// the task's last statement (lane 0 stores the record) away from the loop's first (lane 0 takes the next task): see k_score.
template <int C>
__device__ __noinline__ void score_task(const DevTask& dt, ScoreRec* results, const int lane)
{
    const STask t = stask_of(dt);
    SWave<C> w;
    w.seed(t, dt, lane);
    // The task's row-times: runs of fast blocks (the bases of a block are fetched while the block before it is computed) where
    // FastRange allows them, slow_step for all others.  Written out here and not shared: see gamdp_score_common.inc.
    constexpr int G = S_BLOCK<C>;
    const int LE = (t.Y - 1) / C;
    const FastRange fast(t, C, G, LE);
    const int T = t.X + LE;   // lane LE is at the last row at row-time X - 1 + LE
    for (int tau = 0; tau < T;) {
        if (fast(tau)) {
            SWin wa = load_win_uniform(t.a2, t.an, w.aidx + tau), wb = load_win_uniform(t.b2, t.bn, w.bidx + tau);
            w.to_block(tau, lane);
            do {
                const SWin na = load_win(t.a2, t.an, w.aidx + tau + G), nb = load_win(t.b2, t.bn, w.bidx + tau + G);   // (all lanes the same words)
                w.template fast_block<0>(wa, wb);
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

    int bv = w.bv, bk = w.bk;
    best_of_wave(bv, bk);
    const SEnd e = end_of_key(t, bk);
    const bool ok = e.status == S_ST_OK;
    if (lane == 0) {
        typedef u32 u32x4 __attribute__((ext_vector_type(4)));
        const u32x4 rec = {(u32)(ok ? bv : 0), (u32)(ok ? e.pos : 0), (u32)(ok ? dt.begin_b + e.x : 0), e.status | ((u32)C << 8)};
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
