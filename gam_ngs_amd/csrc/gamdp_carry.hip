// k_carry: the whole result of BandedSmithWaterman(band).find_alignment from a fill alone (gamdp_carry_batch, include/gamdp.h).
// The reference's traceback (banded_smith_waterman.cc:227-311) is a pointer chase whose step from a cell (x, y) depends on that
// cell's value and on its three neighbours' values only (:229-308) -- what the fill holds when it computes the cell.  So every cell
// carries the summary of the traceback that would start in it, made from the summary of the cell that step leads to: where the
// traceback ends (:321), its number of ops, its number of MATCH ops and its first and last MATCH (my_alignment.cc:167-193, :228-262).
// The summary of the end cell (:173-215) is the result.  No directions, no rows of the matrix, no scratch arena, no walk.  The
// wavefront's state, the task as the wavefront knows it, the candidacy of a cell in the end-cell search and the fast range are
// k_score's, stated once in gamdp_score_common.inc (which says what carry_task keeps its own text of, and why); nothing is shared
// with the alignment kernels (gamdp_kernel.hip, kernel_*.inc, gamdp_wide.hip), whose walks this kernel is there to check.
//
// Lane layout as in k_score: one task per wavefront, lane l owns band columns [C*l, C*l + C) and is at row i = tau - l at row-time
// tau.  A cell is (value, summary); both go through the two lane shifts of a row-time (left of column 0: the lane below's last column
// of row-time tau-1; up of the last column: the lane above's column 0 of this row-time).  The end-cell search keeps the winning
// candidate's summary beside its (value, scan key); after the wave reduction the winner's summary is read from its lane.
//
// The summary, five int32 per cell (x < 500 000 < 2^19 rows, y + 1 <= 1088 < 2^11 columns):
//   B    where the traceback ends: (x_p + 1) * 2048 + (y_p + 1) of the first cell (x_p, y_p) outside (x < 0, y < 0 or pos < 0), so that
//        begin_a = pos_p + 1 = A0 + (x_p + 1) + y_p and begin_b = begin_b + x_p + 1 (:321)
//   ln   ops,  nm  MATCH ops
//   F    x * 2048 + y of the MATCH nearest the begin (valid when nm > 0),  Lc  of the MATCH nearest the end cell
// A slow path, cell by cell by the reference's rules, for the special row-times (first rows, pos <= 0, pos >= |a|, the last row, the
// anti-diagonal pos == end_a), and a fast path for all others: there every cell is the plain three-way maximum, and k_score's
// block form (value + 16 i + 8 j) keeps the three candidates' equalities, so "diag if new == D, else up if new == U, else left" is
// the whole step rule (fast_step).
#include <hip/hip_runtime.h>

#include "gamdp_dev.h"

namespace gamdp {
namespace {

#include "gamdp_score_common.inc"
#include "gamdp_carry_task.inc"   // Sum, CWave<C>, carry_task<C>: shared with k_chain_c (gamdp_chain_carry.hip)

// The task loop.  k_score (gamdp_score.hip) documents what went wrong there with the task inlined and nothing between the record
// store that ends a task and the cursor fetch that begins the next (both `if (lane == 0)`): the compiler threaded lane 0 from the one
// into the other and the other lanes ran task 0 for ever.  Of the two things it names that each prevent it, this kernel has the
// second only: every pass of the loop begins with a wave barrier, a convergent operation with side effects that no path may skip or
// duplicate.  The first, the task as a call, is not taken: the callee's saved registers would be private memory (188 to 704 bytes per
// lane when it was tried), which this kernel must not have.  What to look for in the assembly of k_carry<C> after a compiler change:
// one loop over tasks, whose head restores EXEC to all lanes before v_readfirstlane_b32 of the fetched index, and no scratch_ access.
// (register budget: a cell is six registers, a column eight, and the slow path's unrolled cells want many more at a time: five
// wavefronts per SIMD up to 3 columns per lane, four at 5, two at 9, one at 17, which is what compiles without a spill)
template <int C>
__global__ __launch_bounds__(64, C <= 3 ? 5 : C == 5 ? 4 : C == 9 ? 2 : 1) void k_carry(const CarryParams p)
{
    const int lane = threadIdx.x;
    for (;;) {
        __builtin_amdgcn_wave_barrier();
        u32 ti = 0;
        if (lane == 0) ti = atomicAdd(p.cursor, 1u);
        ti = __builtin_amdgcn_readfirstlane(ti);
        if (ti >= p.n_tasks) break;
        const DevTask& dt = p.tasks[ti];
        const DevResult res = carry_task<C>(dt, lane);
        if (lane == 0) p.results[dt.res_idx] = res;
    }
}

}  // namespace

const KernelFamily& carry_family()
{
    static const KernelFamily f = {
        {(const void*)k_carry<2>, (const void*)k_carry<3>, (const void*)k_carry<5>, (const void*)k_carry<9>, (const void*)k_carry<17>},
        {"k_carry<2>", "k_carry<3>", "k_carry<5>", "k_carry<9>", "k_carry<17>"},
        64};
    return f;
}

}  // namespace gamdp
