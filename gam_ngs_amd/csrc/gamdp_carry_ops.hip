// k_carry_f: k_carry (gamdp_carry.hip, which has the argument) with one more field in a cell's summary, the fingerprint of the edit
// string the reference's traceback from that cell would return (gamdp_carry_ops_batch, gamdp_ops_fingerprint: include/gamdp.h).
// The forward edit string of a cell is the forward edit string of the cell its step leads to plus that step's op, and the
// fingerprint is computed left to right, F(s . e) = F(s) * M + e + 1: so it is updated where ln, nm, F and Lc are (step_on), starts
// from 0 where the traceback ends, travels through both lane shifts and the end-cell search with the rest of the summary, and the
// end cell's is that of the whole string.  No directions, no walk, no scratch, and still no private memory.
//
// What it is for: gamdp_align_batch's edit strings come from the walks' want_ops path, which reads every direction on the path --
// every re-created strip, side capture and tagged block.  Two strings can agree in every field k_carry checks and still differ (a
// GAP_A / GAP_B pair in the other order); the fingerprint of the bytes gamdp_align_batch returned against this kernel's checks
// every op (tools/score_crosscheck.py --ops).
//
// A translation unit of its own: k_carry<C> and k_chain_c<C> instantiate carry_task<C, false>, in which the sixth field does not
// exist, and compile to what they were.
#include <hip/hip_runtime.h>

#include "gamdp_dev.h"

namespace gamdp {
namespace {

#include "gamdp_score_common.inc"
#include "gamdp_carry_task.inc"

// The task loop is k_carry's, wave barrier at its head for the reason given there.  Register budget: a cell is seven registers, a
// column nine; five wavefronts per SIMD at 2 columns per lane, four at 3, three at 5, two at 9, one at 17 is what compiles without
// a spill.
template <int C>
__global__ __launch_bounds__(64, C == 2 ? 5 : C == 3 ? 4 : C == 5 ? 3 : C == 9 ? 2 : 1) void k_carry_f(const CarryOpsParams p)
{
    const int lane = threadIdx.x;
    for (;;) {
        __builtin_amdgcn_wave_barrier();
        u32 ti = 0;
        if (lane == 0) ti = atomicAdd(p.cursor, 1u);
        ti = __builtin_amdgcn_readfirstlane(ti);
        if (ti >= p.n_tasks) break;
        const DevTask& dt = p.tasks[ti];
        u32 fp;
        const DevResult res = carry_task<C, true>(dt, lane, &fp);
        if (lane == 0) { p.results[dt.res_idx] = res; p.ops_fp[dt.res_idx] = fp; }
    }
}

}  // namespace

const KernelFamily& carry_ops_family()
{
    static const KernelFamily f = {
        {(const void*)k_carry_f<2>, (const void*)k_carry_f<3>, (const void*)k_carry_f<5>, (const void*)k_carry_f<9>, (const void*)k_carry_f<17>},
        {"k_carry_f<2>", "k_carry_f<3>", "k_carry_f<5>", "k_carry_f<9>", "k_carry_f<17>"},
        64};
    return f;
}

}  // namespace gamdp
