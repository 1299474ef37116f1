// k_chain_c: the main chain of a merge block on the device, built on carry_task (gamdp_carry_task.inc) instead of a fill and a walk.
// One wavefront takes one merge block through alignBlocks' serial chain (PctgBuilder.cc:1617-1708) and the orientation retry of
// findBestAlignment (:1420-1509), one call after the other, both attempts one after the other (what k_chain2 does in role 0,
// GAMDP_L1_NO_TWINS=1).  The next call of a chain needs one thing of this one: its last match (:1660-1667), and carry_task has it in
// the end cell's summary the moment the fill ends.  So there is no walker, no mailbox, no scratch slot, no LDS and no wait loop; the
// only traffic with anyone else is the hand-over to the host at the end.  Any band up to GAMDP_MAX_TUNED_BAND (the instantiations
// of k_carry: C = band_cols(band)); N is always handled (ChainWin::info bit 1 is 0: there is no choice of cell to report).
//
// Everything but the DP is wave-uniform integer arithmetic that restates gamdp_l1.cpp's Machine for the MAIN phase, written here
// anew: this file shares the structures of gamdp_dev.h (DevMB, DevBlk, ChainOut, ChainWin, ChainParams, preflight_hd) with k_chain2
// and no code with gamdp_kernel.hip or kernel_*.inc.  The records (a DevResult and a ChainWin per call, in call order, at the indices
// k_chain2 uses) go to the host's replay (replay_chain), which derives every call once more and compares: a second implementation of
// the device chain, checked the same way as the first.  The scratch and slot fields of ChainParams / DevMB, the twins (n_twins,
// sync), max_rows, n_margin and n_by_contig are not read.  State 3 ("did not fit the slots") cannot occur.
#include <hip/hip_runtime.h>

#include "gamdp_dev.h"

namespace gamdp {
namespace {

#include "gamdp_score_common.inc"
#include "gamdp_carry_task.inc"

// timing diagnostics (ChainOut's t_* / hw fields): the diagnostics build only, 0 in the product
#ifdef GAMDP_DIAG
__device__ __forceinline__ u32 diag_clock() { return (u32)wall_clock64(); }
__device__ __forceinline__ u32 diag_hw_id() { return ((u32)__builtin_amdgcn_s_getreg((3 << 11) | 20) << 16) | ((u32)__builtin_amdgcn_s_getreg((15 << 11) | 4) & 0xffffu); }   // XCC_ID | HW_ID
#else
__device__ __forceinline__ constexpr u32 diag_clock() { return 0u; }
__device__ __forceinline__ constexpr u32 diag_hw_id() { return 0u; }
#endif

// a value all lanes hold, into scalar registers
__device__ __forceinline__ int cu(const int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ u32 cu(const u32 v) { return (u32)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ u64 cu(const u64 v)
{
    return ((u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)(v >> 32)) << 32) | (u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)v);
}
template <class T>
__device__ __forceinline__ const T* cu(const T* p) { return reinterpret_cast<const T*>(cu((u64)reinterpret_cast<uintptr_t>(p))); }

constexpr u32 CC_ST_INVALID = 3;   // GAMDP_ST_INVALID
constexpr u64 CC_MIN_HOMOLOGY = 95;   // MIN_HOMOLOGY, PctgBuilder.cc:1711-1724

__device__ __forceinline__ ChainOut chain_out(const u32 n_dp, const u32 state, const u32 t_begin, const u32 hw)
{
    ChainOut o;
    o.n_dp = n_dp; o.state = state; o.t_begin = t_begin; o.t_end = diag_clock(); o.hw = hw; o.hw_twin = 0;
    o.t_end_att[0] = 0; o.t_end_att[1] = 0; o.t_begin2 = 0; o.pad = 0;
    return o;
}

// The loops below end in stores of lane 0 (a call's records) and begin with reads all lanes share: every pass begins with a wave
// barrier, for the reason the comment above k_carry gives (without it the compiler threaded lane 0 from the store into the next
// pass's head and left the other lanes behind).  Register budget and occupancy as k_carry's: the chain's own state is scalar.
template <int C>
__global__ __launch_bounds__(64, C <= 3 ? 5 : C == 5 ? 4 : C == 9 ? 2 : 1) void k_chain_c(const ChainParams cp)
{
    const int lane = threadIdx.x;
    const u32 mi = cp.first_mb + blockIdx.x;
    const u32 t_begin = diag_clock(), hw_me = diag_hw_id();
    const DevMB* const mb = cu(cp.mbs + mi);
    const u64 mlen = cu(mb->mlen), slen = cu(mb->slen);
    const u64 m_start = cu(mb->m_start), s_start = cu(mb->s_start), s_end = cu(mb->s_end);
    const u64 align_thr = cu(mb->align_thr);
    const u32 first_blk = cu(mb->first_blk), n = cu(mb->n_blocks), audit_first = cu(mb->audit_first);
    const u32 *const a2 = cu(mb->a2), *const an = cu(mb->an);
    const u32 *const b2f = cu(mb->b2), *const bnf = cu(mb->bn), *const b2r = cu(mb->b2rc), *const bnr = cu(mb->bnrc);
    const u32 band = cp.band;
    bool try_rev = cu(mb->try_rev) != 0;
    u32 n_dp = 0, state = 1;
    for (int attempt = 0;;) {
        __builtin_amdgcn_wave_barrier();
        int64_t cur_ms = (int64_t)m_start;
        int64_t cur_ss = (int64_t)(try_rev ? slen - s_end - 1 : s_start);   // reverse_complement maps (start,end) -> (|s|-end-1, |s|-start-1), :1446-1448
        u64 last_a = 0, last_b = 0, sumlen = 0;
        bool bad = false, thrown = false;
        for (u32 k = 0; k < n; ++k) {
            __builtin_amdgcn_wave_barrier();
            const DevBlk* const bk = cu(cp.blks + first_blk + k);
            const int32_t cm_b = cu(bk->m_begin), cm_e = cu(bk->m_end), cs_b = cu(bk->s_begin), cs_e = cu(bk->s_end);
            const int32_t ml = cm_e < cm_b ? 0 : cm_e - cm_b + 1, sl = cs_e < cs_b ? 0 : cs_e - cs_b + 1;   // Frame.cc:124-127
            if (k > 0) {   // :1660-1667: from the last match of the call before, plus the gaps between the blocks (signed, clamped at 0)
                const int32_t pm_b = cu(bk[-1].m_begin), pm_e = cu(bk[-1].m_end), ps_b = cu(bk[-1].s_begin), ps_e = cu(bk[-1].s_end);
                const int32_t mgap = pm_b <= cm_b ? (cm_b - pm_e - 1) : (pm_b - cm_e - 1);
                const int32_t sgap = ps_b <= cs_b ? (cs_b - ps_e - 1) : (ps_b - cs_e - 1);
                cur_ms = (int64_t)(last_a + (u64)(int64_t)mgap); if (cur_ms < 0) cur_ms = 0;
                cur_ss = (int64_t)(last_b + (u64)(int64_t)sgap); if (cur_ss < 0) cur_ss = 0;
            }
#ifdef GAMDP_DIAG
            if (attempt == 0 && k == cp.skew_call) ++cur_ss;   // fault injection (GAMDP_DIAG_CHAIN_SKEW): the host's replay must notice
#endif
            const u64 begin_a = (u64)cur_ms, end_a = (u64)(cur_ms + ml - 1), begin_b = (u64)cur_ss, end_b = (u64)(cur_ss + sl - 1);
            u64 X = 0, cells = 0;
            const int st = preflight_hd(mlen, slen, band, begin_a, end_a, begin_b, end_b, false, false, &X, &cells);
            ChainWin w;
            w.begin_a = begin_a; w.end_a = end_a; w.begin_b = begin_b; w.end_b = end_b; w.X = (u32)X;
            w.info = (try_rev ? 1u : 0u) | ((u32)st << 8);
            DevResult r;
            r.begin_a = r.begin_b = r.score = 0; r.n_match = r.length = 0;
            r.first_a = r.first_b = r.last_a = r.last_b = 0;
            r.flags = (u32)st << 8;   // settled by the pre-checks: a zero record with their status, exactly as the host settles it (Ctx::align)
            if (st == 0) {
                DevTask dt;
                dt.a2 = a2; dt.an = an;
                dt.b2 = try_rev ? b2r : b2f; dt.bn = try_rev ? bnr : bnf;
                dt.a_base = 0; dt.b_base = 0;
                dt.end_a = (int64_t)(end_a < (1ull << 40) ? end_a : (1ull << 40));
                dt.alen = (int32_t)mlen; dt.blen = (int32_t)slen;
                dt.begin_a = (int32_t)begin_a; dt.begin_b = (int32_t)begin_b;
                dt.X = (int32_t)X; dt.band = (int32_t)band;
                dt.flags = 0; dt.res_idx = 0; dt.ops_off = 0; dt.ops_cap = 0;
                r = carry_task<C>(dt, lane);
                r.flags &= (1u << CARRY_COLS_SHIFT) - 1u;   // found | status << 8 and nothing above: the replay reads flags >> 8 as the status
            }
            if (lane == 0) { cp.win[audit_first + n_dp] = w; cp.audit[audit_first + n_dp] = r; }
            ++n_dp;
            const u32 status = cu(r.flags) >> 8;
            const u64 len = cu(r.length), nm = cu(r.n_match);
            // the last match: (0, 0) for an empty alignment (MyAlignment()) and for a call the pre-checks settled
            last_a = status == S_ST_OK ? (u64)(int64_t)cu(r.last_a) : 0;
            last_b = status == S_ST_OK ? (u64)(int64_t)cu(r.last_b) : 0;
            bad = bad || len == 0 || nm * 100 < CC_MIN_HOMOLOGY * len;   // is_good(vector), :1711-1724 (a record without an alignment has length 0)
            sumlen += len;
            if (status == S_ST_OUT_OF_RANGE || status == CC_ST_INVALID) { thrown = true; break; }   // the reference throws / undefined: the machine stops (finish_bad)
        }
        if (thrown) { state = 2; break; }
        if (!bad && sumlen >= align_thr) { state = try_rev ? 0x100u : 0u; break; }
        if (++attempt == 2) { state = 1; break; }   // :1512
        try_rev = !try_rev;
    }
    if (lane == 0) cp.out[mi] = chain_out(n_dp, state, t_begin, hw_me);
    // hand the chain to the host: records, windows and ChainOut into its pinned mirror, then the flag.  (The records are lane 0's
    // stores, the copy reads them in all lanes: out to the device's memory first, then nothing stale in this CU's cache.)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    {
        const u32* src = reinterpret_cast<const u32*>(cp.audit + audit_first);
        u32* dst = reinterpret_cast<u32*>(cp.host_audit + audit_first);
        const u32 nw = n_dp * (u32)(sizeof(DevResult) / sizeof(u32));
        for (u32 w = (u32)lane; w < nw; w += 64) dst[w] = src[w];
        const u32* wsrc = reinterpret_cast<const u32*>(cp.win + audit_first);
        u32* wdst = reinterpret_cast<u32*>(cp.host_win + audit_first);
        const u32 nww = n_dp * (u32)(sizeof(ChainWin) / sizeof(u32));
        for (u32 w = (u32)lane; w < nww; w += 64) wdst[w] = wsrc[w];
        if (lane == 0) cp.host_out[mi] = chain_out(n_dp, state, t_begin, hw_me);
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");   // system scope: every lane's stores above are out before the flag
    if (lane == 0) __hip_atomic_store(cp.host_done + mi, cp.epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace

const KernelFamily& chain_carry_family()
{
    static const KernelFamily f = {
        {(const void*)k_chain_c<2>, (const void*)k_chain_c<3>, (const void*)k_chain_c<5>, (const void*)k_chain_c<9>, (const void*)k_chain_c<17>},
        {"k_chain_c<2>", "k_chain_c<3>", "k_chain_c<5>", "k_chain_c<9>", "k_chain_c<17>"},
        64};
    return f;
}

}  // namespace gamdp
