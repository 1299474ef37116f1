// k_ops_fp: gamdp_ops_fingerprint (include/gamdp.h) of edit strings that lie in device memory -- the strings gamdp_align_batch's
// walks wrote (gamdp_align_batch_fp: they never leave the device), or strings a caller uploaded (gamdp_ops_fingerprint_batch).
//
// F(s . e) = F(s) * M + e + 1 (mod 2^32) unrolls to F = sum_t (s[t] + 1) * M^(len - 1 - t), a sum whose terms commute.  The walks
// leave a string in traceback order, r[k] = s[len - 1 - k], so in memory order F = sum_k (r[k] + 1) * M^k: no reversal.  A string
// is cut into segments of OPS_FP_SEG_BYTES; a wavefront takes a segment, every lane OPS_FP_LANE_BYTES contiguous bytes of it:
//   lane:     h = sum_q v_q * M^q over its 64 bytes, four at a time (Horner in M^4 over the 16 words, the "+ 1" of four bytes as one
//             constant); v_q = byte + 1 inside the string and 0 outside, which a lane that holds the string's end computes byte by byte;
//   wave:     sum_l h_l * M^(64 l) (a 64-entry table), added up over the wavefront;
//   segment:  times M^(4096 s) by square-and-multiply on s; a wavefront takes a run of consecutive segments, adds up the shares of one
//             task's and adds them into fp[idx] with one atomicAdd (zeroed by the host before the launch).
// k_ops_fp<true> takes strings in forward order (descending exponents): the same segments, lanes and table, the string placed so
// that it ENDS where a lane ends (OpsFpTask: `lead` bytes in front of it count nothing), so that a lane's share is again a plain
// Horner sum and the lanes of a segment of m bytes take M^(m - 64 (l + 1)) from the table.
// Which task a run's first segment belongs to: a binary search in the launch's prefix array of segment counts, walked along from
// there (a search per segment was a chain of a dozen dependent loads in front of 4 KiB of work).  Plain C++: vector loads, a vector
// atomic.
#include <hip/hip_runtime.h>

#include "gamdp.h"
#include "gamdp_dev.h"

namespace gamdp {
namespace {

constexpr u32 M1 = GAMDP_OPS_FP_MULT;
constexpr u32 cpow(u32 b, u64 e)
{
    u32 r = 1;
    for (; e; e >>= 1, b *= b) if (e & 1) r *= b;
    return r;
}
constexpr u32 M2 = M1 * M1, M3 = M2 * M1, M4 = M2 * M2, K4 = 1u + M1 + M2 + M3;
constexpr u32 M_LANE = cpow(M1, OPS_FP_LANE_BYTES), M_SEG = cpow(M1, OPS_FP_SEG_BYTES);
constexpr int LANE_WORDS = OPS_FP_LANE_BYTES / 4;
static_assert(OPS_FP_SEG_BYTES == 64 * OPS_FP_LANE_BYTES && OPS_FP_LANE_BYTES == 64, "a segment is one wavefront of lanes, a lane four 16-byte loads");

struct LanePow { u32 v[64]; };   // M^(64 l)
constexpr LanePow lane_pow_table()
{
    LanePow t{};
    u32 x = 1;
    for (int l = 0; l < 64; l++) { t.v[l] = x; x *= M_LANE; }
    return t;
}
__constant__ LanePow lane_pow = lane_pow_table();

__device__ inline u32 mpow(u32 b, u32 e)   // b^e mod 2^32 (wave-uniform arguments)
{
    u32 r = 1;
    for (; e; e >>= 1, b *= b) if (e & 1) r *= b;
    return r;
}

// A lane's share: v_q = byte q + 1 for lo <= q < hi, 0 otherwise;  sum_q v_q M^q, or (FORWARD) sum_q v_q M^(63 - q)
template <bool FORWARD>
__device__ inline u32 lane_poly(const u32 (&w)[LANE_WORDS], const int lo, const int hi)
{
    u32 h = 0;
    if (lo == 0 && hi == (int)OPS_FP_LANE_BYTES) {
#pragma unroll
        for (int k = 0; k < LANE_WORDS; k++) {
            const u32 x = w[FORWARD ? k : LANE_WORDS - 1 - k];
            const u32 b0 = x & 255u, b1 = (x >> 8) & 255u, b2 = (x >> 16) & 255u, b3 = x >> 24;
            const u32 part = FORWARD ? b0 * M3 + b1 * M2 + b2 * M1 + b3 : b0 + b1 * M1 + b2 * M2 + b3 * M3;
            h = h * M4 + part + K4;
        }
    } else {
#pragma unroll
        for (int k = 0; k < (int)OPS_FP_LANE_BYTES; k++) {
            const int q = FORWARD ? k : (int)OPS_FP_LANE_BYTES - 1 - k;
            const u32 b = (w[q >> 2] >> ((q & 3) * 8)) & 255u;
            h = h * M1 + ((q >= lo && q < hi) ? b + 1u : 0u);
        }
    }
    return h;
}

template <bool FORWARD>
__global__ __launch_bounds__(OPS_FP_THREADS) void k_ops_fp(const OpsFpParams p)
{
    const u32 lane = threadIdx.x & 63u;
    const u32 wave = __builtin_amdgcn_readfirstlane((blockIdx.x * OPS_FP_THREADS + threadIdx.x) >> 6);
    const u32 n_waves = gridDim.x * (OPS_FP_THREADS / 64);
    // a wavefront takes a run of consecutive segments: one search for the task of the first, then the prefix array is walked along,
    // and the shares of one task's segments are added up before they go to fp (one atomicAdd per task of the run)
    const u32 per = (p.n_segs + n_waves - 1) / n_waves;
    u32 seg = wave * per;
    const u32 seg_end = min(seg + per, p.n_segs);
    if (seg >= seg_end) return;
    // the task of the first segment: the last one whose first segment is not beyond it (seg_first[0] = 0, seg_first[n_tasks] = n_segs)
    u32 ti = 0;
    for (u32 t_hi = p.n_tasks; t_hi - ti > 1;) {
        const u32 mid = (ti + t_hi) >> 1;
        if (p.seg_first[mid] <= seg) ti = mid; else t_hi = mid;
    }
    u32 first = p.seg_first[ti], next = p.seg_first[ti + 1];
    while (seg < seg_end) {
        while (seg >= next) { ti++; first = next; next = p.seg_first[ti + 1]; }   // (ti + 1 <= n_tasks while seg < n_segs)
        const OpsFpTask t = p.tasks[ti];
        u32 len = t.len;
        if (!FORWARD) {   // what the walk left: its length and status, read where it wrote them
            const DevResult r = p.results[t.idx];
            len = (r.flags >> 8) == 0u ? min(r.length, t.len) : 0u;   // GAMDP_ST_OK = 0; never beyond the task's room
        }
        u32 acc = 0;
        const u32 run_end = min(next, seg_end);   // this task's segments of the run
        for (; seg < run_end; seg++) {
            const u32 s = seg - first;
            const u32 seg_at = s * OPS_FP_SEG_BYTES;
            if (seg_at >= len) continue;   // (wave-uniform)
            const u32 m = min(len - seg_at, OPS_FP_SEG_BYTES);   // bytes of the string's room in this segment
            const u32 at = seg_at + lane * OPS_FP_LANE_BYTES;
            u32 w[LANE_WORDS];
#pragma unroll
            for (int k = 0; k < LANE_WORDS; k++) w[k] = 0;
            const uint4* const src = reinterpret_cast<const uint4*>(p.ops + t.off + at);
#pragma unroll
            for (int g = 0; g < 4; g++) {
                if (at + 16u * g < len) {   // the room ends on a multiple of 16 at or after len: a load that starts inside it stays inside
                    const uint4 x = src[g];
                    w[4 * g] = x.x; w[4 * g + 1] = x.y; w[4 * g + 2] = x.z; w[4 * g + 3] = x.w;
                }
            }
            const int hi = at >= len ? 0 : (int)min(len - at, OPS_FP_LANE_BYTES);
            const int lo = FORWARD ? (t.lead <= at ? 0 : (int)min(t.lead - at, OPS_FP_LANE_BYTES)) : 0;
            u32 f = 0;
            if (lo < hi) {
                const u32 lanes = m / OPS_FP_LANE_BYTES;   // FORWARD: m is a multiple of the lane's bytes, and this lane is one of `lanes`
                f = lane_poly<FORWARD>(w, lo, hi) * lane_pow.v[FORWARD ? (lanes - 1u - lane) & 63u : lane];
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) f += __shfl_xor(f, o);
            acc += f * (FORWARD ? mpow(M_LANE, (len - seg_at - m) / OPS_FP_LANE_BYTES) : mpow(M_SEG, s));
        }
        if (lane == 0 && acc != 0) atomicAdd(p.fp + t.idx, acc);   // (adding 0 changes nothing)
    }
}

}  // namespace

const void* ops_fp_kernel(const bool forward) { return forward ? (const void*)k_ops_fp<true> : (const void*)k_ops_fp<false>; }
const char* ops_fp_kernel_name(const bool forward) { return forward ? "k_ops_fp<true>" : "k_ops_fp<false>"; }

}  // namespace gamdp
