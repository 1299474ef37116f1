// What k_score (gamdp_score.hip) and k_carry (gamdp_carry.hip) share: the constants of the reference, the sequence windows, the
// scoring-matrix rows, the lane shifts and what a wavefront knows of its task.  Included inside namespace gamdp { namespace {
// of either file; nothing of the alignment kernels (gamdp_kernel.hip, kernel_*.inc, gamdp_wide.hip) is used here or there.
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
// ... at an index all lanes share: the three words in scalar registers, so that what is taken from them is scalar work
__device__ __forceinline__ SWin load_win_uniform(splane p2, splane pn, const int64_t idx)
{
    SWin r = load_win(p2, pn, idx);
    r.lo = (u32)__builtin_amdgcn_readfirstlane((int)r.lo);
    r.hi = (u32)__builtin_amdgcn_readfirstlane((int)r.hi);
    r.n = (u32)__builtin_amdgcn_readfirstlane((int)r.n);
    return r;
}
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
