// Micro-benchmark 7: the diag candidate of the packed cell as an INTEGER add on f16 bit patterns.
//
// The bit patterns of the non-negative finite f16 numbers, 0x0000 ... 0x7BFF, are ordered exactly like the unsigned integers
// they are, and -inf (0xFC00) orders below all of them.  A half-word that holds OFFSET + value as a plain integer is then a
// valid operand of v_pk_maximum3_f16 -- which hands back one of its operands bit for bit while they are normal numbers
// (patterns >= 0x0400) -- and "+12 / +21 on both tasks" is one v_add_u32 with (sB << 16) | sA: nothing is rounded.
// Two questions, answered in one process:
//   1. self-check: over patterns spread across 0x0400 ... 0x7BFF plus 0xFC00 (every triple of 128 of them, and every PAIR of
//      all 30 721 with 0xFC00 as the third operand), does the device's v_pk_maximum3_f16 return, per half, bit for bit the
//      operand that is the largest 16-bit integer (0xFC00 counting as the smallest)?  Exit status 1 if not.
//   2. rate: the bare software-pipelined cell stream of kernel_pair.inc (as in valu_rate6.hip, V = 2) at 1, 2 and 4
//      wavefronts per SIMD,
//        V = 0  as today:     v_perm_b32 -> v_pk_fma_f16 -> v_pk_maximum3_f16   (values as f16 numbers)
//        V = 1  as proposed:  v_perm_b32 -> v_add_u32    -> v_pk_maximum3_f16   (values as patterns OFFSET + value)
//      on the SAME pseudo-random sequences, REPS launches each, alternating.  Both streams compute the same recurrence, so
//      their decoded results must agree word for word (exit status 1 if not).  The state is put back at every block (19
//      moves per 816 instructions, the same in both streams) so that the values stay inside the exact range of f16.
//      "faster" = the proposed stream's median lies below today's by more than today's own min-max spread.
// Build: hipcc --offload-arch=gfx950 -O3 tools/valu_rate7.hip -o tools/valu_rate7 ; run on the GPU box.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef unsigned u32;
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef unsigned short us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ h2 as_h2(u32 x) { return __builtin_bit_cast(h2, x); }
__device__ __forceinline__ u32 as_u(h2 x) { return __builtin_bit_cast(u32, x); }
__device__ __forceinline__ u32 max3(u32 a, u32 b, u32 c)
{
    return as_u(__builtin_elementwise_maximum(__builtin_elementwise_maximum(as_h2(a), as_h2(b)), as_h2(c)));
}
#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)

constexpr int C = 17, ROWS = 16;
constexpr int TN = 256;   // (small tables: 3 KB of LDS per wavefront)
constexpr u32 OFFSET = 0x2000u;
constexpr u32 NINF2 = 0xFC00FC00u;

// ---- 1. the self-check ---------------------------------------------------------------------------------------------------
__host__ __device__ inline int key_of(u32 p) { return p == 0xFC00u ? -1 : (int)p; }   // 0xFC00 below every pattern
__host__ __device__ inline u32 best_of(u32 a, u32 b, u32 c) { u32 m = a; if (key_of(b) > key_of(m)) m = b; if (key_of(c) > key_of(m)) m = c; return m; }

// every triple (i, j, k) of the n patterns in s[]: low halves (s[i], s[j], s[k]), high halves (s[k], s[i], s[j])
__global__ void k_check3(const u32* s, int n, u32* bad)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long)n * n * n) return;
    const u32 a = s[t % n], b = s[(t / n) % n], c = s[t / ((long)n * n)];
    const u32 got = max3(a | (c << 16), b | (a << 16), c | (b << 16));
    const u32 want = best_of(a, b, c) | (best_of(c, a, b) << 16);
    if (got != want) atomicAdd(bad, 1u);
}
// every pair of ALL patterns 0x0400 ... 0x7BFF and 0xFC00 (index 30 720), the third operand "no source", in all three positions
__global__ void k_check2(u32* bad)
{
    constexpr long N = 0x7C00 - 0x0400 + 1;
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N * N) return;
    const u32 ia = (u32)(t % N), ib = (u32)(t / N);
    const u32 a = ia == N - 1 ? 0xFC00u : 0x0400u + ia, b = ib == N - 1 ? 0xFC00u : 0x0400u + ib;
    const u32 want = best_of(a, b, 0xFC00u) * 0x00010001u;
    const u32 g0 = max3(a | (b << 16), b | (a << 16), NINF2);
    const u32 g1 = max3(a | (b << 16), NINF2, b | (a << 16));
    const u32 g2 = max3(NINF2, a | (b << 16), b | (a << 16));
    if (g0 != want || g1 != want || g2 != want) atomicAdd(bad, 1u);
}

// ---- 2. the two streams ---------------------------------------------------------------------------------------------------
__shared__ u32 s_tab[2][TN + 16];
__shared__ u32 s_w[TN + 16];

template <int V> __device__ __forceinline__ u32 enc(const int v)   // the same value in both halves
{
    if constexpr (V == 0) { const h2 x = {(_Float16)(float)v, (_Float16)(float)v}; return as_u(x); }
    else return (OFFSET + (u32)v) * 0x00010001u;
}
template <int V> __device__ __forceinline__ int dec_lo(const u32 w)
{
    if constexpr (V == 0) return (int)(float)as_h2(w).x;
    else return (int)(w & 0xFFFFu) - (int)OFFSET;
}
template <int V> __device__ __forceinline__ int dec_hi(const u32 w)
{
    if constexpr (V == 0) return (int)(float)as_h2(w).y;
    else return (int)(w >> 16) - (int)OFFSET;
}
// a hand-off's base difference: packed f16 add today, packed 16-bit integer add on patterns (no carry between the tasks)
template <int V> __device__ __forceinline__ u32 add_d(const u32 v, const u32 d)
{
    if constexpr (V == 0) return as_u(as_h2(v) + as_h2(d));
    else return __builtin_bit_cast(u32, __builtin_bit_cast(us2, v) + __builtin_bit_cast(us2, d));
}

// tabs: [0][TN + 16] task A's, [1][..] task B's look-up words; sel: [TN + 16] selectors (all in the form of stream V)
template <int V>
__global__ __launch_bounds__(64, 4) void k(u32* out, const u32* tabs, const u32* sel, int blocks16)
{
    const int lane = threadIdx.x;
    for (int i = lane; i < TN + 16; i += 64) { s_tab[0][i] = tabs[i]; s_tab[1][i] = tabs[TN + 16 + i]; s_w[i] = sel[i]; }
    __syncthreads();
    u32 Lp[C], Lp0[C], W[C + ROWS - 1];
#pragma unroll
    for (int c = 0; c < C; ++c) Lp0[c] = enc<V>(15 * c + lane % 5);
#pragma unroll
    for (int k2 = 0; k2 < C + ROWS - 1; ++k2) W[k2] = sel[(lane * 3 + k2) & (TN - 1)];
    const u32 Lin0 = enc<V>(-8);
    u32 Lin = Lin0, xk = NINF2;
    u32 dl = 0, dr = 0;
    asm volatile("" : "+v"(dl), "+v"(dr));   // (base differences: zero here, but not known to the compiler)
    [[maybe_unused]] const h2 three = {(_Float16)3.0f, (_Float16)3.0f};
    for (int b = 0; b < blocks16; ++b) {
        const u32* ta = &s_tab[0][(b * 16 + lane) & (TN - 1)];
        const u32* tb = &s_tab[1][(b * 16 + lane) & (TN - 1)];
        const u32* wa = &s_w[(b * 16 + 3 * lane) & (TN - 1)];
#pragma unroll
        for (int c = 0; c < C; ++c) Lp[c] = Lp0[c];
        Lin = Lin0; xk = NINF2;
        // flat cell index g = r * C + c; stage s of group g: max3(g), add(g + 1), perm(g + 2)
        u32 tA[ROWS], tB[ROWS];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) { W[C - 1 + r] = wa[r]; tA[r] = ta[r]; tB[r] = tb[r]; }
        u32 m[3];   // perm results in flight (cell g % 3)
        u32 D[2];   // diag candidates in flight
        u32 L = Lin, x = NINF2;
        auto do_perm = [&](const int g) __attribute__((always_inline)) {
            const int r = g / C, c = g % C;
            m[g % 3] = __builtin_amdgcn_perm(tB[r], tA[r], W[r + c]);
        };
        auto do_diag = [&](const int g) __attribute__((always_inline)) {
            const int c = g % C;
            if constexpr (V == 0) D[g % 2] = as_u(__builtin_elementwise_fma(as_h2(m[g % 3]), three, as_h2(Lp[c])));
            else D[g % 2] = m[g % 3] + Lp[c];
        };
        do_perm(0); do_perm(1); do_diag(0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int g = r * C + c;
            const u32 U = (c < C - 1) ? Lp[(c < C - 1) ? c + 1 : c] : x;
            if (c == 0) L = Lin;
            L = max3(D[g % 2], U, L);
            // diag(g+1) reads the OLD Lp[c+1] (as does the max3 above, as its `up` source); Lp[c] is written after
            if (g + 1 < ROWS * C) do_diag(g + 1);
            Lp[c] = L;
            if (g + 2 < ROWS * C) do_perm(g + 2);
            if (c == 2) {   // the hand-off of column 0, two groups after its max3 (DPP needs two wait states)
                xk = (u32)__builtin_amdgcn_update_dpp((int)xk, (int)Lp[0], 0x130, 0xf, 0xf, false);
            }
            if (c == 4) x = add_d<V>(xk, dr);
            __builtin_amdgcn_sched_barrier(0);
            if (c == C - 1) {
                Lin = (u32)__builtin_amdgcn_update_dpp((int)Lin, (int)L, 0x138, 0xf, 0xf, false);
                Lin = add_d<V>(Lin, dl);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        }
#pragma unroll
        for (int k2 = 0; k2 < C - 1; ++k2) W[k2] = W[k2 + ROWS];
    }
    int s = dec_lo<V>(Lin) - 3 * dec_hi<V>(Lin);
#pragma unroll
    for (int c = 0; c < C; ++c) s += (c + 1) * dec_lo<V>(Lp[c]) + (c + 20) * dec_hi<V>(Lp[c]);
    out[blockIdx.x * 64 + lane] = (u32)s;
}

struct Inputs { u32 *tabs, *sel; };

template <int V>
float run(u32* out, const Inputs& in, int waves_per_simd, int blocks16)
{
    const int grid = 256 * 4 * waves_per_simd;
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    CHECK(hipEventRecord(e0));
    k<V><<<grid, 64>>>(out, in.tabs, in.sel, blocks16);
    CHECK(hipEventRecord(e1));
    CHECK(hipDeviceSynchronize());
    float ms = 0;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    CHECK(hipEventDestroy(e0)); CHECK(hipEventDestroy(e1));
    return ms;
}

int main()
{
    constexpr int MAXW = 4, REPS = 7, BLOCKS16 = 6000;
    // --- self-check
    std::vector<u32> pat;
    for (u32 e = 0x0400u; e < 0x7C00u; e += 0x0400u) { pat.push_back(e); pat.push_back(e + 1); pat.push_back(e + 0x03FFu); }   // the edges of every binade
    u32 rng = 12345u;
    auto next = [&]() { rng = rng * 1664525u + 1013904223u; return rng >> 8; };
    while (pat.size() < 127) pat.push_back(0x0400u + next() % (0x7C00u - 0x0400u));
    pat.push_back(0xFC00u);
    const int n = (int)pat.size();
    u32 *d_pat, *d_bad;
    CHECK(hipMalloc(&d_pat, n * sizeof(u32))); CHECK(hipMalloc(&d_bad, 2 * sizeof(u32)));
    CHECK(hipMemcpy(d_pat, pat.data(), n * sizeof(u32), hipMemcpyHostToDevice));
    CHECK(hipMemset(d_bad, 0, 2 * sizeof(u32)));
    const long n3 = (long)n * n * n, n2 = 30721L * 30721L;
    k_check3<<<(unsigned)((n3 + 255) / 256), 256>>>(d_pat, n, d_bad);
    k_check2<<<(unsigned)((n2 + 255) / 256), 256>>>(d_bad + 1);
    CHECK(hipDeviceSynchronize());
    u32 bad[2];
    CHECK(hipMemcpy(bad, d_bad, sizeof bad, hipMemcpyDeviceToHost));
    printf("self-check: v_pk_maximum3_f16 on patterns: %ld triples of %d patterns, %u wrong; %ld pairs of all 30721 patterns x 3 positions, %u wrong\n",
           n3, n, bad[0], n2, bad[1]);
    bool ok = bad[0] == 0 && bad[1] == 0;

    // --- the two streams on the same pseudo-random sequences
    std::vector<u32> tabs[2], sel[2];
    for (int v = 0; v < 2; ++v) { tabs[v].resize(2 * (TN + 16)); sel[v].resize(TN + 16); }
    for (int i = 0; i < TN + 16; ++i) {
        const u32 bA = next() & 3u, bB = next() & 3u, cA = next() & 3u, cB = next() & 3u;
        tabs[0][i] = 0x44444444u + (0x03u << (bA * 8u));            tabs[0][TN + 16 + i] = 0x44444444u + (0x03u << (bB * 8u));   // high byte of 4.0 / 7.0
        tabs[1][i] = 0x0C0C0C0Cu + (0x09u << (bA * 8u));            tabs[1][TN + 16 + i] = 0x0C0C0C0Cu + (0x09u << (bB * 8u));   // 12 / 21
        sel[0][i] = 0x000C000Cu | (cA << 8) | ((4u + cB) << 24);    // look-up in the high byte of each half, zero below
        sel[1][i] = 0x0C000C00u | cA | ((4u + cB) << 16);           // look-up in the low byte of each half, zero above
    }
    Inputs in[2];
    for (int v = 0; v < 2; ++v) {
        CHECK(hipMalloc(&in[v].tabs, tabs[v].size() * sizeof(u32))); CHECK(hipMalloc(&in[v].sel, sel[v].size() * sizeof(u32)));
        CHECK(hipMemcpy(in[v].tabs, tabs[v].data(), tabs[v].size() * sizeof(u32), hipMemcpyHostToDevice));
        CHECK(hipMemcpy(in[v].sel, sel[v].data(), sel[v].size() * sizeof(u32), hipMemcpyHostToDevice));
    }
    const size_t nout = (size_t)256 * 4 * MAXW * 64;
    u32* out[2];
    for (int v = 0; v < 2; ++v) CHECK(hipMalloc(&out[v], nout * sizeof(u32)));
    std::vector<u32> h0(nout), h1(nout);
    for (int w = 1; w <= MAXW; w *= 2) {
        (void)run<0>(out[0], in[0], w, 10); (void)run<1>(out[1], in[1], w, 10);   // warm-up
        std::vector<float> t[2];
        for (int rep = 0; rep < REPS; ++rep) { t[0].push_back(run<0>(out[0], in[0], w, BLOCKS16)); t[1].push_back(run<1>(out[1], in[1], w, BLOCKS16)); }
        const size_t nw = (size_t)256 * 4 * w * 64;
        CHECK(hipMemcpy(h0.data(), out[0], nw * sizeof(u32), hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(h1.data(), out[1], nw * sizeof(u32), hipMemcpyDeviceToHost));
        size_t diff = 0;
        for (size_t i = 0; i < nw; ++i) diff += h0[i] != h1[i];
        if (diff) ok = false;
        const double cells = (double)nw * C * ROWS * BLOCKS16 * 2;
        float med[2], lo[2], hi[2];
        for (int v = 0; v < 2; ++v) {
            printf("%d waves/SIMD  %-38s ms:", w, v ? "perm -> v_add_u32 -> max3 (patterns)" : "perm -> v_pk_fma_f16 -> max3 (today)");
            for (float x : t[v]) printf(" %.3f", x);
            std::sort(t[v].begin(), t[v].end());
            med[v] = t[v][REPS / 2]; lo[v] = t[v].front(); hi[v] = t[v].back();
            printf("   median %.3f  min %.3f  max %.3f  %.2f Tcells/s  %.1f ns per row-time of a wave\n", med[v], lo[v], hi[v],
                   cells / med[v] / 1e9, med[v] * 1e6 / ((double)ROWS * BLOCKS16));
        }
        const float gain = med[0] - med[1], spread = hi[0] - lo[0];
        printf("%d waves/SIMD  results of the two streams: %zu of %zu words differ;  proposed - today = %+.2f %% of today's median, today's spread %.2f %%: %s\n",
               w, diff, nw, -100.0f * gain / med[0], 100.0f * spread / med[0], gain > spread ? "FASTER" : "not faster");
    }
    printf("%s\n", ok ? "self-check PASSED" : "self-check FAILED");
    return ok ? 0 : 1;
}
