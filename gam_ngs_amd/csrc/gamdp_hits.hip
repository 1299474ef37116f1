// libgamdp, gfx950: ABlast::findHits (lib/src/alignment/ablast.cc:41-76, lib/include/alignment/ablast.hpp:53-99) for a batch
// of queries over the packed planes of uploaded sequence sets: gamdp_find_hits_batch.
//
// The spec is the host find_hits of gamdp_l1.cpp (pinned to the reference).  Per query, after the host has applied the
// early returns and clamps of ablast.cc:47-53:
//   * k_hits_insert: one lane per a k-mer computes its code (base-4 digits 0..4, mod 2^64) and pushes its position onto the
//     chain of that code in an open-addressing table of 64-bit keys (atomic CAS on the key, atomic exchange on the chain head);
//   * k_hits_vote:   one lane per b k-mer, consecutive lanes on consecutive b positions, probes the table and walks its chain;
//     the lanes of a wavefront step through their chains together, and a run of neighbouring lanes that vote for the same
//     diagonal adds once (one atomic of +run per run head) -- a true overlap is one long such run;
//   * k_hits_collect: one workgroup per query: the maximum vote, then the diagonals holding it compacted in order, in place;
//   * k_hits_gather: the first hits_cap of each query's list packed for the download;
//   * k_hits_summary (instead of the last two when no hit list is wanted -- hits_buf == NULL, and the merge-block driver, which
//     reads hitsList.empty() / .front() / .back() alone, PctgBuilder.cc:1544-1551, 1584-1591): one workgroup per query, ONE pass
//     over the votes: maximum, number of diagonals holding it, the lowest and the highest of them.
// Everything a piece of the batch needs lives in the context's scratch arena; a batch that does not fit goes in pieces.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "gamdp_internal.h"

// the layouts gam_ngs_amd/lib.py mirrors (HitsTask, HitsResult)
static_assert(sizeof(gamdp_hits_task) == 64 && offsetof(gamdp_hits_task, word) == 28 && offsetof(gamdp_hits_task, a_start) == 32 &&
              offsetof(gamdp_hits_task, b_end) == 56, "gamdp_hits_task layout");
static_assert(sizeof(gamdp_hits_result) == 32 && offsetof(gamdp_hits_result, first) == 16 && offsetof(gamdp_hits_result, status) == 24,
              "gamdp_hits_result layout");
static_assert(sizeof(gamdp_l1_hits_stats) == 64 && offsetof(gamdp_l1_hits_stats, host_queries) == 32 && offsetof(gamdp_l1_hits_stats, hits_launches) == 40 &&
              offsetof(gamdp_l1_hits_stats, mode) == 44 && offsetof(gamdp_l1_hits_stats, hits_kernel_ms) == 48 && offsetof(gamdp_l1_hits_stats, host_hits_ms) == 56,
              "gamdp_l1_hits_stats layout");   // (L1HitsStats)
static_assert(sizeof(gamdp_l1_tail_call) == 16 && offsetof(gamdp_l1_tail_call, merge_block) == 8 && offsetof(gamdp_l1_tail_call, right) == 12 &&
              offsetof(gamdp_l1_tail_call, source) == 13, "gamdp_l1_tail_call layout");   // (L1TailCall)

namespace gamdp {
namespace {

constexpr int HT = 256;                 // threads per workgroup = k-mers per tile
constexpr u64 EMPTY_KEY = ~0ull;        // free table slot; a k-mer whose code is ~0 (word >= 32 only) has a chain of its own

// one query of a piece, as the kernels see it (all offsets in u32 words of the piece's scratch)
struct HitsQuery {
    const u32 *a2, *an, *b2, *bn;   // plane words holding base 0 of the a / b sequence (forward or reverse complement)
    u64 a_pos, b_pos;               // first a / b k-mer, in bases from base 0 of that plane (view offset included)
    u64 key_off;                    // keys: 2 * (mask + 1) words (8-byte aligned: every query's key count is even)
    u64 head_off;                   // head: mask + 1 words (0 = empty chain, else 1 + a k-mer index); then the ~0 chain's head
    u64 next_off;                   // next: na words
    u64 f_off;                      // f: nf words (votes per diagonal; the hits afterwards)
    u32 na, nb, nf, word;
    u32 mask;
    u32 a_start;                    // hits are (uint32_t)(a_start + diagonal)
    u32 tile_a, tile_b;             // first tile of this query in the insert / vote grids
};

struct HitsSum {   // what k_hits_collect finds for a query
    u32 n_hits, votes, first, last;
};

struct HitsGather {
    u64 src_off, dst_off;   // src in scratch words, dst in the packed output
    u32 n, pad_;
};

__device__ __forceinline__ u32 h_base(const u32* p2, const u32* pn, u64 i)
{
    const u32 n = (pn[i >> 5] >> (i & 31)) & 1u;
    return n ? 4u : (p2[i >> 4] >> ((i & 15) * 2)) & 3u;
}

// code = 4 * code + base over the word's bases (ablast.hpp:53-58) in u64 arithmetic: a digit 32 or more places from the end is
// multiplied by 4^32 = 2^64 and vanishes, so only the last min(word, 32) bases are read
__device__ __forceinline__ u64 h_code(const u32* p2, const u32* pn, u64 p, u32 word)
{
    const u32 L = word < 32 ? word : 32;
    u64 code = 0;
    for (u64 i = p + word - L; i < p + word; i++) code = 4 * code + h_base(p2, pn, i);
    return code;
}

__device__ __forceinline__ u64 h_slot(u64 code, u32 mask) { return (code * 0x9E3779B97F4A7C15ull) >> 17 & mask; }

// the query that owns tile t of a grid (tile_a or tile_b ascending over the queries)
template <bool B>
__device__ __forceinline__ u32 h_query_of(const HitsQuery* qs, u32 nq, u32 t)
{
    u32 lo = 0, hi = nq - 1;
    while (lo < hi) {
        const u32 mid = (lo + hi + 1) / 2;
        if ((B ? qs[mid].tile_b : qs[mid].tile_a) <= t) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(HT) void k_hits_insert(const HitsQuery* qs, u32 nq, u32* scratch)
{
    const u32 q = h_query_of<false>(qs, nq, blockIdx.x);
    const HitsQuery& Q = qs[q];
    const u32 me = (blockIdx.x - Q.tile_a) * HT + threadIdx.x;
    if (me >= Q.na) return;
    const u64 code = h_code(Q.a2, Q.an, Q.a_pos + me, Q.word);
    u32* head = scratch + Q.head_off;
    u32* at = head + (u64)Q.mask + 1;   // the ~0 chain
    if (code != EMPTY_KEY) {
        unsigned long long* keys = reinterpret_cast<unsigned long long*>(scratch + Q.key_off);
        u64 h = h_slot(code, Q.mask);
        for (;;) {   // the table holds at least twice as many slots as the query has a k-mers: a free slot exists
            const u64 old = atomicCAS(keys + h, (unsigned long long)EMPTY_KEY, (unsigned long long)code);
            if (old == EMPTY_KEY || old == code) break;
            h = (h + 1) & Q.mask;
        }
        at = head + h;
    }
    scratch[Q.next_off + me] = atomicExch(at, me + 1);
}

__global__ __launch_bounds__(HT) void k_hits_vote(const HitsQuery* qs, u32 nq, u32* scratch)
{
    const u32 q = h_query_of<true>(qs, nq, blockIdx.x);
    const HitsQuery& Q = qs[q];
    const u32 ib = (blockIdx.x - Q.tile_b) * HT + threadIdx.x;
    const u32 lane = threadIdx.x & 63;
    const u32* next = scratch + Q.next_off;
    u32* f = scratch + Q.f_off;
    u32 e = 0;   // 1 + the a k-mer this lane looks at, 0 = none left
    if (ib < Q.nb) {
        const u64 code = h_code(Q.b2, Q.bn, Q.b_pos + ib, Q.word);
        const u32* head = scratch + Q.head_off;
        if (code == EMPTY_KEY) e = head[(u64)Q.mask + 1];
        else {
            const u64* keys = reinterpret_cast<const u64*>(scratch + Q.key_off);
            for (u64 h = h_slot(code, Q.mask);; h = (h + 1) & Q.mask) {
                const u64 k = keys[h];
                if (k == code) { e = head[h]; break; }
                if (k == EMPTY_KEY) break;
            }
        }
    }
    // the lanes of the wavefront go through their chains together (the loop condition is the wavefront's)
    for (;;) {
        while (e != 0 && e - 1 < ib) e = next[e - 1];   // only pairs with idx_a >= idx_b vote (mark_found, ablast.hpp:71-78)
        const bool v = e != 0;
        if (!__any(v)) break;
        const u32 d = v ? e - 1 - ib : 0xFFFFFFFFu;
        const u32 dp = __shfl_up(d, 1);
        const bool cont = v && lane > 0 && dp == d;           // this lane extends the run of the lane below it
        const unsigned long long cm = __ballot(cont);
        if (v && !cont) {
            const u32 extra = lane == 63 ? 0u : (u32)__builtin_ctzll(~(cm >> (lane + 1)));
            atomicAdd(f + d, 1u + extra);
        }
        if (v) e = next[e - 1];
    }
}

__global__ __launch_bounds__(HT) void k_hits_collect(const HitsQuery* qs, u32* scratch, HitsSum* sums)
{
    __shared__ u32 s_w[HT / 64];
    __shared__ u32 s_max;
    const HitsQuery& Q = qs[blockIdx.x];
    u32* f = scratch + Q.f_off;
    const u32 t = threadIdx.x, lane = t & 63, w = t / 64;
    u32 m = 0;
    for (u32 i = t; i < Q.nf; i += HT) m = max(m, f[i]);
    for (int s = 32; s > 0; s >>= 1) m = max(m, (u32)__shfl_xor(m, s));
    if (lane == 0) s_w[w] = m;
    __syncthreads();
    if (t == 0) { u32 x = 0; for (int k = 0; k < HT / 64; k++) x = max(x, s_w[k]); s_max = x; }
    __syncthreads();
    m = s_max;
    if (m == 0) {
        if (t == 0) sums[blockIdx.x] = HitsSum{0, 0, 0, 0};
        return;
    }
    // the diagonals holding the maximum, in order, written over f[0 ..): a write lands at or below the index it comes from,
    // and every read of a chunk happens before the barrier its writes wait for
    u32 cnt = 0;
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    for (u32 base = 0; base < Q.nf; base += HT) {
        const u32 i = base + t;
        const bool hit = i < Q.nf && f[i] == m;
        const unsigned long long b = __ballot(hit);
        if (lane == 0) s_w[w] = (u32)__popcll(b);
        __syncthreads();
        u32 pre = cnt + (u32)__popcll(b & below), tot = 0;
        for (u32 k = 0; k < HT / 64; k++) { if (k < w) pre += s_w[k]; tot += s_w[k]; }
        __syncthreads();
        if (hit) f[pre] = Q.a_start + i;
        cnt += tot;
    }
    __syncthreads();
    if (t == 0) sums[blockIdx.x] = HitsSum{cnt, m, f[0], f[cnt - 1]};
}

// (maximum, how many hold it, the lowest and the highest index holding it) of two parts of a vote array, into the first
__device__ __forceinline__ void h_best_merge(u32& m, u32& cnt, u32& lo, u32& hi, u32 m2, u32 cnt2, u32 lo2, u32 hi2)
{
    if (m2 > m) { m = m2; cnt = cnt2; lo = lo2; hi = hi2; }
    else if (m2 == m) { cnt += cnt2; lo = min(lo, lo2); hi = max(hi, hi2); }
}

// What k_hits_collect reports, without the list: every lane folds its share of the votes (indices t, t + HT, ...) into one
// (maximum, count, lowest, highest) record, the 64 records of a wavefront fold across lanes (butterfly: every lane ends with the
// wavefront's record), the four wavefronts' records meet in LDS.  One read of f, no write to it, one barrier.
__global__ __launch_bounds__(HT) void k_hits_summary(const HitsQuery* qs, const u32* scratch, HitsSum* sums)
{
    __shared__ u32 s_r[HT / 64][4];
    const HitsQuery& Q = qs[blockIdx.x];
    const u32* f = scratch + Q.f_off;
    const u32 nf = Q.nf, t = threadIdx.x, lane = t & 63, w = t / 64;
    u32 m = 0, cnt = 0, lo = 0xFFFFFFFFu, hi = 0;   // (while m == 0 the other three count zeros: dropped at the end)
    for (u32 i = t; i < nf; i += HT) {
        const u32 v = f[i];
        if (v > m) { m = v; cnt = 1; lo = i; hi = i; }
        else if (v == m) { cnt++; lo = min(lo, i); hi = i; }
    }
    for (int s = 32; s > 0; s >>= 1)
        h_best_merge(m, cnt, lo, hi, (u32)__shfl_xor(m, s), (u32)__shfl_xor(cnt, s), (u32)__shfl_xor(lo, s), (u32)__shfl_xor(hi, s));
    if (lane == 0) { s_r[w][0] = m; s_r[w][1] = cnt; s_r[w][2] = lo; s_r[w][3] = hi; }
    __syncthreads();
    if (t == 0) {
        for (u32 k = 1; k < HT / 64; k++) h_best_merge(m, cnt, lo, hi, s_r[k][0], s_r[k][1], s_r[k][2], s_r[k][3]);
        sums[blockIdx.x] = m ? HitsSum{cnt, m, Q.a_start + lo, Q.a_start + hi} : HitsSum{0, 0, 0, 0};
    }
}

__global__ __launch_bounds__(HT) void k_hits_gather(const HitsGather* g, const u32* scratch, u32* out)
{
    const HitsGather G = g[blockIdx.x];
    for (u32 i = threadIdx.x; i < G.n; i += HT) out[G.dst_off + i] = scratch[G.src_off + i];
}

}  // namespace

// buffers of gamdp_find_hits_batch, kept between calls (Ctx::hits)
struct HitsBuffers {
    HitsQuery* d_q = nullptr; u64 cap_q = 0;
    HitsSum* d_sum = nullptr; u64 cap_sum = 0;
    HitsGather* d_g = nullptr; u64 cap_g = 0;
    u32* d_out = nullptr; u64 cap_out = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    ~HitsBuffers()
    {
        for (auto& ev : events) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
        if (d_q) (void)hipFree(d_q);
        if (d_sum) (void)hipFree(d_sum);
        if (d_g) (void)hipFree(d_g);
        if (d_out) (void)hipFree(d_out);
    }
};
void hits_free(HitsBuffers* h) { delete h; }

namespace {

#define HCHK(c, expr)                                                                             \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            (c)->set_error(std::string(#expr) + ": " + hipGetErrorString(e_));                    \
            return GAMDP_EHIP;                                                                    \
        }                                                                                         \
    } while (0)

template <class T>
int hgrow(Ctx* c, T*& p, u64& cap, u64 need)
{
    if (need <= cap) return 0;
    if (p) { c->free_dev(p); p = nullptr; cap = 0; }   // (beside a chain launch the old buffer waits for the end of the call: Ctx::defer_frees)
    u64 want = need + need / 4;
    if (hipMalloc(&p, want * sizeof(T)) != hipSuccess) {
        if (hipMalloc(&p, need * sizeof(T)) != hipSuccess) {
            c->set_error("hipMalloc of " + std::to_string(need * sizeof(T)) + " bytes failed");
            return GAMDP_ENOMEM;
        }
        want = need;
    }
    cap = want;
    return 0;
}

// a query after the early returns and clamps of ablast.cc:47-53 (find_hits in gamdp_l1.cpp): work == false means no hits
struct HitsPlan {
    bool work = false;
    u64 a_start = 0, b_start = 0, na = 0, nb = 0, nf = 0, cap = 0;
    u64 words = 0;   // scratch words
};

HitsPlan plan_query(const gamdp_hits_task& t, u64 alen, u64 blen)
{
    HitsPlan p;
    const u64 word = t.word;
    u64 a_start = t.a_start, a_end = t.a_end, b_start = t.b_start, b_end = t.b_end;
    if (alen == 0 || blen == 0) return p;                                   // ablast.cc:47
    if (a_end >= alen) a_end = alen - 1;                                    // :49-50
    if (b_end >= blen) b_end = blen - 1;
    if (a_start > a_end || b_start > b_end) return p;                       // :52
    if (a_end + 1 < word + a_start || b_end + 1 < word + b_start) return p; // :53
    if (word == 0) return p;
    p.work = true;
    p.a_start = a_start; p.b_start = b_start;
    p.na = a_end - word + 2 - a_start;
    p.nb = b_end - word + 2 - b_start;
    p.nf = a_end - a_start + 1;
    u64 cap = 16;
    while (cap < 2 * p.na) cap *= 2;
    p.cap = cap;
    p.words = 3 * cap + 2 + p.na + p.nf;
    return p;
}

}  // namespace

// one piece: queries [first, last) of the snapshot, laid out in the scratch arena and run
static int hits_piece(Ctx* c, HitsBuffers& hb, const std::vector<HitsReq>& tk, const std::vector<HitsPlan>& plan,
                      const std::vector<u32>& idx, size_t first, size_t last, gamdp_hits_result* out, uint32_t* hits_buf,
                      const std::vector<u64>& hoff, const std::vector<u64>& hcap, double* kernel_ms, u32* launches)
{
    const size_t nq = last - first;
    std::vector<HitsQuery> hq(nq);
    // three regions, so that two memsets prepare the piece: every query's keys (set to EMPTY_KEY), then its chain heads and
    // votes (set to 0), then its next links (written before they are read)
    u64 n_keys = 0, n_zero = 0, tiles_a = 0, tiles_b = 0;
    for (size_t k = 0; k < nq; k++) { const HitsPlan& p = plan[idx[first + k]]; n_keys += 2 * p.cap; n_zero += p.cap + 2 + p.nf; }
    u64 at_key = 0, at_zero = n_keys, at_next = n_keys + n_zero;
    for (size_t k = 0; k < nq; k++) {
        const u32 i = idx[first + k];
        const gamdp_hits_task& t = tk[i].t;
        const HitsPlan& p = plan[i];
        const DevSeq& da = t.a_rc ? tk[i].sa->rc[t.a_id] : tk[i].sa->fwd[t.a_id];
        const DevSeq& db = t.b_rc ? tk[i].sb->rc[t.b_id] : tk[i].sb->fwd[t.b_id];
        HitsQuery& Q = hq[k];
        Q.a2 = da.p2; Q.an = da.pn; Q.b2 = db.p2; Q.bn = db.pn;
        Q.a_pos = t.a_off + p.a_start; Q.b_pos = t.b_off + p.b_start;
        Q.key_off = at_key; Q.head_off = at_zero; Q.f_off = at_zero + p.cap + 2; Q.next_off = at_next;
        at_key += 2 * p.cap; at_zero += p.cap + 2 + p.nf; at_next += p.na;
        Q.na = (u32)p.na; Q.nb = (u32)p.nb; Q.nf = (u32)p.nf; Q.word = t.word;
        Q.mask = (u32)(p.cap - 1);
        Q.a_start = (u32)p.a_start;
        Q.tile_a = (u32)tiles_a; Q.tile_b = (u32)tiles_b;
        tiles_a += (p.na + HT - 1) / HT;
        tiles_b += (p.nb + HT - 1) / HT;
    }
    const u64 words = at_next;
    if (tiles_a >= (1ull << 31) || tiles_b >= (1ull << 31)) { c->set_error("find_hits piece needs more than 2^31 workgroups"); return GAMDP_EINVAL; }
    { int r = hgrow(c, c->d_scratch, c->cap_scratch, words); if (r) return r; }
    { int r = hgrow(c, hb.d_q, hb.cap_q, nq); if (r) return r; }
    { int r = hgrow(c, hb.d_sum, hb.cap_sum, nq); if (r) return r; }
    while (hb.events.size() < 4) {
        hipEvent_t e0, e1;
        HCHK(c, hipEventCreate(&e0));
        if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); c->set_error("hipEventCreate failed"); return GAMDP_EHIP; }
        hb.events.push_back({e0, e1});
    }
    HCHK(c, hipMemcpyAsync(hb.d_q, hq.data(), nq * sizeof(HitsQuery), hipMemcpyHostToDevice, c->stream));
    HCHK(c, hipMemsetAsync(c->d_scratch, 0xFF, (size_t)n_keys * sizeof(u32), c->stream));
    HCHK(c, hipMemsetAsync(c->d_scratch + n_keys, 0, (size_t)n_zero * sizeof(u32), c->stream));
    auto launch = [&](int li, auto kernel, u64 grid, auto... args) -> int {
        HCHK(c, hipEventRecord(hb.events[li].first, c->stream));
        hipLaunchKernelGGL(kernel, dim3((u32)grid), dim3(HT), 0, c->stream, args...);
        HCHK(c, hipGetLastError());
        HCHK(c, hipEventRecord(hb.events[li].second, c->stream));
        return 0;
    };
    int r;
    if ((r = launch(0, k_hits_insert, tiles_a, (const HitsQuery*)hb.d_q, (u32)nq, c->d_scratch))) return r;
    if ((r = launch(1, k_hits_vote, tiles_b, (const HitsQuery*)hb.d_q, (u32)nq, c->d_scratch))) return r;
    if (hits_buf) r = launch(2, k_hits_collect, nq, (const HitsQuery*)hb.d_q, c->d_scratch, hb.d_sum);
    else r = launch(2, k_hits_summary, nq, (const HitsQuery*)hb.d_q, (const u32*)c->d_scratch, hb.d_sum);
    if (r) return r;
    std::vector<HitsSum> sums(nq);
    HCHK(c, hipMemcpyAsync(sums.data(), hb.d_sum, nq * sizeof(HitsSum), hipMemcpyDeviceToHost, c->stream));
    HCHK(c, hipStreamSynchronize(c->stream));
    int n_launch = 3;
    // the hits the caller asked for, packed: one download
    std::vector<HitsGather> g;
    u64 total = 0;
    if (hits_buf) {
        for (size_t k = 0; k < nq; k++) {
            const u64 n = std::min<u64>(sums[k].n_hits, hcap[idx[first + k]]);
            if (n == 0) continue;
            g.push_back(HitsGather{hq[k].f_off, total, (u32)n, 0});
            total += n;
        }
    }
    std::vector<u32> packed(total);
    if (!g.empty()) {
        if ((r = hgrow(c, hb.d_g, hb.cap_g, g.size()))) return r;
        if ((r = hgrow(c, hb.d_out, hb.cap_out, total))) return r;
        HCHK(c, hipMemcpyAsync(hb.d_g, g.data(), g.size() * sizeof(HitsGather), hipMemcpyHostToDevice, c->stream));
        if ((r = launch(3, k_hits_gather, g.size(), (const HitsGather*)hb.d_g, (const u32*)c->d_scratch, hb.d_out))) return r;
        HCHK(c, hipMemcpyAsync(packed.data(), hb.d_out, total * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
        HCHK(c, hipStreamSynchronize(c->stream));
        n_launch = 4;
    }
    for (int li = 0; li < n_launch; li++) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, hb.events[li].first, hb.events[li].second) != hipSuccess) continue;
        c->kernel_ms += ms; c->kernel_launches++;
        if (kernel_ms) *kernel_ms += ms;
        if (launches) ++*launches;
        if (c->interval_sink && c->ref_event) {   // merge-block calls: where this launch sat on the call's time line (as Ctx::align_collect)
            float t0 = 0;
            if (hipEventElapsedTime(&t0, c->ref_event, hb.events[li].first) == hipSuccess) c->interval_sink->push_back({t0, t0 + ms});
        }
    }
    u64 pk = 0;
    for (size_t k = 0; k < nq; k++) {
        const u32 i = idx[first + k];
        gamdp_hits_result& o = out[i];
        o.n_hits = sums[k].n_hits; o.votes = sums[k].votes; o.first = sums[k].first; o.last = sums[k].last;
        if (hits_buf) {
            const u64 n = std::min<u64>(sums[k].n_hits, hcap[i]);
            if (n) std::memcpy(hits_buf + hoff[i], packed.data() + pk, (size_t)n * sizeof(u32));
            pk += n;
        }
    }
    return 0;
}

int find_hits_queries(Ctx* c, const HitsReq* q, size_t n, gamdp_hits_result* out, uint32_t* hits_buf, const uint64_t* hits_off,
                      const uint64_t* hits_cap, uint8_t* how, double* kernel_ms, u32* launches)
{
    // the caller's arrays are read once, here
    const std::vector<HitsReq> tk(q, q + n);
    std::vector<u64> hoff, hcap;
    if (hits_buf) { hoff.assign(hits_off, hits_off + n); hcap.assign(hits_cap, hits_cap + n); }
    for (size_t i = 0; i < n; i++) {
        const gamdp_hits_task& t = tk[i].t;
        if (t.a_id >= tk[i].sa->lens.size() || t.b_id >= tk[i].sb->lens.size()) {
            c->set_error("find_hits query " + std::to_string(i) + ": sequence id out of range");
            return GAMDP_EINVAL;
        }
        if ((t.a_rc && !tk[i].sa->has_codes()) || (t.b_rc && !tk[i].sb->has_codes())) {
            c->set_error("find_hits query " + std::to_string(i) + ": reverse complement requested on a packed-only (synthetic) sequence set");
            return GAMDP_EINVAL;
        }
    }
    const u64 arena_words = c->arena_call() / sizeof(u32);
    std::vector<HitsPlan> plan(n);
    std::vector<u32> idx;   // the queries that run on the device, in batch order
    for (size_t i = 0; i < n; i++) {
        const gamdp_hits_task& t = tk[i].t;
        gamdp_hits_result& o = out[i];
        std::memset(&o, 0, sizeof(o));
        if (how) how[i] = HITS_TRIVIAL;
        const u64 alen_full = tk[i].sa->lens[t.a_id], blen_full = tk[i].sb->lens[t.b_id];
        if (t.a_off > alen_full || t.b_off > blen_full) { o.status = GAMDP_ST_INVALID; continue; }
        o.status = GAMDP_ST_OK;
        plan[i] = plan_query(t, alen_full - t.a_off, blen_full - t.b_off);
        if (!plan[i].work) continue;
        if (plan[i].words > arena_words) {
            if (how) { how[i] = HITS_UNFIT; continue; }
            c->set_error("find_hits query " + std::to_string(i) + " needs " + std::to_string(plan[i].words * sizeof(u32)) +
                         " bytes of scratch; the arena allows " + std::to_string(arena_words * sizeof(u32)));
            return GAMDP_ENOMEM;
        }
        if (how) how[i] = HITS_DEVICE;
        idx.push_back((u32)i);
    }
    if (idx.empty()) return 0;
    // the reverse complements the device queries read, set by set (SeqSet::ensure_rc: shared by the cohort threads of a
    // merge-block call under the set's rc_mu)
    std::vector<std::pair<const SeqSet*, std::vector<u32>>> need;
    auto want_rc = [&](const SeqSet* s, u32 id) {
        for (auto& e : need) if (e.first == s) { e.second.push_back(id); return; }
        need.push_back({s, {id}});
    };
    for (u32 i : idx) {
        if (tk[i].t.a_rc) want_rc(tk[i].sa, tk[i].t.a_id);
        if (tk[i].t.b_rc) want_rc(tk[i].sb, tk[i].t.b_id);
    }
    for (auto& e : need) { int r = e.first->ensure_rc(e.second, c); if (r) return r; }
    if (!c->hits) c->hits = new HitsBuffers();
    // pieces: consecutive queries while their scratch fits the arena (and the tile counts stay far below 2^31)
    size_t first = 0;
    while (first < idx.size()) {
        size_t last = first;
        u64 words = 0, tiles = 0;
        while (last < idx.size()) {
            const HitsPlan& p = plan[idx[last]];
            const u64 t = (std::max(p.na, p.nb) + HT - 1) / HT;
            if (last > first && (words + p.words > arena_words || tiles + t > (1ull << 30))) break;
            words += p.words; tiles += t;
            last++;
        }
        const int r = hits_piece(c, *c->hits, tk, plan, idx, first, last, out, hits_buf, hoff, hcap, kernel_ms, launches);
        if (r) return r;
        first = last;
    }
    return 0;
}

}  // namespace gamdp

using namespace gamdp;

extern "C" int gamdp_find_hits_batch(gamdp_ctx* ctx, const gamdp_seqset* set_a, const gamdp_seqset* set_b,
                                     const gamdp_hits_task* tasks, size_t n, gamdp_hits_result* out, uint32_t* hits_buf,
                                     const uint64_t* hits_off, const uint64_t* hits_cap)
{
    if (!ctx || !set_a || !set_b || (n && (!tasks || !out)) || (n && hits_buf && (!hits_off || !hits_cap))) return GAMDP_EINVAL;
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    return guarded(c, [&]() -> int {
        if (c->arena_budget(true) == 0) { c->set_error("hipMemGetInfo failed"); return GAMDP_EHIP; }
        if (hipSetDevice(c->device) != hipSuccess) { c->set_error("hipSetDevice failed"); return GAMDP_EHIP; }
        std::vector<HitsReq> q(n);
        for (size_t i = 0; i < n; i++) q[i] = HitsReq{reinterpret_cast<const SeqSet*>(set_a), reinterpret_cast<const SeqSet*>(set_b), tasks[i]};
        return find_hits_queries(c, q.data(), n, out, hits_buf, hits_off, hits_cap, nullptr);
    });
}
