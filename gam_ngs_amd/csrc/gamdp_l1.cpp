// L1: the merge-block chain driver -- a batched, round-based re-design of
//   PctgBuilder::alignMergeBlock    lib/src/pctg/PctgBuilder.cc:726-844
//   PctgBuilder::findBestAlignment  :1361-1614
//   PctgBuilder::alignBlocks        :1617-1708
//   PctgBuilder::is_good            :1711-1730
// and ABlast::findHits (lib/src/alignment/ablast.cc:41-76).
//
// The reference walks one merge block at a time and blocks on every find_alignment call.  Inside a
// merge block the DP calls form a serial chain (block k starts where block k-1's last match ended,
// then up to one orientation retry and two tail alignments), but different merge blocks are
// independent (BuildPctgFunctions.cc:82-84).  Here every merge block is a small state machine; each
// round collects the next pending DP call of every unfinished merge block into ONE gamdp L0 batch on
// the GPU, feeds the results back and advances the machines.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "gamdp.h"
#include "gamdp_internal.h"

namespace gamdp {

// ---- ABlast::findHits ---------------------------------------------------------------------------
void find_hits(const uint8_t* a, u64 alen, u64 a_start, u64 a_end, const uint8_t* b, u64 blen, u64 b_start, u64 b_end,
               u64 word, std::vector<uint32_t>& hits)
{
    hits.clear();
    if (alen == 0 || blen == 0) return;                                   // ablast.cc:47
    if (a_end >= alen) a_end = alen - 1;                                  // :49-50
    if (b_end >= blen) b_end = blen - 1;
    if (a_start > a_end || b_start > b_end) return;                       // :52
    if (a_end + 1 < word + a_start || b_end + 1 < word + b_start) return; // :53
    if (word == 0) return;

    // k-mer codes are base-4 numbers with digits 0..4 (ablast.hpp:53-59), rolled along the window
    u64 top = 1;  // 4^(word-1) mod 2^64
    for (u64 i = 1; i < word; i++) top *= 4;
    auto roll = [&](const uint8_t* s, u64 first, u64 last, auto&& emit) {
        u64 code = 0;
        for (u64 i = first; i < first + word; i++) code = 4 * code + s[i];
        for (u64 p = first;; p++) {
            emit(code, p);
            if (p == last) break;
            code = 4 * (code - top * s[p]) + s[p + word];
        }
    };
    // index of the a k-mers: open-addressing table code -> chain of positions (the reference keeps a std::map of
    // position lists, ablast.hpp:61-69; only the multiset of (code, position) pairs matters for the vote)
    const u64 n_a = a_end - word + 2 - a_start;
    u64 cap = 16;
    while (cap < 2 * n_a) cap *= 2;
    static thread_local std::vector<u64> keys;
    static thread_local std::vector<u32> head, next;
    keys.assign(cap, 0);
    head.assign(cap, 0);  // 0 = empty slot, else 1 + index of the newest position in the chain
    next.assign(n_a, 0);
    const u64 mask = cap - 1;
    auto slot_of = [&](u64 code) {
        u64 h = (code * 0x9E3779B97F4A7C15ull) >> 17 & mask;
        while (head[h] != 0 && keys[h] != code) h = (h + 1) & mask;
        return h;
    };
    roll(a, a_start, a_end - word + 1, [&](u64 code, u64 p) {
        const u64 h = slot_of(code);
        const u32 me = (u32)(p - a_start);
        keys[h] = code;
        next[me] = head[h];
        head[h] = me + 1;
    });

    std::vector<u64> f(a_end - a_start + 1, 0);
    roll(b, b_start, b_end - word + 1, [&](u64 code, u64 bp) {
        const u64 ib = bp - b_start;
        for (u32 e = head[slot_of(code)]; e != 0; e = next[e - 1]) {
            const u64 ia = e - 1;
            if (ia >= ib) f[ia - ib]++;  // mark_found, ablast.hpp:71-78
        }
    });
    u64 best = 0;
    for (u64 v : f) best = std::max(best, v);
    if (best == 0) return;
    for (u64 i = 0; i < f.size(); i++)
        if (f[i] == best) hits.push_back((uint32_t)(a_start + i));
}

// ---- merge-block state machine ------------------------------------------------------------------
namespace {

constexpr double MIN_HOMOLOGY = 95.0;  // PctgBuilder.hpp:63

inline int32_t frame_len(int32_t b, int32_t e) { return e < b ? 0 : e - b + 1; }  // Frame.cc:124-127
inline u64 umin(u64 x, u64 y) { return x < y ? x : y; }

// The host's 1 B/base reverse complements of the slave contigs of one call, built on first use, shared by its cohort threads
struct RcCache {
    std::unordered_map<u32, std::vector<uint8_t>> map;
    std::mutex mu;
    const uint8_t* get(const SeqSet* ss, u32 id)
    {
        std::lock_guard<std::mutex> g(mu);  // node-based map: the data pointer stays valid after unlock
        auto it = map.find(id);
        if (it != map.end()) return it->second.data();
        std::vector<uint8_t> r = ss->codes[id];
        gamdp_revcomp(r.data(), r.size());
        return map.emplace(id, std::move(r)).first->second.data();
    }
};

struct Machine {
    enum Phase { MAIN, LEFT, RIGHT, DONE };   // LEFT / RIGHT also name the side of a tail alignment
    const gamdp_mb_in* in = nullptr;
    gamdp_mb_out* out = nullptr;
    const SeqSet *ms = nullptr, *ss = nullptr;
    u64 mlen = 0, slen = 0;
    u32 band = GAMDP_DEFAULT_BAND;
    Phase phase = DONE;
    // region (alignMergeBlock :741-744) and orientation evidence (findBestAlignment :1380-1408)
    u64 m_start = 0, s_start = 0, s_end = 0;
    double con_prob = 0;
    u64 mt = 0, st = 0, align_thr = 0, thr = 0;
    bool forward = true;
    // main chain
    int attempt = 0;
    bool try_rev = false;
    u32 k = 0;
    int64_t cur_ms = 0, cur_ss = 0;
    u64 last_a = 0, last_b = 0;
    std::vector<gamdp_result> A;
    bool rev = false;
    // tails
    u64 sa = 0, sb = 0, ea = 0, eb = 0, i1 = 0, i2 = 0, j1 = 0, j2 = 0;
    gamdp_result left{}, right{};
    bool left_rev = false, right_rev = false;  // the reference leaves these uninitialised when a tail is skipped
    // audit
    gamdp_result* audit = nullptr;
    u32 audit_cap = 0;
    bool on_device = false;   // its main chain is part of the chain launch of this call (launch_main_chains)

    const gamdp_block& blk(u32 i) const { return forward ? in->blocks[i] : in->blocks[in->n_blocks - 1 - i]; }

    void finish_bad(int status)
    {
        out->status = (uint8_t)status;
        out->align_ok = 0;
        phase = DONE;
    }

    void init()
    {
        out->align_ok = 1;  // :757
        out->align_rev = 0; out->status = GAMDP_ST_OK; out->coords_set = 0;
        out->m_start = out->m_end = out->s_start = out->s_end = 0;
        out->n_dp = 0; out->cells = 0;
        const u32 n = in->n_blocks;
        if (n == 0 || !in->blocks) { finish_bad(GAMDP_ST_INVALID); return; }  // front() of an empty list: UB
        const gamdp_block &fb = in->blocks[0], &lb = in->blocks[n - 1];
        m_start = (u64)(int64_t)std::min(fb.m_begin, lb.m_begin);
        s_start = (u64)(int64_t)std::min(fb.s_begin, lb.s_begin);
        s_end = (u64)(int64_t)std::max(fb.s_end, lb.s_end);
        forward = fb.m_begin <= lb.m_begin;  // :1650
        u64 con = 0, dis = 0;
        int32_t min_frame_len = 100;
        for (u32 i = 0; i < n; i++) {
            const gamdp_block& b = in->blocks[i];
            const int32_t mn = std::min(frame_len(b.m_begin, b.m_end), frame_len(b.s_begin, b.s_end));
            if (i == 0 || min_frame_len > mn) min_frame_len = mn;
            if (b.m_strand != b.s_strand) dis += (u64)b.n_reads; else con += (u64)b.n_reads;
        }
        con_prob = (double)con / (double)(con + dis);
        mt = (u64)(0.3 * (double)mlen);
        st = (u64)(0.3 * (double)slen);
        align_thr = (u64)(int64_t)(int32_t)(0.7 * min_frame_len);
        thr = (u64)(int64_t)(int32_t)umin(200, umin(mt, st));
        A.assign(n, gamdp_result{});
        attempt = 0;
        if (con_prob >= 0.5) try_rev = false;
        else if (con_prob < 0.5) try_rev = true;
        else { finish_bad(GAMDP_ST_OK); return; }  // NaN: neither branch of :1420/:1463 runs
        start_attempt();
    }

    void start_attempt()
    {
        phase = MAIN;
        k = 0;
        cur_ms = (int64_t)m_start;
        // reverse_complement maps (start,end) -> (|s|-end-1, |s|-start-1), :1446-1448
        cur_ss = (int64_t)(try_rev ? slen - s_end - 1 : s_start);
        last_a = last_b = 0;
    }

    // MAIN: the next find_alignment call of the chain (alignBlocks, :1652-1677)
    void pending(ITask& t)
    {
        t = ITask{};
        t.band = band;
        const gamdp_block& cur = blk(k);
        const int32_t ml = frame_len(cur.m_begin, cur.m_end), sl = frame_len(cur.s_begin, cur.s_end);
        if (k > 0) {  // :1660-1667
            const gamdp_block& prev = blk(k - 1);
            const int32_t mgap = prev.m_begin <= cur.m_begin ? (cur.m_begin - prev.m_end - 1) : (prev.m_begin - cur.m_end - 1);
            const int32_t sgap = prev.s_begin <= cur.s_begin ? (cur.s_begin - prev.s_end - 1) : (prev.s_begin - cur.s_end - 1);
            cur_ms = (int64_t)(last_a + (u64)(int64_t)mgap); if (cur_ms < 0) cur_ms = 0;
            cur_ss = (int64_t)(last_b + (u64)(int64_t)sgap); if (cur_ss < 0) cur_ss = 0;
        }
        t.sa = ms; t.a_id = (u32)in->m_id; t.sb = ss; t.b_id = (u32)in->s_id; t.b_rc = try_rev;
        t.begin_a = (u64)cur_ms; t.end_a = (u64)(cur_ms + ml - 1);
        t.begin_b = (u64)cur_ss; t.end_b = (u64)(cur_ss + sl - 1);
    }

    // How the tail alignment of one side, and the findHits call that seeds it, see the two contigs (PctgBuilder.cc:1535-1611):
    // the contig with less left over on that side is the `a` sequence, the reversed slave is an *_rc view, the right tail's
    // chop_begin copy of `a` a suffix view.  Valid once the main chain is good (after_main_good).
    struct TailView {
        bool a_slave, a_rc, b_rc;  // the slave contig is `a`; the views are reversed
        const SeqSet *sa, *sb;
        u32 a_id, b_id;
        u64 alen, blen;            // the whole contigs
        u64 xa, xb;                // where the main alignment ends on this side, in a and in b: its first match (LEFT), its last (RIGHT)
        u64 a_off;                 // RIGHT: the suffix view of `a` starts behind xa;  LEFT: 0
    };
    TailView tail_view(Phase side) const
    {
        TailView v;
        const bool s = v.a_slave = side == LEFT ? i1 < j1 : i2 < j2;
        v.sa = s ? ss : ms; v.sb = s ? ms : ss;
        v.a_id = (u32)(s ? in->s_id : in->m_id); v.b_id = (u32)(s ? in->m_id : in->s_id);
        v.a_rc = s && rev; v.b_rc = !s && rev;
        v.alen = s ? slen : mlen; v.blen = s ? mlen : slen;
        const u64 xm = side == LEFT ? sa : ea, xs = side == LEFT ? sb : eb;
        v.xa = s ? xs : xm; v.xb = s ? xm : xs;
        v.a_off = side == LEFT ? 0 : v.xa + 1;
        return v;
    }

    // A tail, step 1: the ABlast(20).findHits call that seeds the alignment (PctgBuilder.cc:1544, 1554 left; :1584, 1597 right),
    // as a query over the views.  The windows are the reference's own numbers (xa - 1 / xb - 1 wrap when a threshold is 0); the
    // clamps of ablast.cc:47-53 are applied by whoever answers the query (find_hits on the host, plan_query on the device).
    void tail_query(Phase side, HitsReq& q) const
    {
        const TailView v = tail_view(side);
        q = HitsReq{};
        q.sa = v.sa; q.sb = v.sb;
        gamdp_hits_task& h = q.t;
        h.word = 20;
        h.a_id = v.a_id; h.b_id = v.b_id; h.a_rc = v.a_rc; h.b_rc = v.b_rc; h.a_off = v.a_off;
        if (side == LEFT) { h.a_start = 0; h.a_end = v.xa - 1; h.b_start = 0; h.b_end = v.xb - 1; }
        else { h.a_start = 0; h.a_end = v.alen - v.a_off - 1; h.b_start = v.xb + 1; h.b_end = v.blen - 1; }
    }

    // ... answered on the host's codes (the reversed slave from the call's cache)
    void host_tail_hits(Phase side, const HitsReq& q, RcCache& rc, std::vector<uint32_t>& hits) const
    {
        const TailView v = tail_view(side);
        const uint8_t* mc = ms->codes[in->m_id].data();
        const uint8_t* sc = rev ? rc.get(ss, (u32)in->s_id) : ss->codes[in->s_id].data();
        const gamdp_hits_task& h = q.t;
        find_hits((v.a_slave ? sc : mc) + h.a_off, v.alen - h.a_off, h.a_start, h.a_end, v.a_slave ? mc : sc, v.blen, h.b_start,
                  h.b_end, h.word, hits);
    }

    // A tail, step 2: the find_alignment call, given what the driver reads of the hits list: hitsList.empty(), .back() for the
    // left tail (:1544-1551, 1554-1561, force_end), .front() for the right one (:1584-1591, 1597-1604, force_start)
    void tail_task(Phase side, ITask& t, const u64 n_hits, const u32 first, const u32 last) const
    {
        const TailView v = tail_view(side);
        t = ITask{};
        t.band = band;
        t.sa = v.sa; t.sb = v.sb; t.a_id = v.a_id; t.b_id = v.b_id; t.a_rc = v.a_rc; t.b_rc = v.b_rc; t.a_off = v.a_off;
        if (side == LEFT) {
            t.force_end = true;
            t.begin_a = n_hits == 0 ? v.xa - v.xb : last; t.end_a = v.xa - 1; t.begin_b = 0; t.end_b = v.xb - 1;
        } else {
            t.force_start = true;
            t.begin_a = n_hits == 0 ? 0 : first; t.end_a = v.alen - v.a_off - 1; t.begin_b = v.xb + 1; t.end_b = v.blen - 1;
        }
    }

    bool good_vec() const
    {  // is_good(vector), :1711-1724
        u64 len = 0;
        for (const gamdp_result& r : A) { if (r.homology < MIN_HOMOLOGY) return false; len += r.length; }
        return len >= align_thr;
    }
    static bool good_one(const gamdp_result& r, u64 min_len) { return r.homology >= MIN_HOMOLOGY && r.length >= min_len; }

    // LEFT phase only: will the right tail be aligned once the left one is fed?  (It depends on the main chain alone -- the
    // two tail alignments of findBestAlignment, :1535-1611, do not use each other's result -- so the round loop issues both in
    // one round; they are fed left first, as the reference computes them.)
    bool right_follows_left() const
    {
        if (!(umin(i2, j2) >= thr)) return false;
        return !((i2 < j2 && slen <= eb + 1) || (!(i2 < j2) && mlen <= ea + 1));   // (else chop_borders throws: enter_right_or_finalize)
    }

    void enter_right_or_finalize()
    {
        if (umin(i2, j2) >= thr) {
            // chop_borders throws std::domain_error when nothing is left to keep (contig.code.hpp:236-238)
            if ((i2 < j2 && slen <= eb + 1) || (!(i2 < j2) && mlen <= ea + 1)) { finish_bad(GAMDP_ST_OUT_OF_RANGE); return; }
            phase = RIGHT;
        } else finalize();
    }

    void after_main_good()
    {
        sa = A.front().first_a; sb = A.front().first_b;     // :1515-1517
        ea = A.back().last_a; eb = A.back().last_b;
        i1 = sa; i2 = mlen - ea - 1; j1 = sb; j2 = slen - eb - 1;
        std::memset(&left, 0, sizeof(left)); std::memset(&right, 0, sizeof(right));
        left.homology = right.homology = 100.0;             // MyAlignment(100)
        left_rev = right_rev = false;
        if (umin(i1, j1) < thr && umin(i2, j2) < thr) { finalize(); return; }  // :1526
        if (umin(i1, j1) >= thr) phase = LEFT;
        else enter_right_or_finalize();
    }

    // left_rev / right_rev ("the slave was `a`") are set here, with the result they describe, not where the call is built: a
    // tail that is skipped is never fed and keeps the `false` of after_main_good, and finalize() -- their only reader -- runs
    // after every call that was built has been fed (or not at all: a failed call ends the machine in finish_bad).
    void feed(const gamdp_result& r)
    {
        if (audit && out->n_dp < audit_cap) audit[out->n_dp] = r;
        out->n_dp++;
        out->cells += r.cells;
        if (r.status == GAMDP_ST_OUT_OF_RANGE || r.status == GAMDP_ST_INVALID) { finish_bad(r.status); return; }
        if (phase == MAIN) {
            A[k] = r;
            last_a = r.last_a; last_b = r.last_b;  // last_match_pos; (0,0) for an empty alignment
            if (++k < in->n_blocks) return;
            if (good_vec()) { rev = try_rev; after_main_good(); return; }
            if (++attempt == 2) { finish_bad(GAMDP_ST_OK); return; }  // :1512 -> :825-829, coords untouched
            try_rev = !try_rev;
            start_attempt();
        } else if (phase == LEFT) {
            left = r; left_rev = tail_view(LEFT).a_slave;
            enter_right_or_finalize();
        } else if (phase == RIGHT) {
            right = r; right_rev = tail_view(RIGHT).a_slave;
            finalize();
        }
    }

    void finalize()
    {  // alignMergeBlock :759-843 (main_homology() >= 95 is implied by good_vec())
        const u64 thr2 = umin(100, umin(mt, st));
        const u64 left_min = (u64)(0.7 * (double)umin(i1, j1));
        const u64 right_min = (u64)(0.7 * (double)umin(i2, j2));
        const bool s_lt = rev ? in->s_rtail : in->s_ltail;
        const bool s_rt = rev ? in->s_ltail : in->s_rtail;
        u64 Sa = sa, Sb = sb, Ea = ea, Eb = eb;
        if (in->m_ltail && s_lt && umin(i1, j1) >= thr2) {
            if (good_one(left, left_min)) {
                Sa = left.first_a; Sb = left.first_b;
                if (left_rev) std::swap(Sa, Sb);
            } else out->align_ok = 0;
        }
        if (in->m_rtail && s_rt && umin(i2, j2) >= thr2) {
            if (good_one(right, right_min)) {
                u64 ta = right.last_a, tb = right.last_b;
                if (right_rev) { std::swap(ta, tb); Ea = ta; Eb += tb + 1; }
                else { Ea += ta + 1; Eb = tb; }
            } else out->align_ok = 0;
        }
        if (rev) { const u64 t = Sb; Sb = slen - Eb - 1; Eb = slen - t - 1; }  // :831-836
        out->align_rev = rev;
        out->m_start = (int32_t)Sa; out->m_end = (int32_t)Ea;
        out->s_start = (int32_t)Sb; out->s_end = (int32_t)Eb;
        out->coords_set = 1;
        phase = DONE;
    }
};

}  // namespace
}  // namespace gamdp

using namespace gamdp;

namespace gamdp {
namespace {

// ---- the main chains on the device (k_chain2, gamdp_dev.h) -----------------------------------------------------------
// One launch takes every merge block through alignBlocks' chain and the orientation retry.  It runs on its own stream beside
// the round loop: a chain that ends copies its result records into a pinned mirror and raises a flag; the cohort that owns the
// merge block then replays its own machine over those records (so every decision is taken twice: a difference is an internal
// error, not a wrong answer) and sends what is left -- the tail alignments, at most two more calls -- through its next round,
// while longer chains are still running.  GAMDP_L1_CHAIN_WALK: scratch slots from the arena; k_chain2 at band 150 (the only band
// gam-merge runs) and, for a context set to GAMDP_L1_WALK_ANY_BAND, k_chain2g<C> at every other band up to GAMDP_MAX_TUNED_BAND (the
// same workgroup around the generic cell).  GAMDP_L1_CHAIN_CARRY (k_chain_c, gamdp_chain_carry.hip): any band up to
// GAMDP_MAX_TUNED_BAND, no scratch, one launch, no twins.  Anything else, and GAMDP_L1_ROUNDS=1, keeps the round loop for the whole call.
struct ChainRun {
    bool launched = false;
    size_t n_mb = 0;
    u32 band = 0;
    std::vector<u32> q_of;     // machine -> its index in the launch (~0u: not part of it)
    const DevMB* hmb = nullptr;
    const ChainOut* hout = nullptr;
    const DevResult* haud = nullptr;
    const ChainWin* hwin = nullptr;
    const volatile u32* done = nullptr;
    u32 epoch = 0;
    hipStream_t stream = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const ChainOut* dout = nullptr;   // device copy of the ChainOut list (progress markers in the diagnostics build)
    bool n_by_contig = false;         // the launch ran every call of a chain with N in its contigs on the N-aware cells
    ChainKernel kernel{};             // which kernel the launch is (pick_chain_kernel; gamdp_l1_chain_stats)
    u64 scratch_bytes = 0;
    u32 n_launches = 0, n_twins = 0;
    const SeqSet *ms = nullptr, *ss = nullptr;
    std::chrono::steady_clock::time_point t_launch;

    ChainRun() = default;
    ChainRun(const ChainRun&) = delete;
    ChainRun& operator=(const ChainRun&) = delete;
    // the one place the events of a launch end: after finish(), or with the object (a launch that failed half-way included)
    void drop_events()
    {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        e0 = e1 = nullptr;
    }
    ~ChainRun()
    {
        if (launched) (void)hipStreamSynchronize(stream);   // (only on a path that skipped finish(): an exception between the launch and the join)
        drop_events();
    }

    bool ended(u32 q) const
    {
        if (done[q] != epoch) return false;
        std::atomic_thread_fence(std::memory_order_acquire);
        return true;
    }
    // waits for the launch (all paths out of the call, errors included: its buffers belong to the context)
    int finish(Ctx* c, float* from_ref_ms, float* ms)
    {
        if (!launched) return 0;
        launched = false;
        bool ok = hipStreamSynchronize(stream) == hipSuccess;
        float k = 0, f = 0;
        if (ok) ok = hipEventElapsedTime(&k, e0, e1) == hipSuccess && hipEventElapsedTime(&f, c->ref_event, e0) == hipSuccess;
        drop_events();
        if (!ok) { c->set_error(std::string("chain kernel: ") + hipGetErrorString(hipGetLastError())); return GAMDP_EHIP; }
        *ms = k; *from_ref_ms = f;
        c->kernel_ms += k; c->kernel_launches++;
        if (diag().timing) {
            std::fprintf(stderr, "gamdp chain: kernel %.3f ms, launched %.3f ms after the call began\n", k, f);
        }
        if (diag().timing && diag().build) {   // (the product kernels read no clock: ChainOut's t_* / hw fields are 0 there)
            // the chains that ended last (the device's 100 MHz clock, relative to the first workgroup's start)
            std::vector<u32> idx(n_mb);
            u32 t0 = hout[0].t_begin;
            for (size_t q = 0; q < n_mb; q++) { idx[q] = (u32)q; if ((int32_t)(hout[q].t_begin - t0) < 0) t0 = hout[q].t_begin; }
            std::sort(idx.begin(), idx.end(), [&](u32 a, u32 b) { return (int32_t)(hout[a].t_end - hout[b].t_end) > 0; });
            {   // the twin that ended last
                size_t qm = 0; int32_t lm = -1;
                for (size_t q = 0; q < n_mb; q++) if (hout[q].t_end_att[1] && (int32_t)(hout[q].t_end_att[1] - t0) > lm) { lm = (int32_t)(hout[q].t_end_att[1] - t0); qm = q; }
                if (lm >= 0) std::fprintf(stderr, "gamdp chain: last twin to end: #%zu's, at %.3f ms (its chain was handed over at %.3f)\n", qm, lm * 1e-5, (hout[qm].t_end - t0) * 1e-5);
            }
            for (size_t i = 0; i < std::min<size_t>(6, n_mb); i++) {
                const u32 q = idx[i];
                std::fprintf(stderr, "gamdp chain: #%u ended at %.3f ms (began %.3f): %u blocks, %u rows, %u calls, has_n %u, state 0x%x\n", q, (hout[q].t_end - t0) * 1e-5,
                             (hout[q].t_begin - t0) * 1e-5, hmb[q].n_blocks, hmb[q].rows, hout[q].n_dp, hmb[q].has_n, hout[q].state);
                auto place = [](u32 h) { char b[64]; std::snprintf(b, sizeof b, "xcc %u se %u sh %u cu %u simd %u", h >> 16, (h >> 13) & 7, (h >> 12) & 1, (h >> 8) & 15, (h >> 4) & 3); return std::string(b); };
                if (hout[q].t_end_att[1]) std::fprintf(stderr, "gamdp chain:     first attempt ended at %.3f ms, the twin began at %.3f and ended at %.3f ms\n", (hout[q].t_end_att[0] - t0) * 1e-5, (hout[q].t_begin2 - t0) * 1e-5, (hout[q].t_end_att[1] - t0) * 1e-5);
                std::fprintf(stderr, "gamdp chain:     filler on %s%s%s\n", place(hout[q].hw).c_str(), hout[q].hw_twin ? "; twin's on " : "", hout[q].hw_twin ? place(hout[q].hw_twin).c_str() : "");
            }
        }
        return 0;
    }
    // diagnostics build: the progress markers of the chains
    void dump(FILE* f) const
    {
        hipStream_t s2;
        if (hipStreamCreateWithFlags(&s2, hipStreamNonBlocking) != hipSuccess) return;
        std::vector<ChainOut> o(n_mb);
        (void)hipMemcpyAsync(o.data(), dout, n_mb * sizeof(ChainOut), hipMemcpyDeviceToHost, s2);
        (void)hipStreamSynchronize(s2);
        for (size_t q = 0; q < n_mb; q++) std::fprintf(f, "gamdp chain watchdog: mb %zu n_blocks %u: n_dp %u state 0x%x flag %u\n", q, hmb[q].n_blocks, o[q].n_dp, o[q].state, (unsigned)(done[q] == epoch));
        std::fflush(f);
        (void)hipStreamDestroy(s2);
    }
};

// The launch in steps (launch_main_chains below runs them in this order); steps 1, 2, 4 and 5 are plain host code.
// 1. Select and order: the machines whose main chain goes to the device, longest chains first.
//    A merge block with an empty slave frame (s_end < s_begin) stays with the round loop: the call of such a block that starts at
//    slave base 0 has end_b = begin_b - 1 wrapped around (the reference computes it in unsigned long, PctgBuilder.cc:1669-1677),
//    so its rows are bounded by the contig, not by the frame the scratch slots are sized for.
struct ChainPick { u32 mi; u64 rows; u32 longest; };   // a machine, the rows of its chain (the sum of its slave frames), its longest slave frame: no call of the chain has more rows
struct ChainSel {
    std::vector<ChainPick> ch;
    std::vector<u32> need_rc;   // the slave contigs (their reverse complements must be resident)
    u64 n_blk = 0, n_tw = 0;
    bool has_n = false;
};
ChainSel select_chains(const std::vector<Machine>& M, const SeqSet* ms, const SeqSet* ss)
{
    ChainSel s;
    for (u32 i = 0; i < (u32)M.size(); i++) {
        if (M[i].phase != Machine::MAIN) continue;
        const gamdp_mb_in& in = *M[i].in;
        ChainPick p{i, 0, 1};
        bool empty_frame = false;
        for (u32 k = 0; k < in.n_blocks; k++) {
            const int32_t sl = frame_len(in.blocks[k].s_begin, in.blocks[k].s_end);
            empty_frame = empty_frame || in.blocks[k].s_end < in.blocks[k].s_begin;
            p.rows += (u64)sl;
            p.longest = std::max<u32>(p.longest, (u32)sl);
        }
        if (empty_frame) continue;
        s.ch.push_back(p);
        s.n_blk += in.n_blocks;
        s.has_n = s.has_n || ms->has_n[in.m_id] || ss->has_n[in.s_id];
        s.need_rc.push_back((u32)in.s_id);
    }
    std::stable_sort(s.ch.begin(), s.ch.end(), [](const ChainPick& x, const ChainPick& y) { return x.rows > y.rows; });
    // the longest chains get a twin workgroup for their second orientation (ChainSync, gamdp_dev.h): those within 1/8 of the
    // longest, at most 256 of them; GAMDP_L1_NO_TWINS=1: none
    const u64 n_mb = s.ch.size();
    const u64 tw_cap = n_mb < 256 ? std::max<u64>(16, 256 - n_mb) : 256;   // (a small call: one workgroup per CU as long as that leaves room for a few)
    if (!tuning().l1_no_twins)
        while (s.n_tw < n_mb && s.n_tw < tw_cap && s.ch[s.n_tw].rows * 8 >= s.ch[0].rows && s.ch[s.n_tw].rows >= 1024) s.n_tw++;
    return s;
}

// 2. Layout (byte offsets, each a multiple of 256).
//    Ctx::d_chain:   DevMB[n_mb] | DevBlk[n_blk] | ChainSync[n_tw + 1] | ChainOut[n_mb] | DevResult audit[2 n_blk] | ChainWin[2 n_blk]
//                    -- the first three, [0, out), are written on the host (Ctx::h_chain) and uploaded
//    Ctx::h_mirror:  ChainOut[n_mb] | done flags u32[n_mb] | DevResult audit[2 n_blk] | ChainWin[2 n_blk]
//                    -- pinned and coherent: written by the chains as they end
struct ChainLayout {
    u64 n_mb, n_audit;
    u64 mb, blk, sync, out, aud, win, total;
    u64 m_out, m_done, m_aud, m_win, m_total;
    ChainLayout(const u64 n_mb_, const u64 n_blk, const u64 n_tw) : n_mb(n_mb_), n_audit(2 * n_blk)
    {
        auto up = [](u64 v) { return (v + 255) & ~255ull; };
        mb = 0; blk = up(mb + n_mb * sizeof(DevMB)); sync = up(blk + n_blk * sizeof(DevBlk)); out = up(sync + (n_tw + 1) * sizeof(ChainSync));
        aud = up(out + n_mb * sizeof(ChainOut)); win = up(aud + n_audit * sizeof(DevResult)); total = up(win + n_audit * sizeof(ChainWin));
        m_out = 0; m_done = up(m_out + n_mb * sizeof(ChainOut)); m_aud = up(m_done + n_mb * sizeof(u32));
        m_win = up(m_aud + n_audit * sizeof(DevResult)); m_total = up(m_win + n_audit * sizeof(ChainWin));
    }
};

// 3. Buffers: the three allocations of the layout (kept between calls, regrown with a quarter to spare: grow, grow_pinned), the
//    chain stream, the flags cleared and a new epoch.  (No launch is running: frees are immediate.)
int chain_buffers(Ctx* c, const ChainLayout& L, uint8_t*& d_mirror)
{
    int rc_ = grow(c, c->d_chain, c->cap_chain, L.total);
    if (!rc_) rc_ = grow_pinned(c, c->h_chain, c->cap_hchain, L.out, hipHostMallocDefault);
    if (!rc_) rc_ = grow_pinned(c, c->h_mirror, c->cap_mirror, L.m_total, hipHostMallocMapped | hipHostMallocCoherent);
    if (rc_) return rc_;
    if (hipHostGetDevicePointer((void**)&d_mirror, c->h_mirror, 0) != hipSuccess) { c->set_error("hipHostGetDevicePointer failed"); return GAMDP_EHIP; }
    if (!c->chain_stream) {
        // A stream of its own priority class: the runtime multiplexes the streams of one class over a few hardware queues, and a
        // round loop whose stream shares the chain launch's queue waits for the whole launch (measured: two of ten cohorts sat
        // 27 ms behind it).  The lowest class: the launch is resident at once, the round loops' small launches go ahead of nothing.
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) { least = 0; (void)hipGetLastError(); }
        if (hipStreamCreateWithPriority(&c->chain_stream, hipStreamNonBlocking, least) != hipSuccess) { c->set_error("hipStreamCreate failed"); return GAMDP_EHIP; }
    }
    // the flags: cleared for every launch (the layout moves with the call's sizes, so what lies there may be an earlier call's
    // records), and raised to a value that changes from launch to launch
    std::memset(c->h_mirror + L.m_done, 0, L.n_mb * sizeof(u32));
    if (++c->chain_epoch == 0) c->chain_epoch = 1;
    return 0;
}

// 4. Describe: DevMB[] and DevBlk[] in the upload buffer, and which place of the launch each machine has
void describe_chains(const std::vector<Machine>& M, const ChainSel& sel, const SeqSet* ms, const SeqSet* ss, DevMB* hmb, DevBlk* hbk,
                     std::vector<u32>& q_of)
{
    q_of.assign(M.size(), ~0u);
    u32 blk_at = 0;
    for (size_t q = 0; q < sel.ch.size(); q++) {
        const Machine& m = M[sel.ch[q].mi];
        const gamdp_mb_in& in = *m.in;
        q_of[sel.ch[q].mi] = (u32)q;
        DevMB& x = hmb[q];
        x.a2 = ms->fwd[in.m_id].p2; x.an = ms->fwd[in.m_id].pn;
        x.b2 = ss->fwd[in.s_id].p2; x.bn = ss->fwd[in.s_id].pn;
        x.b2rc = ss->rc[in.s_id].p2; x.bnrc = ss->rc[in.s_id].pn;
        x.mlen = m.mlen; x.slen = m.slen;
        x.m_start = m.m_start; x.s_start = m.s_start; x.s_end = m.s_end;
        x.align_thr = m.align_thr;
        x.first_blk = blk_at; x.n_blocks = in.n_blocks; x.audit_first = 2 * blk_at;
        x.rows = (u32)std::min<u64>(sel.ch[q].rows, 0x7fffffffu);
        x.try_rev = m.try_rev ? 1u : 0u;
        x.has_n = (ms->has_n[in.m_id] || ss->has_n[in.s_id] || diag().force_n) ? 1u : 0u;
        x.npre_a = (size_t)in.m_id < ms->dev_npre.size() ? ms->dev_npre[in.m_id] : nullptr;
        x.npre_b = (size_t)in.s_id < ss->dev_npre.size() ? ss->dev_npre[in.s_id] : nullptr;
        for (u32 k = 0; k < in.n_blocks; k++) {
            const gamdp_block& b = m.blk(k);
            hbk[blk_at + k] = DevBlk{b.m_begin, b.m_end, b.s_begin, b.s_end};
        }
        blk_at += in.n_blocks;
    }
}

// 5. Slots and pieces.  Every workgroup of a kernel with slots (ChainKernel::slots) goes round its own scratch slots
//    (chain_slots_per_workgroup(): k_chain2 has a filling and two walking wavefronts per merge block), sized for the longest call
//    ITS chain can make (x_size <= its longest slave frame) -- a call of a 30 Mb genome has a few chains with frames of 100 kb
//    and two thousand with frames of a few kb.  What
//    does not fit the arena at once goes in pieces, one launch after the other over the same memory; twins only when everything
//    fits at once.  Returns false when a frame is too long for the arena: the round loop peels such calls off by itself.
struct ChainSlots {
    std::vector<std::pair<u32, u32>> pieces;   // [first, first + count) of the list, each within the arena; slot offsets are relative to the piece
    u64 need_scratch = 0, slotw_max = 0, n_tw = 0;   // u32 words; the twins that are left
    u32 ypad = 0;
};
// `ki`: the kernel_info row of the one-task kernel whose fill and walk the chain kernel runs (ChainKernel::slots).  A chain's slots are
// that kernel's slots for a task of the chain's longest frame: slot_geom (gamdp_dev.h), which also sizes the slots of a batch launch.
// nullptr: a kernel without slots -- the slot fields cleared (so that the upload does not carry what an earlier call left there), one
// piece, no twins, no scratch.
bool plan_slots(const ChainSel& sel, DevMB* hmb, const KernelInfo* ki, const u32 band, const u64 arena, ChainSlots& S)
{
    const u64 n_mb = sel.ch.size();
    if (ki == nullptr) {
        for (size_t q = 0; q < n_mb; q++) {
            DevMB& x = hmb[q];
            x.max_x = 0; x.slot_off[0] = x.slot_off[1] = 0; x.slot_words = x.dir_words = x.ckpt_off = x.bnd_off = 0;
        }
        S.pieces.emplace_back(0u, (u32)n_mb);
        return true;
    }
    const u64 per_wg = (u64)chain_slots_per_workgroup();
    const u64 arena_words = arena / sizeof(u32);
    S.n_tw = sel.n_tw;
    u64 words_all = 0, words_twins = 0;
    for (size_t q = 0; q < n_mb; q++) {
        DevMB& x = hmb[q];
        const SlotGeom g = slot_geom(*ki, dir_words_for(*ki, sel.ch[q].longest, band), band);
        S.ypad = g.ypad;
        x.max_x = sel.ch[q].longest;
        x.dir_words = g.dir_words; x.slot_words = g.slot_words;
        x.ckpt_off = g.ckpt_off; x.bnd_off = g.bnd_off;
        S.slotw_max = std::max(S.slotw_max, x.slot_words);
        words_all += per_wg * x.slot_words;
        if (q < S.n_tw) words_twins += per_wg * x.slot_words;
    }
    if (per_wg * S.slotw_max > arena_words) return false;
    if (words_all + words_twins > arena_words) S.n_tw = 0;
    u64 at = 0;
    for (size_t q = 0; q < S.n_tw; q++) { hmb[q].slot_off[1] = at; at += per_wg * hmb[q].slot_words; }   // (the twins' workgroups come first in the grid)
    u32 first = 0;
    for (size_t q = 0; q < n_mb; q++) {
        const u64 mine = per_wg * hmb[q].slot_words;
        if (at + mine > arena_words) {   // (never with twins: then everything fits)
            S.pieces.emplace_back(first, (u32)q - first);
            S.need_scratch = std::max(S.need_scratch, at);
            first = (u32)q; at = 0;
        }
        hmb[q].slot_off[0] = at;
        if (q >= S.n_tw) hmb[q].slot_off[1] = 0;
        at += mine;
    }
    S.pieces.emplace_back(first, (u32)n_mb - first);
    S.need_scratch = std::max(S.need_scratch, at);
    return true;
}

// 6. Enqueue: the kernel's parameters, what the host keeps of the launch (`run`), upload, the launches of kernel `ck`, the two events.
int enqueue_chains(Ctx* c, const ChainSel& sel, const ChainLayout& L, const ChainSlots& S, uint8_t* const dm, const u32 band,
                   const SeqSet* ms, const SeqSet* ss, const ChainKernel& ck, ChainRun& run)
{
    uint8_t *const h = c->h_chain, *const d = c->d_chain, *const hm = c->h_mirror;
    ChainParams cp;
    cp.mbs = (const DevMB*)(d + L.mb); cp.blks = (const DevBlk*)(d + L.blk); cp.n_mbs = (u32)L.n_mb;
    cp.n_twins = (u32)S.n_tw; cp.sync = (ChainSync*)(d + L.sync);
    std::memset(h + L.sync, 0, (S.n_tw + 1) * sizeof(ChainSync));
    cp.cursor = nullptr; cp.audit = (DevResult*)(d + L.aud); cp.out = (ChainOut*)(d + L.out); cp.win = (ChainWin*)(d + L.win);
    cp.scratch = c->d_chain_scratch; cp.ypad = S.ypad; cp.band = band;
    cp.max_rows = (u32)std::min<u64>(std::max<u64>(1, sel.ch[0].rows), 0x7fffffffu);
    cp.host_out = (ChainOut*)(dm + L.m_out); cp.host_done = (u32*)(dm + L.m_done); cp.host_audit = (DevResult*)(dm + L.m_aud); cp.host_win = (ChainWin*)(dm + L.m_win);
    cp.epoch = c->chain_epoch;
    cp.skew_call = diag().chain_skew;
    // N by window: the chains pick the cell of every call by the bases it touches (+ 64 on either side, as the batch path does);
    // the diagnostics build's GAMDP_DIAG_FORCE_N: by the contigs' flags, as in rounds 3-4
    cp.n_margin = (int32_t)(64 - diag().n_window_shrink); cp.n_by_contig = diag().force_n ? 1u : 0u;
    run.n_by_contig = cp.n_by_contig != 0;
    run.kernel = ck;
    run.scratch_bytes = S.need_scratch * sizeof(u32); run.n_launches = (u32)S.pieces.size(); run.n_twins = (u32)S.n_tw;
    // (the events belong to `run` from here on: every path out leaves them to it)
    if (hipEventCreate(&run.e0) != hipSuccess || hipEventCreate(&run.e1) != hipSuccess) { c->set_error("hipEventCreate failed"); return GAMDP_EHIP; }
    if (diag().timing) std::fprintf(stderr, "gamdp chain: %zu merge blocks, %llu blocks, %zu piece(s), %.1f MB of scratch (slots of up to %llu words), %llu twins, has_n %d\n", (size_t)L.n_mb, (unsigned long long)sel.n_blk, S.pieces.size(), S.need_scratch * 4e-6, (unsigned long long)S.slotw_max, (unsigned long long)S.n_tw, (int)sel.has_n);
    run.n_mb = L.n_mb; run.band = band; run.hmb = (const DevMB*)(h + L.mb); run.ms = ms; run.ss = ss;
    run.hout = (const ChainOut*)(hm + L.m_out); run.done = (const volatile u32*)(hm + L.m_done); run.haud = (const DevResult*)(hm + L.m_aud); run.hwin = (const ChainWin*)(hm + L.m_win);
    run.epoch = cp.epoch; run.stream = c->chain_stream; run.dout = cp.out;
    run.t_launch = std::chrono::steady_clock::now();
    bool ok = hipMemcpyAsync(d, h, L.out, hipMemcpyHostToDevice, c->chain_stream) == hipSuccess;
    ok = ok && hipEventRecord(run.e0, c->chain_stream) == hipSuccess;
    for (size_t pc = 0; ok && pc < S.pieces.size(); pc++) {   // (one launch unless the arena is too small for all the slots at once)
        cp.first_mb = S.pieces[pc].first;
        ok = launch_kernel(ck.kernel, ck.threads, cp, (unsigned)(S.pieces[pc].second + S.n_tw), c->chain_stream) == 0;   // (a workgroup per merge block of the piece, the twins' in front)
    }
    ok = ok && hipEventRecord(run.e1, c->chain_stream) == hipSuccess;
    if (!ok) {
        (void)hipStreamSynchronize(c->chain_stream);
        c->set_error(std::string("chain launch: ") + hipGetErrorString(hipGetLastError()));
        return GAMDP_EHIP;
    }
    run.launched = true;
    return 0;
}

// The chain kernel of a call (kernel == nullptr: none, the round loop takes every merge block).  `has_n`: a contig of the launch holds
// an N.  `rounds`: GAMDP_L1_ROUNDS=1.
// CARRY mode (Ctx::l1_chain): k_chain_c at any band the carry kernels take -- no slots, no twins, one cell.
// WALK mode: band 150 on k_chain2; with Ctx::walk_bands == GAMDP_L1_WALK_ANY_BAND every other band up to GAMDP_MAX_TUNED_BAND on
// k_chain2g<band_cols(band)>, its slots laid out for the K_GEN_* kernel of that column count.
ChainKernel pick_chain_kernel(const int l1_chain, const int walk_bands, const u32 band, const bool has_n, const bool rounds)
{
    const bool carry = l1_chain == GAMDP_L1_CHAIN_CARRY;
    const bool generic = !carry && band != 150 && walk_bands == GAMDP_L1_WALK_ANY_BAND;
    if (rounds || ((carry || generic) ? band > GAMDP_MAX_TUNED_BAND : band != 150)) return ChainKernel{};
    const int cols = band_cols(band);
    if (carry) return family_chain_kernel(chain_carry_family(), cols, nullptr, false, CHAIN_N_UNREPORTED);
    if (generic) return family_chain_kernel(chain_gen_family(), cols, &kernel_info[gen_kernel_id(cols)], true, CHAIN_N_EVERY_DP);
    return chain2_kernel(has_n);
}

// Starts the launch (asynchronous).  `arena` = bytes its scratch slots may take.  Returns 0 (run.launched says whether there is
// one: not when the call has no chain kernel, no merge block has a chain, or a frame is too long for the arena) or an error code.
int launch_main_chains(Ctx* c, std::vector<Machine>& M, const SeqSet* ms, const SeqSet* ss, const u32 band, const u64 arena, ChainRun& run)
{
    run.launched = false;
    ChainSel sel = select_chains(M, ms, ss);
    const ChainKernel ck = pick_chain_kernel(c->l1_chain, c->walk_bands, band, sel.has_n || diag().force_n, tuning().l1_rounds);
    if (!ck.kernel || sel.ch.empty()) return 0;
    if (!ck.twins) sel.n_tw = 0;
    int rc_ = ss->ensure_rc(sel.need_rc, c);
    if (rc_) return rc_;
    const ChainLayout L(sel.ch.size(), sel.n_blk, sel.n_tw);
    uint8_t* d_mirror = nullptr;
    if ((rc_ = chain_buffers(c, L, d_mirror))) return rc_;
    DevMB* const hmb = (DevMB*)(c->h_chain + L.mb);
    describe_chains(M, sel, ms, ss, hmb, (DevBlk*)(c->h_chain + L.blk), run.q_of);
    ChainSlots slots;
    if (!plan_slots(sel, hmb, ck.slots, band, arena, slots)) return 0;
    // (the slots themselves: exactly what the pieces need -- the arena is a budget, a quarter to spare would overdraw it; none for a
    // kernel without slots)
    if ((rc_ = grow(c, c->d_chain_scratch, c->cap_chain_scratch, slots.need_scratch, true))) return rc_;
    if ((rc_ = enqueue_chains(c, sel, L, slots, d_mirror, band, ms, ss, ck, run))) return rc_;
    for (const ChainPick& p : sel.ch) M[p.mi].on_device = true;
    return 0;
}

// The host's machine of merge block `mi` over the records its chain left (after run.ended()).  Every call of the chain is
// derived twice: the device left, next to each result record, the window it ran (ChainWin), the host's machine derives its own
// next call from the records so far (Machine::pending, PctgBuilder.cc:1652-1677) and runs its own pre-checks; the two must
// agree in every number -- window, orientation, rows, status -- or the call fails with GAMDP_EHIP naming the merge block and the
// call: a chain kernel that derived a different window can not hand back a plausible wrong answer.
int replay_chain(Ctx* cc, const ChainRun& run, Machine& m, const u32 mi, u64* calls_used)
{
    const u32 q = run.q_of[mi];
    const DevMB& x = run.hmb[q];
    const u32 n_dp = run.hout[q].n_dp;
    *calls_used = 0;
    if ((run.hout[q].state & 0xffu) == 3u) {   // a call did not fit the chain's scratch slots: nothing of the chain is used, the round loop takes the merge block
        m.on_device = false;
        return 0;
    }
    u32 used = 0;
    auto differs = [&](const char* what, const u64 dev, const u64 host) {
        cc->set_error("internal: merge block " + std::to_string(mi) + ", call " + std::to_string(used) + " of its chain: the device's " + what + " is " +
                      std::to_string(dev) + ", the host's " + std::to_string(host));
        return GAMDP_EHIP;
    };
    while (m.phase == Machine::MAIN) {
        if (used >= n_dp) { cc->set_error("internal: the device's chain of merge block " + std::to_string(mi) + " is shorter than the host's"); return GAMDP_EHIP; }
        ITask t;
        m.pending(t);
        u64 X = 0, cells = 0;
        const int st = preflight(m.mlen, m.slen, run.band, t.begin_a, t.end_a, t.begin_b, t.end_b, false, false, &X, &cells);
        const ChainWin& w = run.hwin[x.audit_first + used];
        const DevResult& rec = run.haud[x.audit_first + used];
        if (w.begin_a != t.begin_a) return differs("begin_a", w.begin_a, t.begin_a);
        if (w.end_a != t.end_a) return differs("end_a", w.end_a, t.end_a);
        if (w.begin_b != t.begin_b) return differs("begin_b", w.begin_b, t.begin_b);
        if (w.end_b != t.end_b) return differs("end_b", w.end_b, t.end_b);
        if ((w.info & 1u) != (t.b_rc ? 1u : 0u)) return differs("orientation", w.info & 1u, t.b_rc ? 1u : 0u);
        if ((w.info >> 8) != (u32)st) return differs("pre-check status", w.info >> 8, (u64)st);
        if (w.X != (u32)X) return differs("row count", w.X, X);
        if (run.kernel.n_bit != CHAIN_N_UNREPORTED) {   // the cell the device picked for this call: every call that runs a DP, or (N by window) the host's own answer for the same window, with the full margin
            const bool want_n = run.kernel.n_bit == CHAIN_N_EVERY_DP ? st == GAMDP_ST_OK : st == GAMDP_ST_OK && x.has_n != 0 &&
                                (run.n_by_contig || run.ms->window_has_n(t.a_id, false, 0, (int64_t)t.begin_a - (int64_t)run.band - 64, (int64_t)t.begin_a + (int64_t)X - 1 + (int64_t)run.band + 64) ||
                                 run.ss->window_has_n(t.b_id, t.b_rc, 0, (int64_t)t.begin_b - 64, (int64_t)t.begin_b + (int64_t)X - 1 + 64));
            if (((w.info >> 1) & 1u) != (want_n ? 1u : 0u)) return differs("choice of the N-aware cell", (w.info >> 1) & 1u, want_n ? 1u : 0u);
        }
        if (st != GAMDP_ST_OK && (rec.flags >> 8) != (u32)st) return differs("record status", rec.flags >> 8, (u64)st);
        gamdp_result r;
        fill_result(rec, cells, r);
        m.feed(r);
        used++;
    }
    if (used != n_dp) { cc->set_error("internal: the device's chain of merge block " + std::to_string(mi) + " is longer than the host's"); return GAMDP_EHIP; }
    *calls_used = used;
    return 0;
}

struct CohortStats {
    int rounds = 0; double pending_ms = 0, align_ms = 0, feed_ms = 0; int rc = 0;
    gamdp_l1_hits_stats hits{};   // the findHits calls of this cohort
    std::vector<gamdp_l1_tail_call> tails;   // ... and the seed each gave its tail call
    u64 chains = 0, chain_calls = 0;         // chains of the launch this cohort replayed and used, and their records (gamdp_l1_chain_stats)
};

inline auto now() { return std::chrono::steady_clock::now(); }
template <class T> double msec(T a, T b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

// A cohort with nothing to align while chains of its merge blocks (`waiting`) still run: waits a little for one of them.
enum class Wait { NOTHING, AGAIN, FAILED };   // nothing to wait for / look again / the launch failed (error set)
Wait wait_for_chain(Ctx* c, const ChainRun& run, const std::vector<u32>& waiting, bool& drained)
{
    if (waiting.empty()) return Wait::NOTHING;
    // a launch that is over without every flag up has failed (`drained`: it is known to be over; then one more look at the flags)
    if (drained) { c->set_error("internal: the chain launch ended without handing over merge block " + std::to_string(waiting[0])); return Wait::FAILED; }
    const hipError_t qs = hipStreamQuery(run.stream);
    if (qs == hipSuccess) { drained = true; return Wait::AGAIN; }
    if (qs != hipErrorNotReady) { c->set_error(std::string("chain kernel: ") + hipGetErrorString(qs)); return Wait::FAILED; }
    if (diag().timing && diag().build && std::chrono::duration<double>(now() - run.t_launch).count() > 5.0) {
        run.dump(stderr);   // diagnostics build: a watchdog instead of a blind wait
        std::_Exit(3);
    }
    for (int spin = 0; spin < 256; spin++) {
        bool any = false;
        for (u32 i : waiting) any = any || run.done[run.q_of[i]] == run.epoch;
        if (any) break;
        std::this_thread::yield();
    }
    return Wait::AGAIN;
}

// A tail alignment of a round: the findHits query that seeds it, and what the driver reads of the answer
struct TailQuery { u32 mi; Machine::Phase side; u32 task; HitsReq req; };   // the machine, LEFT or RIGHT, the call it seeds in the round's batch
struct Seed { u64 n_hits; u32 first, last; int source; };                   // source: GAMDP_L1_SEED_*
inline Seed seed_of(const std::vector<uint32_t>& hits, const int source)
{
    return Seed{hits.size(), hits.empty() ? 0 : hits.front(), hits.empty() ? 0 : hits.back(), source};
}

// Answers the round's queries.  GAMDP_L1_HITS_HOST: find_hits on the host, query by query.  GAMDP_L1_HITS_DEVICE: ONE batch of
// the hits kernels on this cohort's context and stream (find_hits_queries, summaries only); a query whose scratch does not fit
// this cohort's share of the arena (HITS_UNFIT) is answered by the host; it never fails the call.
int answer_tails(Ctx* c, const std::vector<Machine>& M, const std::vector<TailQuery>& tq, const bool device_hits, RcCache& rc_cache,
                 gamdp_l1_hits_stats& hs, std::vector<Seed>& seeds)
{
    std::vector<uint32_t> hits;
    auto on_host = [&](const TailQuery& q, const int source) {
        const auto h0 = now();
        M[q.mi].host_tail_hits(q.side, q.req, rc_cache, hits);
        hs.host_hits_ms += msec(h0, now());
        return seed_of(hits, source);
    };
    seeds.clear();
    if (tq.empty()) return 0;
    if (!device_hits) {
        for (const TailQuery& q : tq) seeds.push_back(on_host(q, GAMDP_L1_SEED_HOST));
        hs.host_queries += tq.size();
        return 0;
    }
    std::vector<HitsReq> reqs;
    for (const TailQuery& q : tq) reqs.push_back(q.req);
    std::vector<gamdp_hits_result> res(tq.size(), gamdp_hits_result{});
    std::vector<uint8_t> how(tq.size(), 0);
    u32 n_launch = 0;
    const int rc_ = find_hits_queries(c, reqs.data(), reqs.size(), res.data(), nullptr, nullptr, nullptr, how.data(), &hs.hits_kernel_ms, &n_launch);
    if (rc_) return rc_;
    hs.hits_launches += n_launch;
    for (size_t k = 0; k < tq.size(); k++) {
        if (how[k] == HITS_UNFIT) {
            seeds.push_back(on_host(tq[k], GAMDP_L1_SEED_FALLBACK));
            hs.host_fallback++;
            continue;
        }
        const bool trivial = how[k] == HITS_TRIVIAL;
        if (trivial && res[k].status != GAMDP_ST_OK) { c->set_error("internal: a tail's findHits view starts beyond its contig"); return GAMDP_EHIP; }
        seeds.push_back(Seed{res[k].n_hits, res[k].first, res[k].last, trivial ? GAMDP_L1_SEED_TRIVIAL : GAMDP_L1_SEED_DEVICE});
        if (!trivial && diag().hits_drop) seeds.back() = Seed{0, 0, 0, GAMDP_L1_SEED_DEVICE};   // diagnostics build: a wrong seed the tests must notice
        (trivial ? hs.trivial_queries : hs.device_queries)++;
    }
    return 0;
}

// The round loop over one cohort of merge blocks on one context (= one host thread + one stream): every round collects the
// pending find_alignment calls of its machines into ONE L0 batch, feeds the results back and advances the machines.  A
// machine whose main chain is on the device (ChainRun) joins once its chain has ended and been replayed; until then the
// rounds go on without it -- so the tails of the short chains are aligned while the long chains run, and a round is whatever
// became ready while the last one was in flight.  Cohorts run concurrently: while one waits for its kernel, another builds
// pending calls (findHits over contig tails, descriptor preparation) or feeds results -- host work hides behind GPU work.
//
// The tail alignments are seeded by findHits: a round describes the queries of all its machines (Machine::tail_query), has them
// answered (answer_tails: on the host or, `hits_mode` GAMDP_L1_HITS_DEVICE -- the owner context's, its helpers inherit it -- as
// one batch on the device), then builds the calls from (n_hits, first, last) (Machine::tail_task).
void run_cohort(Ctx* c, std::vector<Machine>& M, const std::vector<u32>& ids, RcCache& rc_cache, CohortStats& st, const ChainRun& run,
                const int hits_mode)
{
    std::vector<ITask> tasks;
    std::vector<u32> owner, first, waiting;
    std::vector<gamdp_result> res;
    std::vector<TailQuery> tq;
    std::vector<Seed> seeds;
    auto add_tail = [&](u32 mi, Machine::Phase side) {
        tq.push_back(TailQuery{mi, side, (u32)tasks.size(), HitsReq{}});
        M[mi].tail_query(side, tq.back().req);
        tasks.push_back(ITask{});
    };
    const bool chained = run.launched;
    if (chained)
        for (u32 i : ids)
            if (M[i].phase == Machine::MAIN && M[i].on_device) waiting.push_back(i);
    bool drained = false;   // the chain launch is known to be complete
    for (;;) {
        const auto t0 = now();
        if (!waiting.empty()) {
            size_t keep = 0;
            for (u32 i : waiting) {
                if (run.ended(run.q_of[i])) {
                    u64 calls_used = 0;
                    st.rc = replay_chain(c, run, M[i], i, &calls_used);
                    if (st.rc) return;
                    if (M[i].on_device) { st.chains++; st.chain_calls += calls_used; }
                } else waiting[keep++] = i;
            }
            waiting.resize(keep);
        }
        owner.clear();
        for (u32 i : ids)
            if (M[i].phase != Machine::DONE && !(M[i].phase == Machine::MAIN && M[i].on_device)) owner.push_back(i);
        if (owner.empty()) {   // nothing to do until a chain ends
            const Wait w = wait_for_chain(c, run, waiting, drained);
            if (w == Wait::NOTHING) break;
            if (w == Wait::FAILED) { st.rc = GAMDP_EHIP; return; }
            continue;
        }
        // one call per machine -- two for a machine whose left AND right tails are due (independent of each other)
        tasks.clear(); tq.clear();
        first.assign(owner.size(), 0);
        for (size_t q = 0; q < owner.size(); q++) {
            Machine& m = M[owner[q]];
            first[q] = (u32)tasks.size();
            if (m.phase == Machine::MAIN) { tasks.push_back(ITask{}); m.pending(tasks.back()); continue; }
            add_tail(owner[q], m.phase);
            if (m.phase == Machine::LEFT && m.right_follows_left()) add_tail(owner[q], Machine::RIGHT);
        }
        st.hits.tail_queries += tq.size();
        st.rc = answer_tails(c, M, tq, hits_mode == GAMDP_L1_HITS_DEVICE, rc_cache, st.hits, seeds);
        if (st.rc) return;
        for (size_t k = 0; k < tq.size(); k++) {
            const TailQuery& q = tq[k];
            M[q.mi].tail_task(q.side, tasks[q.task], seeds[k].n_hits, seeds[k].first, seeds[k].last);
            st.tails.push_back(gamdp_l1_tail_call{tasks[q.task].begin_a, q.mi, (uint8_t)(q.side == Machine::RIGHT), (uint8_t)seeds[k].source, {0, 0}});
        }
        const auto t1 = now();
        res.assign(tasks.size(), gamdp_result{});
        st.rc = c->align(tasks, res.data(), nullptr);
        if (st.rc) return;
        const auto t2 = now();
        for (size_t q = 0; q < owner.size(); q++) {
            Machine& m = M[owner[q]];
            const u32 cnt = (q + 1 < owner.size() ? first[q + 1] : (u32)tasks.size()) - first[q];
            m.feed(res[first[q]]);
            if (cnt == 2 && m.phase == Machine::RIGHT) m.feed(res[first[q] + 1]);   // (not RIGHT: the left call threw, the machine is done)
        }
        const auto t3 = now();
        st.pending_ms += msec(t0, t1); st.align_ms += msec(t1, t2); st.feed_ms += msec(t2, t3);
        st.rounds++;
        if (diag().timing && chained)
            std::fprintf(stderr, "gamdp cohort %p: round %d at %.2f ms after the chain launch: %zu calls of %zu machines, pending %.2f ms, align %.2f ms, %zu still on the device\n",
                         (void*)c, st.rounds, msec(run.t_launch, t0), tasks.size(), owner.size(), msec(t0, t1), msec(t1, t2), waiting.size());
    }
}

// ---- the entry point, step by step ----------------------------------------------------------------------------------------

// 1. The machines of the call (argument checks included) and the predicted cells of each
int build_machines(Ctx* c, const SeqSet* ms, const SeqSet* ss, const gamdp_mb_in* in, const size_t n, const u32 band, gamdp_mb_out* out,
                   gamdp_result* audit, const u32 audit_stride, std::vector<Machine>& M, std::vector<u64>& weight)
{
    M.assign(n, Machine{});
    weight.assign(n, 0);
    for (size_t i = 0; i < n; i++) {
        Machine& m = M[i];
        m.in = &in[i]; m.out = &out[i]; m.ms = ms; m.ss = ss; m.band = band;
        if (!ms->has_codes() || !ss->has_codes()) { c->set_error("merge blocks need sequence sets with host codes"); return GAMDP_EINVAL; }
        if (in[i].m_id < 0 || in[i].s_id < 0 || (size_t)in[i].m_id >= ms->lens.size() || (size_t)in[i].s_id >= ss->lens.size()) {
            c->set_error("merge block " + std::to_string(i) + ": contig id out of range");
            return GAMDP_EINVAL;
        }
        m.mlen = ms->lens[in[i].m_id];
        m.slen = ss->lens[in[i].s_id];
        if (audit) { m.audit = audit + i * (size_t)audit_stride; m.audit_cap = audit_stride; }
        m.init();
        for (u32 k = 0; k < in[i].n_blocks && in[i].blocks; k++)
            weight[i] += (u64)frame_len(in[i].blocks[k].s_begin, in[i].blocks[k].s_end) * (2ull * band + 1);
    }
    return 0;
}

// 2. Cohorts: host threads, each with its own context (stream, staging buffers, scratch arena) on this device; the merge
// blocks are dealt by predicted cells (LPT), so the cohorts' chains have similar depth.  A round lasts as long as its
// longest call, so smaller cohorts mean shorter rounds that overlap on the (nearly empty) GPU -- up to a point: 4 cohorts
// of >= 48 merge blocks, up to 16 from ~1 500 merge blocks on (measured on the GAGE-shaped workloads when every call went
// through this loop: 192 merge blocks 12.5 / 11.5 / 8.8 / 13.1 ms with 1 / 2 / 4 / 8 cohorts, 1 967 merge blocks 103 / 77 /
// 60 / 54 / 63 ms with 1 / 2 / 4 / 8 / 12; with the main chains on the device only the tails are left, two rounds bound by
// findHits on the host: 192 merge blocks 7.4 / 7.2 / 7.0 / 7.1 ms with 1 / 2 / 4 / 8, 1 967: 56 / 46 / 38 / 37 ms with
// 2 / 4 / 8 / 16).  GAMDP_L1_HITS_DEVICE moves those findHits calls to the device, a round's as one batch: DESIGN.md section 6
// has both modes side by side.
// GAMDP_L1_COHORTS=k (<= 16) and GAMDP_L1_COHORT_MIN=m set the cap and the floor by hand.  Results do not depend on the
// split: every machine only sees its own results.
int cohort_count(const size_t n, const Tuning& t)
{
    const size_t forced = (size_t)t.l1_cohorts, cmin = t.l1_cohort_min;
    return forced ? (int)std::max<size_t>(1, std::min<size_t>(forced, n / cmin))
                  : (int)std::max<size_t>(1, std::max(std::min<size_t>(4, n / cmin), std::min<size_t>(16, n / (4 * cmin))));
}

// 3. The K cohort contexts (the owner and its first K - 1 helpers, which exist) share the device for this call: 1/K of the owner's
// budget each, whatever was set or determined before -- or 1/2K while a chain launch runs beside them: half of the budget is for
// its scratch slots (`chain_arena`).  Every path out of the call leaves arena_div = 1 behind.
struct ArenaSplit {
    Ctx* c; int K;
    u64 chain_arena;
    void drop_chain_scratch() { if (c->d_chain_scratch) { (void)hipFree(c->d_chain_scratch); c->d_chain_scratch = nullptr; c->cap_chain_scratch = 0; } }
    void set(u32 div) { c->arena_div = div; for (int k = 1; k < K; k++) c->helpers[(size_t)k - 1]->arena_div = div; }
    ArenaSplit(Ctx* c_, int K_) : c(c_), K(K_)
    {
        set(2u * (u32)K);
        for (int k = 1; k < K; k++) {
            Ctx* h = c->helpers[(size_t)k - 1];
            h->arena_limit = c->arena_limit; h->arena_share = c->arena_share;
            h->trim_scratch();
        }
        c->trim_scratch();
        chain_arena = c->arena_limit / (2ull * (u64)(c->arena_share ? c->arena_share : 1));
        if (c->cap_chain_scratch * sizeof(u32) > chain_arena) drop_chain_scratch();
    }
    // no chain launch after all (another band, GAMDP_L1_ROUNDS=1, no main chain to run, a frame too long for the slots): the
    // round loops take the whole budget
    void no_chains() { set((u32)K); drop_chain_scratch(); }
    ~ArenaSplit() { set(1); }
};

// (see Ctx::defer_frees: on while a chain launch runs beside the K cohort contexts; what they outgrew is freed when the call is over)
struct DeferFrees {
    Ctx* c; int K;
    void set(bool on) { c->defer_frees = on; for (int k = 1; k < K; k++) c->helpers[(size_t)k - 1]->defer_frees = on; }
    ~DeferFrees() { set(false); c->flush_frees(); for (int k = 1; k < K; k++) c->helpers[(size_t)k - 1]->flush_frees(); }
};

// 5. The cohort threads: cohort k runs the round loop over ids[k] on its own context, the owner's thread takes cohort 0
void run_cohorts(Ctx* c, const int K, std::vector<Machine>& M, const std::vector<std::vector<u32>>& ids, const ChainRun& run,
                 std::vector<CohortStats>& cst, std::vector<std::vector<std::pair<float, float>>>& intervals)
{
    RcCache rc_cache;
    auto body = [&](int k) noexcept {
        Ctx* cc = k == 0 ? c : c->helpers[(size_t)k - 1];
        if (k > 0) { cc->kernel_ms = 0; cc->kernel_launches = 0; cc->ref_event = c->ref_event; }
        cc->interval_sink = &intervals[(size_t)k];
        const int rc_k = guarded(cc, [&]() -> int {
            if (hipSetDevice(cc->device) != hipSuccess) { cc->set_error("hipSetDevice failed"); return GAMDP_EHIP; }
            run_cohort(cc, M, ids[(size_t)k], rc_cache, cst[(size_t)k], run, c->l1_hits_mode);
            return 0;
        });
        if (rc_k && !cst[(size_t)k].rc) cst[(size_t)k].rc = rc_k;
        cc->interval_sink = nullptr;
        if (k > 0) cc->ref_event = nullptr;  // borrowed
    };
    Threads pool;   // joined on every path out, also when starting a later thread fails
    for (int k = 1; k < K; k++) pool.start(body, k);
    body(0);
}

// the time a set of intervals covers (sorts the list)
double union_ms(std::vector<std::pair<float, float>>& iv)
{
    std::sort(iv.begin(), iv.end());
    double sum = 0;
    float lo = 0, hi = -1;
    for (const auto& x : iv) {
        if (hi < lo) { lo = x.first; hi = x.second; }
        else if (x.first <= hi) hi = std::max(hi, x.second);
        else { sum += hi - lo; lo = x.first; hi = x.second; }
    }
    return hi >= lo ? sum + (hi - lo) : sum;
}

// 6. The statistics of the call (gamdp_ctx_l1_stats, _l1_hits_stats, _l1_tail_calls); the helpers' kernel time is accounted to
// the caller's context.  k0_ms / k0_n: the context's kernel time and launches when the call began.
void collect_stats(Ctx* c, const size_t n, const gamdp_mb_out* out, const int K, const std::vector<CohortStats>& cst,
                   const std::vector<std::vector<std::pair<float, float>>>& intervals, const bool chained, const float chain_at,
                   const float chain_ms, const double k0_ms, const u64 k0_n)
{
    gamdp_l1_stats& S = c->last_l1;
    S = gamdp_l1_stats{};
    for (int k = 1; k < K; k++) { c->kernel_ms += c->helpers[(size_t)k - 1]->kernel_ms; c->kernel_launches += c->helpers[(size_t)k - 1]->kernel_launches; }
    S.merge_blocks = n; S.cohorts = (uint32_t)K;
    for (size_t i = 0; i < n; i++) { S.dp_calls += out[i].n_dp; S.cells += out[i].cells; }
    gamdp_l1_hits_stats& H = c->last_l1_hits;
    H = gamdp_l1_hits_stats{};
    H.mode = (uint32_t)c->l1_hits_mode;
    c->last_l1_tails.clear();
    std::vector<std::pair<float, float>> all;
    for (int k = 0; k < K; k++) {
        const CohortStats& s = cst[(size_t)k];
        const gamdp_l1_hits_stats& h = s.hits;
        c->last_l1_tails.insert(c->last_l1_tails.end(), s.tails.begin(), s.tails.end());
        H.tail_queries += h.tail_queries; H.device_queries += h.device_queries; H.trivial_queries += h.trivial_queries;
        H.host_fallback += h.host_fallback; H.host_queries += h.host_queries; H.hits_launches += h.hits_launches;
        H.hits_kernel_ms += h.hits_kernel_ms; H.host_hits_ms += h.host_hits_ms;
        S.rounds = std::max<uint32_t>(S.rounds, (uint32_t)s.rounds + (chained ? 1u : 0u));
        S.host_pending_ms += s.pending_ms; S.host_feed_ms += s.feed_ms;
        all.insert(all.end(), intervals[(size_t)k].begin(), intervals[(size_t)k].end());
    }
    std::sort(c->last_l1_tails.begin(), c->last_l1_tails.end(), [](const gamdp_l1_tail_call& x, const gamdp_l1_tail_call& y) {
        return x.merge_block != y.merge_block ? x.merge_block < y.merge_block : x.right < y.right;
    });
    if (chained) all.emplace_back(chain_at, chain_at + chain_ms);
    S.launches = (uint32_t)(c->kernel_launches - k0_n);
    S.kernel_sum_ms = c->kernel_ms - k0_ms;
    S.gpu_busy_ms = union_ms(all);
}

}  // namespace
}  // namespace gamdp

extern "C" int gamdp_align_merge_blocks(gamdp_ctx* ctx, const gamdp_seqset* master, const gamdp_seqset* slave,
                                        const gamdp_mb_in* in, size_t n, uint32_t band, gamdp_mb_out* out,
                                        gamdp_result* audit, uint32_t audit_stride)
{
    if (!ctx || !master || !slave || (n && (!in || !out))) return GAMDP_EINVAL;
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    const SeqSet* ms = reinterpret_cast<const SeqSet*>(master);
    const SeqSet* ss = reinterpret_cast<const SeqSet*>(slave);
    if (band > GAMDP_MAX_BAND) { c->set_error("band exceeds GAMDP_MAX_BAND"); return GAMDP_ENOTSUP; }
    if (hipSetDevice(c->device) != hipSuccess) { c->set_error("hipSetDevice failed"); return GAMDP_EHIP; }
    return guarded(c, [&]() -> int {
        const auto t_begin = now();
        std::vector<Machine> M;
        std::vector<u64> weight;
        int rc_ = build_machines(c, ms, ss, in, n, band, out, audit, audit_stride, M, weight);
        if (rc_) return rc_;
        const double k0_ms = c->kernel_ms; const u64 k0_n = c->kernel_launches;
        const int K = cohort_count(n, tuning());
        while ((int)c->helpers.size() < K - 1) {
            Ctx* h = new (std::nothrow) Ctx();
            if (!h || h->init(c->device) != 0) { c->set_error("helper context: " + (h ? h->err : std::string("out of memory"))); delete h; return GAMDP_ENODEV; }
            c->helpers.push_back(h);
        }
        for (Ctx* h : c->helpers) copy_walk_skip_modes(h, c);   // (gamdp_ctx_set_walk_skip, _pair, _i32, _backoff: the helpers launch for this context)
        if (c->arena_budget(true) == 0) { c->set_error("hipMemGetInfo failed"); return GAMDP_EHIP; }
        ArenaSplit arena(c, K);
        std::vector<u32> part(n, 0);
        if (K > 1) partition_lpt(weight.data(), n, K, part.data());
        std::vector<std::vector<u32>> ids((size_t)K);
        for (size_t i = 0; i < n; i++) ids[part[i]].push_back((u32)i);
        // the reference point of the call's time line
        if (!c->ref_event && hipEventCreate(&c->ref_event) != hipSuccess) { c->set_error("hipEventCreate failed"); return GAMDP_EHIP; }
        if (hipEventRecord(c->ref_event, c->stream) != hipSuccess || hipEventSynchronize(c->ref_event) != hipSuccess) { c->set_error("hipEventRecord failed"); return GAMDP_EHIP; }
        // the main chains: one launch on the device, beside the round loops that take over what it hands back
        ChainRun run;
        u64 n_main = 0;   // merge blocks with a main chain to run at all
        for (const Machine& m : M) n_main += m.phase == Machine::MAIN ? 1u : 0u;
        if ((rc_ = launch_main_chains(c, M, ms, ss, band, arena.chain_arena, run))) return rc_;
        const bool chained = run.launched;
        if (!chained) arena.no_chains();
        DeferFrees defer{c, K};
        defer.set(chained);
        std::vector<std::vector<std::pair<float, float>>> intervals((size_t)K);
        std::vector<CohortStats> cst((size_t)K);
        run_cohorts(c, K, M, ids, run, cst, intervals);
        float chain_ms = 0, chain_at = 0;
        const int rc_fin = run.finish(c, &chain_at, &chain_ms);   // (also after an error in a cohort: the launch owns buffers of the context)
        for (int k = 0; k < K; k++)
            if (cst[(size_t)k].rc) {
                if (k > 0) c->set_error(c->helpers[(size_t)k - 1]->err);
                return cst[(size_t)k].rc;
            }
        if (rc_fin) return rc_fin;
        collect_stats(c, n, out, K, cst, intervals, chained, chain_at, chain_ms, k0_ms, k0_n);
        {   // gamdp_ctx_l1_chain_stats
            gamdp_l1_chain_stats& Q = c->last_l1_chain;
            Q = gamdp_l1_chain_stats{};
            Q.mode = (uint32_t)c->l1_chain;
            for (const CohortStats& s : cst) { Q.chains += s.chains; Q.chain_calls += s.chain_calls; }
            Q.round_loop_mbs = n_main - Q.chains;
            if (chained) {
                Q.scratch_bytes = run.scratch_bytes; Q.launches = run.n_launches; Q.twins = run.n_twins; Q.cols = (uint32_t)run.kernel.cols;
                std::snprintf(Q.kernel, sizeof(Q.kernel), "%s", run.kernel.name);
                Q.chain_ms = (double)chain_ms;
            }
        }
        gamdp_l1_stats& S = c->last_l1;
        S.wall_ms = msec(t_begin, now());
        if (gamdp::diag().timing)
            std::fprintf(stderr, "gamdp_align_merge_blocks: %zu merge blocks, %d cohorts, %u rounds, %u launches: wall %.2f ms, GPU busy %.2f ms (kernels %.2f ms), pending %.2f ms, feed %.2f ms\n",
                         n, K, S.rounds, S.launches, S.wall_ms, S.gpu_busy_ms, S.kernel_sum_ms, S.host_pending_ms, S.host_feed_ms);
        return 0;
    });
}


extern "C" int gamdp_ctx_set_l1_hits(gamdp_ctx* ctx, int mode)
{
    if (!ctx || (mode != GAMDP_L1_HITS_HOST && mode != GAMDP_L1_HITS_DEVICE)) return GAMDP_EINVAL;
    reinterpret_cast<Ctx*>(ctx)->l1_hits_mode = mode;
    return 0;
}

static_assert(sizeof(gamdp_l1_chain_stats) == 80 && offsetof(gamdp_l1_chain_stats, scratch_bytes) == 24 && offsetof(gamdp_l1_chain_stats, mode) == 32 &&
              offsetof(gamdp_l1_chain_stats, cols) == 44 && offsetof(gamdp_l1_chain_stats, kernel) == 48 && offsetof(gamdp_l1_chain_stats, chain_ms) == 72,
              "gamdp_l1_chain_stats: the layout include/gamdp.h documents (gam_ngs_amd/lib.py L1ChainStats mirrors it)");

extern "C" int gamdp_ctx_set_l1_chain(gamdp_ctx* ctx, int mode)
{
    if ((mode != GAMDP_L1_CHAIN_WALK && mode != GAMDP_L1_CHAIN_CARRY) || !ctx) return GAMDP_EINVAL;
    reinterpret_cast<Ctx*>(ctx)->l1_chain = mode;
    return 0;
}

extern "C" int gamdp_ctx_set_l1_walk_bands(gamdp_ctx* ctx, int which)
{
    if ((which != GAMDP_L1_WALK_BAND_150 && which != GAMDP_L1_WALK_ANY_BAND) || !ctx) return GAMDP_EINVAL;
    reinterpret_cast<Ctx*>(ctx)->walk_bands = which;
    return 0;
}

extern "C" int gamdp_ctx_l1_chain_stats(const gamdp_ctx* ctx, gamdp_l1_chain_stats* out)
{
    if (!ctx || !out) return GAMDP_EINVAL;
    *out = reinterpret_cast<const Ctx*>(ctx)->last_l1_chain;
    return 0;
}

extern "C" int gamdp_ctx_l1_hits_stats(const gamdp_ctx* ctx, gamdp_l1_hits_stats* out)
{
    if (!ctx || !out) return GAMDP_EINVAL;
    *out = reinterpret_cast<const Ctx*>(ctx)->last_l1_hits;
    return 0;
}

extern "C" int gamdp_ctx_l1_tail_calls(const gamdp_ctx* ctx, gamdp_l1_tail_call* out, size_t cap, size_t* n)
{
    if (!ctx || (cap && !out)) return GAMDP_EINVAL;
    const Ctx* c = reinterpret_cast<const Ctx*>(ctx);
    if (n) *n = c->last_l1_tails.size();
    for (size_t i = 0; i < c->last_l1_tails.size() && i < cap; i++) out[i] = c->last_l1_tails[i];
    return 0;
}

extern "C" int gamdp_ctx_l1_stats(const gamdp_ctx* ctx, gamdp_l1_stats* out)
{
    if (!ctx || !out) return GAMDP_EINVAL;
    *out = reinterpret_cast<const Ctx*>(ctx)->last_l1;
    return 0;
}
