// Host-internal types of libgamdp (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <thread>
#include <string>
#include <utility>
#include <vector>

#include "gamdp.h"
#include "gamdp_dev.h"

namespace gamdp {

constexpr int64_t FORCE_MAXGAP_ = 10;  // FORCE_MAXGAP_LEN, banded_smith_waterman.hpp:37

struct Ctx;

// Diagnostics switches (environment, read once per process: gamdp_host.cpp).  The product build reads GAMDP_DIAG_TIMING alone;
// everything else keeps its default there.
struct Diag {
    bool build = false;            // compiled with -DGAMDP_DIAG
    bool timing = false;           // GAMDP_DIAG_TIMING: host-side timing lines on stderr (results untouched)
    bool skip_traceback = false;   // GAMDP_DIAG_SKIP_TRACEBACK: no walk (results invalid)
    bool no_dirfree = false;       // GAMDP_DIAG_NO_DIRFREE: a direction per cell everywhere
    bool count_mat = false;        // GAMDP_DIAG_COUNT_MAT: n_match := number of materialise() calls (results invalid)
    bool force_n = false;          // GAMDP_DIAG_FORCE_N: N-free input through the N-aware kernels
    int64_t n_window_shrink = 0;   // GAMDP_DIAG_N_WINDOW_SHRINK=k: the N windows k bases too small on either side (fault injection)
    u32 chain_skew = ~0u;          // GAMDP_DIAG_CHAIN_SKEW=k: the device chains start call k one slave base late (fault injection)
    bool hits_drop = false;        // GAMDP_DIAG_HITS_DROP: every device findHits query of the merge-block driver reports no hits (fault injection)
};
const Diag& diag();

// The kernel families whose walks can jump over indel-free groups, one property of the C ABI each (gamdp_ctx_set_walk_skip, _pair,
// _i32): the launch flag that switches the test on, the environment variable that makes GAMDP_WALK_SKIP_DIAG the mode of new
// contexts, and the family's kernels.
enum WalkSkipFamilyId : int {
    WS_O19 = 0,   // the eight-task kernel
    WS_P17,       // the two-task kernel, both of its walk paths
    WS_I32,       // the six int32 direction-free kernels: one or four tasks per wavefront, checkpoint rows as int32 images
    WS_COUNT
};
struct WalkSkipFamily {
    u32 flag;
    const char* env;
    bool (*has)(int kid);
};
constexpr WalkSkipFamily walk_skip_families[WS_COUNT] = {
    {LP_WALK_SKIP_DIAG, "GAMDP_WALK_SKIP", [](int kid) { return kid == K_O19_CE15; }},
    {LP_WALK_SKIP_PAIR, "GAMDP_WALK_SKIP_PAIR", [](int kid) { return kid == K_P17_CE4; }},
    {LP_WALK_SKIP_I32, "GAMDP_WALK_SKIP_I32", [](int kid) { return kid == K_C17_CE4 || kid == K_C17_CE4_N || kid == K_Q19_CE15 || kid == K_Q19_CE15_N || kid == K_GEN_C9 || kid == K_GEN_C17; }},
};
// the family of a kernel, -1 for a kernel whose walks have no test
constexpr int walk_skip_family(int kid)
{
    for (int f = 0; f < WS_COUNT; f++)
        if (walk_skip_families[f].has(kid)) return f;
    return -1;
}
static_assert([] {
    for (int kid = 0; kid < K_COUNT; kid++) {
        int n = 0;
        for (int f = 0; f < WS_COUNT; f++) n += walk_skip_families[f].has(kid) ? 1 : 0;
        if (n > 1) return false;
    }
    return true;
}(), "walk_skip_families: no kernel is in two families");

// The four properties of a context: GAMDP_WALK_* per family, GAMDP_WALK_BACKOFF_* for whichever of them is on
static_assert(GAMDP_WALK_STRIPS == 0 && GAMDP_WALK_BACKOFF_OFF == 0, "WalkSkipModes: the defaults are 0");
struct WalkSkipModes {
    int family[WS_COUNT] = {};
    int backoff = 0;
};
// What a family's launches of one gamdp_align_batch counted (the LS_SKIP_* words of gamdp_dev.h, summed): what the four public
// statistics structs are filled from
struct WalkSkipCount {
    u64 tests = 0, groups_tested = 0, groups_skipped = 0, rows_skipped = 0, strips = 0;
    u64 held = 0;                                  // points passed without a test (backoff)
    u32 launches = 0, launches_side_by_side = 0;   // (side by side: the two-task kernel)
    bool ran = false;                              // the call launched a kernel of the family
    void add(const WalkSkipCount& o)
    {
        tests += o.tests; groups_tested += o.groups_tested; groups_skipped += o.groups_skipped; rows_skipped += o.rows_skipped; strips += o.strips;
        held += o.held; launches += o.launches; launches_side_by_side += o.launches_side_by_side; ran |= o.ran;
    }
};

// What the OPSRUN walks of one gamdp_align_batch / gamdp_align_batch_fp counted (the LS_OPS_* words of gamdp_dev.h, summed)
struct OpsWalkCount {
    u64 tasks = 0, ops_by_run = 0, ops_by_step = 0, runs = 0;
    void add(const OpsWalkCount& o) { tasks += o.tasks; ops_by_run += o.ops_by_run; ops_by_step += o.ops_by_step; runs += o.runs; }
};

// Product-library switches (environment, read once per process: gamdp_host.cpp).  None changes a result: each takes the planner
// to the other side of a threshold that real inputs also reach (A/B measurements, and a second way through the tests).
struct Tuning {
    bool no_merge_n = false;            // GAMDP_NO_MERGE_N (or GAMDP_QUAD_MIN set): a small batch keeps its N-free and N-aware band-150 launches apart
    long quad_min = -1;                 // GAMDP_QUAD_MIN=n: band-150 groups of n tasks or more take the multi-task kernels (-1: by the chip's wave slots)
    size_t octo_min_rows = 0;           // GAMDP_OCTO_MIN_ROWS=r (0..500 000): the eight-task kernel only for tasks of r rows or more on average
    bool no_pair = false;               // GAMDP_NO_PAIR: neither the two-task (band 512) nor the eight-task (band 150) kernel
    bool no_aux_launch = false;         // GAMDP_NO_AUX_LAUNCH: a batch's small launch after its big one instead of beside it
    u64 side_walk_rounds = 2;           // GAMDP_SIDE_WALK_ROUNDS=r (0..1 000 000): two-task launches of up to r rounds walk side by side
    bool no_packed_top = false;         // GAMDP_NO_PACKED_TOP: int32 top blocks everywhere
    bool no_packed_top_mixed = false;   // GAMDP_NO_PACKED_TOP_MIXED: int32 top blocks for wavefronts whose calls differ in begin_a or force their start
    int walk_prio = -1;                 // GAMDP_WALK_PRIO=0..3 (& 3): issue priority of the walk phase (-1: by the launch's rounds)
    bool no_prio = false;               // GAMDP_NO_PRIO: no longest-remaining-first priority
    long chunk_min = -1;                // GAMDP_CHUNK_MIN=n: batches of n calls or more go in pieces, whatever their size (-1: by the batch's shape)
    double chunk_min_rounds = -1;       // GAMDP_CHUNK_MIN_ROUNDS=r (0..1000): rounds a piece must keep the chip busy (-1: 3 or 2.5)
    size_t chunk_first_div = 8;         // GAMDP_CHUNK_FIRST_DIV=d (4..1024): the first piece is 1/d of the batch
    bool l1_rounds = false;             // GAMDP_L1_ROUNDS: every merge-block call through the round loop (no device chains)
    bool l1_no_twins = false;           // GAMDP_L1_NO_TWINS: no twin workgroups for the device chains
    int l1_cohorts = 0;                 // GAMDP_L1_COHORTS=k (1..16): cohorts of a merge-block call (0: by its size)
    size_t l1_cohort_min = 48;          // GAMDP_L1_COHORT_MIN=m (1 or more): merge blocks per cohort at least
    bool l1_device_hits = false;        // GAMDP_L1_DEVICE_HITS=1: new contexts start in GAMDP_L1_HITS_DEVICE mode (gamdp_ctx_set_l1_hits)
    bool l1_chain_carry = false;        // GAMDP_L1_CHAIN_CARRY=1: new contexts start in GAMDP_L1_CHAIN_CARRY mode (gamdp_ctx_set_l1_chain)
    bool l1_walk_any_band = false;      // GAMDP_L1_WALK_ANY_BAND=1: new contexts start with GAMDP_L1_WALK_ANY_BAND (gamdp_ctx_set_l1_walk_bands)
    int ops_walk = GAMDP_OPS_WALK_STEPS;   // GAMDP_OPS_WALK_RUNS=1: new contexts start in GAMDP_OPS_WALK_RUNS mode (gamdp_ctx_set_ops_walk)
    WalkSkipModes walk_skip;            // GAMDP_WALK_SKIP=1, _PAIR=1, _I32=1 (walk_skip_families), GAMDP_WALK_SKIP_BACKOFF=1: the modes new contexts start in
};
const Tuning& tuning();

// banded_smith_waterman.cc:90-132 on plain numbers: GAMDP_ST_OK = has to run on the GPU, else the final status
int preflight(u64 alen, u64 blen, u64 band, u64 begin_a, u64 end_a, u64 begin_b, u64 end_b, bool fs, bool fe,
              u64* X_out, u64* cells_out);

struct DevSeq {
    u32* p2;  // word holding base 0 in the 2-bit plane
    u32* pn;  // word holding base 0 in the N plane
};

// RefSequence equivalent: host codes (1 B/base, for findHits and lazy reverse complements) plus the
// packed planes resident in HBM.
struct SeqSet {
    Ctx* ctx = nullptr;
    std::vector<std::vector<uint8_t>> codes;  // empty for packed-only sets (gamdp_seqset_create_synth)
    std::vector<u64> lens;
    std::vector<uint8_t> has_n;
    // N by window: npre[i][k] = number of N among bases [0, 256 k) of sequence i, forward orientation (empty for a sequence without N)
    std::vector<std::vector<u32>> npre;
    // may bases [lo, hi] of the view (reverse complement or not, chopped by `off` bases) hold an N?  Positions outside the sequence
    // do not count; the answer is by blocks of 256 bases, i.e. "yes" a little more often than the truth.
    bool window_has_n(u32 id, bool rc, u64 off, int64_t lo, int64_t hi) const
    {
        if (!has_n[id]) return false;
        if (id >= npre.size() || npre[id].empty()) return true;   // no counts kept: the contig's flag decides
        return npre_window_has_n(npre[id].data(), (int64_t)lens[id], rc, off, lo, hi);   // (gamdp_dev.h: shared with the chain kernels)
    }
    // the same counts on the device, for the chain kernels (all sequences with N in one buffer; nullptr for a sequence without)
    u32* d_npre = nullptr;
    std::vector<const u32*> dev_npre;
    std::vector<DevSeq> fwd;
    mutable std::vector<DevSeq> rc;  // reverse complements, uploaded on first use
    mutable std::vector<u32*> rc_allocs;
    mutable std::mutex rc_mu;        // the cohort threads of one merge-block call share a set (ensure_rc)
    u32 *d2 = nullptr, *dn = nullptr;

    int upload(Ctx* ctx, const uint8_t* const* seqs, const uint64_t* lens, uint32_t n, bool ascii);
    int ensure_rc(const std::vector<u32>& ids, Ctx* use = nullptr) const;
    int upload_synth(Ctx* ctx, uint64_t first_pair, uint64_t stride_pairs, uint32_t n_pairs, uint64_t len);
    bool has_codes() const { return !codes.empty() || lens.empty(); }
    ~SeqSet();
};

// one find_alignment call with explicit sequence sets per operand (the tails of findBestAlignment
// put the slave contig in the `a` role, PctgBuilder.cc:1544-1551)
struct ITask {
    const SeqSet* sa;
    const SeqSet* sb;
    u32 a_id, b_id;
    u64 a_off, b_off;
    bool a_rc, b_rc, force_start, force_end;
    u32 band;
    u64 begin_a, end_a, begin_b, end_b;
};

// Where the tasks of a batch call come from: an array of ITask (the merge-block driver builds its own), or the caller's gamdp_task
// array read in place (round 6: taking 100 000 calls over into an ITask array first was 0.2 - 0.5 ms of the call and 13 MB of traffic).
struct TaskSrc {
    const ITask* it = nullptr;
    const gamdp_task* gt = nullptr;
    const SeqSet* sa = nullptr;
    const SeqSet* sb = nullptr;
    ITask operator[](size_t i) const
    {
        if (it) return it[i];
        const gamdp_task& t = gt[i];
        return ITask{sa, sb, t.a_id, t.b_id, t.a_off, t.b_off, t.a_rc != 0, t.b_rc != 0, t.force_start != 0, t.force_end != 0, t.band, t.begin_a, t.end_a, t.begin_b, t.end_b};
    }
};

// a validated task: device descriptor + what the launch planner needs
struct Prepared {
    DevTask dt;
    int kid;
    u64 cells;
    u64 dir_words;
};

// One launch of a batch call, as the planner lays it out (Ctx::align_plan)
struct Launch {
    int kid;
    u32 first, count;             // its tasks in the staged task list (count: padded to whole wavefronts)
    u64 slot_words, dir_words;
    u32 ypad, n_slots, dyn_lds;
    u64 ckpt_off, bnd_off;
    u32 band_max;
    u64 scratch_off = 0;          // where its slots begin in the scratch arena
    bool aux = false;             // runs beside the other launch, on aux_stream
};
// The launches of a batch call, the tasks of each (in launch order) and the padded task count of all
struct Plan {
    std::vector<Launch> launches;
    std::vector<std::vector<u32>> items;
    u64 n_host_tasks = 0;
};
struct AlignCall;   // one align() call under way (gamdp_host.cpp)
struct HitsBuffers;  // device buffers of gamdp_find_hits_batch (gamdp_hits.hip)
void hits_free(HitsBuffers* h);

struct Ctx {
    int device = -1;
    int n_cu = 0;
    u32 max_lds_per_wg = 65536;
    hipStream_t stream = nullptr;
    // A batch call's small N-aware launch runs BESIDE its big throughput launch (Ctx::align): a second stream, created on first use,
    // and the event that tells the first one when it is done
    hipStream_t aux_stream = nullptr;
    hipEvent_t aux_done = nullptr, aux_go = nullptr;
    std::string err;
    // Scratch-arena budget.  arena_limit is THE budget of this context's device as its owner sees it: what
    // gamdp_ctx_set_arena_bytes set, or -- while 0 -- 75 % of the free HBM at the first call.  It is never overwritten by
    // a call.  What one align() call may claim is arena_limit / (arena_share * arena_div): arena_share = contexts a
    // gamdp_multi handle created on this same device (set once by gamdp_multi_create), arena_div = contexts of THIS call
    // that run at the same time on the device (the two of a chunked batch, the K cohorts of a merge-block call; set by
    // the entry point for the duration of the call, which also hands the owner's budget to its helpers).
    u64 arena_limit = 0;
    bool arena_auto = true;   // arena_limit was determined from the free memory, not set by the caller
    u32 arena_share = 1, arena_div = 1;
    // The automatic budget: 75 % of (free HBM + what this context and its helper contexts hold as scratch).  Determined on first
    // use and again at every entry point of the C ABI (`refresh`): sequence sets created or destroyed between calls, reverse
    // complements uploaded on demand and other users of the device move what is free.
    u64 arena_budget(bool refresh = false);
    u64 arena_call() const { return arena_limit / ((u64)(arena_share ? arena_share : 1) * (u64)(arena_div ? arena_div : 1)); }
    void trim_scratch();  // gives back a scratch allocation larger than this call's share (before helper contexts allocate theirs)

    u32* d_scratch = nullptr; u64 cap_scratch = 0;  // in u32 words
    DevTask* d_tasks = nullptr; u64 cap_tasks = 0;
    DevResult* d_results = nullptr; u64 cap_results = 0;
    uint8_t* d_ops = nullptr; u64 cap_ops = 0;
    u32* d_cursor = nullptr;         // [cap_cursor] work-queue heads, then [cap_cursor][LS_COUNT] device-side launch statistics
    u32 cap_cursor = 0;
    // gamdp_ctx_launch_info: what the last gamdp_align_batch call launched (Ctx::align appends while log_launches is set)
    std::vector<gamdp_launch_info> launch_log;
    bool log_launches = false;
    u32 log_piece = 0;
    DevTask* h_tasks = nullptr;      // pinned staging
    DevResult* h_results = nullptr;  // pinned staging
    u64 cap_pinned = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    double kernel_ms = 0;
    u64 kernel_launches = 0;
    // merge-block calls: helper contexts on the same device (one per extra cohort thread, created on first use), the
    // reference event kernel intervals are measured against, the intervals of the current call, its statistics
    std::vector<Ctx*> helpers;
    hipEvent_t ref_event = nullptr;
    std::vector<std::pair<float, float>>* interval_sink = nullptr;
    gamdp_l1_stats last_l1{};
    // where the merge-block driver computes the findHits seeds of its tail alignments (gamdp_ctx_set_l1_hits), and what the last
    // call did there
    int l1_hits_mode = GAMDP_L1_HITS_HOST;
    gamdp_l1_hits_stats last_l1_hits{};
    std::vector<gamdp_l1_tail_call> last_l1_tails;   // gamdp_ctx_l1_tail_calls
    // which kernel runs the main chains of a merge-block call on the device (gamdp_ctx_set_l1_chain), and what the last call's
    // chain launch was
    int l1_chain = GAMDP_L1_CHAIN_WALK;
    int walk_bands = GAMDP_L1_WALK_BAND_150;   // WALK mode: the bands that have a chain kernel (gamdp_ctx_set_l1_walk_bands); CARRY ignores it
    gamdp_l1_chain_stats last_l1_chain{};
    // whether the walks of a family's kernels jump over indel-free groups (gamdp_ctx_set_walk_skip, _pair, _i32 -> the family's launch
    // flag) and back off from the test after failures (gamdp_ctx_set_walk_skip_backoff -> LP_WALK_SKIP_BACKOFF); the modes the last
    // gamdp_align_batch ran in (all 0 before the first) and what its launches counted, family by family (align_collect adds while
    // log_launches is set): gamdp_ctx_walk_skip*_stats
    WalkSkipModes walk_skip, walk_skip_ran;
    WalkSkipCount walk_skip_count[WS_COUNT];
    void reset_walk_skip_counts()   // at the start of a gamdp_align_batch
    {
        for (WalkSkipCount& n : walk_skip_count) n = WalkSkipCount{};
        walk_skip_ran = walk_skip;
    }
    // whether the walks of calls that want an edit string write it a diagonal run at a time (gamdp_ctx_set_ops_walk -> LP_OPS_WALK_RUNS
    // for every systolic launch); the mode the last gamdp_align_batch / gamdp_align_batch_fp ran in and what its launches counted
    // (align_collect adds while log_launches is set; the chunks of an _fp call add up): gamdp_ctx_ops_walk_stats
    int ops_walk = GAMDP_OPS_WALK_STEPS, ops_walk_ran = GAMDP_OPS_WALK_STEPS;
    OpsWalkCount ops_walk_count;
    void reset_ops_walk_count()   // at the start of a gamdp_align_batch / gamdp_align_batch_fp
    {
        ops_walk_count = OpsWalkCount{};
        ops_walk_ran = ops_walk;
    }
    HitsBuffers* hits = nullptr;   // gamdp_find_hits_batch, created on first use

    void set_error(const std::string& s) { err = s; }
    int init(int dev);
    // work arrays of align(), kept between calls
    std::vector<Prepared> w_prep;
    std::vector<int> w_status;
    std::vector<u64> w_key;
    std::vector<int8_t> w_kid;   // per task of the batch under way: its kernel (-1: settled by the pre-checks) ...
    std::vector<u32> w_rows;     // ... and its rows
    std::vector<std::vector<u32>> w_groups;            // the tasks of the batch under way by kernel
    std::vector<u32> w_sort_tmp; std::vector<size_t> w_sort_count;   // scratch of the planner's sort
    Plan w_plan;                                       // the launches of the batch under way

    // buffers of the merge-block chain kernel (gamdp_l1.cpp), kept between calls
    uint8_t* d_chain = nullptr; u64 cap_chain = 0;    // device, bytes: laid out by ChainLayout (gamdp_l1.cpp)
    uint8_t* h_chain = nullptr; u64 cap_hchain = 0;   // pinned: the part of it that is uploaded
    // the chain launch runs beside the round loop's launches: own stream, own scratch slots, and a pinned coherent mirror
    // (ChainLayout's second half) the chains write when they end
    hipStream_t chain_stream = nullptr;
    // hipFree / hipHostFree wait for the whole device; while the chain launch runs, a round loop that regrows a buffer keeps
    // the old one until the call is over (flush_frees) instead of waiting for the launch to end
    bool defer_frees = false;
    std::vector<void*> deferred_dev, deferred_host;
    void free_dev(void* p) { if (!p) return; if (defer_frees) deferred_dev.push_back(p); else (void)hipFree(p); }
    void free_host(void* p) { if (!p) return; if (defer_frees) deferred_host.push_back(p); else (void)hipHostFree(p); }
    void flush_frees()
    {
        for (void* p : deferred_dev) (void)hipFree(p);
        for (void* p : deferred_host) (void)hipHostFree(p);
        deferred_dev.clear(); deferred_host.clear();
    }
    u32* d_chain_scratch = nullptr; u64 cap_chain_scratch = 0;   // u32 words
    uint8_t* h_mirror = nullptr; u64 cap_mirror = 0;
    u32 chain_epoch = 0;

    // resident_caps (gamdp_align_batch_fp): an edit string for every task, left in d_ops in traceback order, task i in a room of
    // resident_caps[i] bytes (a multiple of 16) behind the rooms of the tasks before it; nothing of them is downloaded
    int align(const TaskSrc& tasks, size_t n, gamdp_result* out, const gamdp_ops* ops, const u64* resident_caps = nullptr);
    // the steps of align(), in the order they run (gamdp_host.cpp)
    int align_check(const TaskSrc& tasks, size_t n);
    void align_prepare(AlignCall& a);
    void align_group(AlignCall& a);
    int align_plan(u64 arena_call);
    int align_stage(const AlignCall& a);
    int align_scratch(u64 arena_call);
    int align_run(AlignCall& a);
    void align_collect(AlignCall& a);
    int grow_staging(u64 base);   // h_tasks / h_results
    // gamdp_score_batch (gamdp_host.cpp; the kernel: gamdp_score.hip), and what its last call launched (gamdp_ctx_score_info)
    std::vector<gamdp_score_launch_info> score_log;
    // gamdp_carry_batch (the kernel: gamdp_carry.hip), and what its last call launched (gamdp_ctx_carry_info)
    std::vector<gamdp_score_launch_info> carry_log;
    // gamdp_carry_ops_batch (the kernel: gamdp_carry_ops.hip), and what its last call launched (gamdp_ctx_carry_ops_info)
    std::vector<gamdp_score_launch_info> carry_ops_log;
    u32* d_ops_fp = nullptr; u64 cap_ops_fp = 0;   // its fingerprints, one per task of the batch
    // gamdp_align_batch_fp / gamdp_ops_fingerprint_batch (the kernel: gamdp_ops_fp.hip): fingerprints of strings that lie in d_ops, a
    // batch in chunks of at most ops_chunk() bytes of d_ops (gamdp_ctx_set_ops_chunk_bytes), and what the last call of either did
    u64 ops_chunk_bytes = 0;   // 0: the default
    u64 ops_chunk() const { return ops_chunk_bytes ? std::min<u64>(ops_chunk_bytes, 1ull << 40) : (1ull << 30); }
    OpsFpTask* d_fp_tasks = nullptr; u64 cap_fp_tasks = 0;
    u32* d_fp_segs = nullptr; u64 cap_fp_segs = 0;
    gamdp_ops_fp_info last_ops_fp{};
    int align_fp(const gamdp_task* tasks, const SeqSet* sa, const SeqSet* sb, size_t n, gamdp_result* out, u32* ops_fp);
    int strings_fp(const uint8_t* ops, const u64* off, const u64* len, size_t n, u32* fp);
    // one launch of k_ops_fp<forward> over `tasks` (strings in d_ops; seg_first as OpsFpParams) and the download of fp[0 .. n_fp)
    int ops_fp_launch(bool forward, const std::vector<OpsFpTask>& tasks, const std::vector<u32>& seg_first, size_t n_fp, u32* fp);
    // what the three share (gamdp_host.cpp): K is the call's traits, which name its log; ops_fp: the caller's fingerprint array of a
    // call that has one
    template <class K> int fill_only(const TaskSrc& tasks, size_t n, typename K::Out* out, u32* ops_fp = nullptr);
    int align(const ITask* tasks, size_t n, gamdp_result* out, const gamdp_ops* ops) { TaskSrc s; s.it = tasks; return align(s, n, out, ops); }
    int align(const std::vector<ITask>& tasks, gamdp_result* out, const gamdp_ops* ops) { return align(tasks.data(), tasks.size(), out, ops); }
    ~Ctx();
};
// a helper context launches for its owner: in the owner's modes, its counts from zero
inline void copy_walk_skip_modes(Ctx* to, const Ctx* from)
{
    to->walk_skip = from->walk_skip;
    to->reset_walk_skip_counts();
    to->ops_walk = from->ops_walk;   // (gamdp_ctx_set_ops_walk)
    to->reset_ops_walk_count();
}

// what gamdp_fasta points to: the host-side RefSequence (names + 1 B/base codes), no GPU involved
struct Fasta {
    std::vector<std::string> names;
    std::vector<std::vector<uint8_t>> codes;
    std::string err;
};

// Nothing may leave the C ABI as a C++ exception (the host program would std::terminate inside gam-merge instead of
// falling back to its CPU path): the bodies of the entry points that allocate or start threads run under guarded(),
// host threads are kept in a Threads object (joined on every path out), and thread bodies catch for themselves.
template <class F>
int guarded(Ctx* c, F&& f) noexcept
{
    auto note = [&](const char* what) noexcept { try { if (c) c->set_error(what); } catch (...) {} };
    try { return f(); }
    catch (const std::bad_alloc&) { note("out of host memory"); return GAMDP_ENOMEM; }
    catch (const std::exception& e) { try { if (c) c->set_error(std::string("host exception: ") + e.what()); } catch (...) {} return GAMDP_EHIP; }
    catch (...) { note("unknown host exception"); return GAMDP_EHIP; }
}
template <class F>
int guarded_thread_body(F&& f) noexcept   // the return code of a thread body that must not throw
{
    try { return f(); }
    catch (const std::bad_alloc&) { return GAMDP_ENOMEM; }
    catch (...) { return GAMDP_EHIP; }
}
struct Threads {
    std::vector<std::thread> th;
    template <class... A> void start(A&&... a) { th.emplace_back(std::forward<A>(a)...); }
    void join() { for (auto& t : th) if (t.joinable()) t.join(); }
    ~Threads() { join(); }
};

// Regrows a device buffer that is kept between calls: `need` elements or more, with a quarter to spare (`exact`: none), or just
// `need` when that much can not be had.  The old buffer goes through Ctx::free_dev: beside a chain launch it waits for the end of
// the call, and a round loop there asks for twice the size instead (see the scratch arena in Ctx::align).
template <class T>
int grow(Ctx* ctx, T*& ptr, u64& cap, u64 need, bool exact = false)
{
    if (need <= cap) return 0;
    if (ptr) { ctx->free_dev(ptr); ptr = nullptr; cap = 0; }
    u64 want = exact ? need : need + (ctx->defer_frees ? need + 1024 : need / 4);
    if (hipMalloc(&ptr, want * sizeof(T)) != hipSuccess) {
        if (hipMalloc(&ptr, need * sizeof(T)) != hipSuccess) {
            ctx->set_error("hipMalloc of " + std::to_string(need * sizeof(T)) + " bytes failed");
            return GAMDP_ENOMEM;
        }
        want = need;
    }
    cap = want;
    return 0;
}

// ... and a pinned one, in bytes (no second try: the merge-block driver's upload buffer and mirror are small)
inline int grow_pinned(Ctx* ctx, uint8_t*& ptr, u64& cap, u64 need, unsigned flags)
{
    if (need <= cap) return 0;
    if (ptr) { ctx->free_host(ptr); ptr = nullptr; cap = 0; }
    const u64 want = need + need / 4;
    if (hipHostMalloc(&ptr, want, flags) != hipSuccess) {
        ptr = nullptr;
        ctx->set_error("hipHostMalloc of " + std::to_string(want) + " bytes failed");
        return GAMDP_ENOMEM;
    }
    cap = want;
    return 0;
}

// Launches a kernel that takes its parameters as one struct, by value: `grid` workgroups of `threads` on `stream`, no dynamic LDS.
// Returns hipError_t as int.
template <class P>
int launch_kernel(const void* kernel, unsigned threads, const P& p, unsigned grid, void* stream)
{
    P copy = p;
    void* args[] = {&copy};
    return (int)hipLaunchKernel(kernel, dim3(grid), dim3(threads), args, 0, static_cast<hipStream_t>(stream));
}
// resident workgroups per CU of a family's instantiation, from the occupancy the runtime reports (4 if it does not say)
inline int family_waves_per_cu(const KernelFamily& f, int cols)
{
    int n = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, f.kernel[cols_index(cols)], (int)f.threads, 0);
    return (e == hipSuccess && n > 0) ? n : 4;
}

// DevResult record + the cell count of its call -> the C ABI's result (gamdp_host.cpp)
void fill_result(const DevResult& r, u64 cells, gamdp_result& o);

// deterministic longest-processing-time-first partition (gamdp_multi.cpp)
void partition_lpt(const u64* weights, size_t n, int parts, u32* part_of);

// ABlast::findHits (ablast.cc:41-76) on the device with the sequence sets given query by query, as ITask carries them
// (gamdp_hits.hip).  gamdp_find_hits_batch is this with one pair of sets; the merge-block driver mixes queries whose `a` is the
// slave with queries whose `a` is the master.  how == nullptr: a query that does not fit the arena fails the call (GAMDP_ENOMEM);
// otherwise how[i] says what became of query i and a query that does not fit is left to the caller.  No arena refresh, no
// hipSetDevice: the entry points do that.
struct HitsReq {
    const SeqSet *sa, *sb;
    gamdp_hits_task t;
};
enum HitsHow : uint8_t { HITS_DEVICE = 0, HITS_TRIVIAL = 1, HITS_UNFIT = 2 };   // ran on the device / no work after the clamps / too big
int find_hits_queries(Ctx* c, const HitsReq* q, size_t n, gamdp_hits_result* out, uint32_t* hits_buf, const uint64_t* hits_off,
                      const uint64_t* hits_cap, uint8_t* how, double* kernel_ms = nullptr, u32* launches = nullptr);

// ABlast::findHits (ablast.cc:41-76) on code arrays
void find_hits(const uint8_t* a, u64 alen, u64 a_start, u64 a_end, const uint8_t* b, u64 blen, u64 b_start, u64 b_end,
               u64 word, std::vector<uint32_t>& hits);

}  // namespace gamdp
