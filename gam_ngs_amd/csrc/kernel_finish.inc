// Part of gamdp_kernel.hip (included inside namespace gamdp::{anonymous}): end-cell search and traceback walk.

// ---- phases C + D: end-cell search and traceback ------------------------------------------------------
// Kept out of line (like the slow block) so that its registers -- and the scalar registers holding its many
// compare masks -- are allocated separately from the hot fill loop.
// Four tasks per wavefront: called once per task with lane_base = 16 * (task's position in the wavefront) and *tp holding
// that task's values in every lane; the whole wavefront works on one task at a time here, exactly as with one task per
// wavefront -- only the lanes that own the direction words / strips are offset by lane_base.
// Two tasks per wavefront in packed f16 (PK): the strips' inputs are the packed stores, pk_half_ = which task of the pair.
// What the end-cell search hands to the walk, and what a walk that stops early hands to the one that finishes it (the
// walk of several tasks at once, kernel_walk.inc, leaves the steps the reference treats specially to finish_walk).
// The mailbox of a chain workgroup (k_chain2, gamdp_kernel.hip): wavefront 0 fills call after call, CH_NW walker wavefronts find
// the end cells and walk, CH_NS = CH_NW + 1 scratch slots go round.  The next call's window only needs the LAST match of this call
// -- the first match the walk meets, a few steps from the end cell -- so a walk posts it at once (`early`) and the fill of the next
// call runs beside the rest of the walk; and the walks of different calls do not need each other at all, so a chain whose walks
// are slower than its fills (alignments of unrelated sequence: both orientations of a merge block that fails) has several going.
// Counters only grow; the data behind a counter is written before it (workgroup-scope release).
constexpr int CH_NW = 2, CH_NS = CH_NW + 1;
struct ChainMail {
    int filled, quit, total;         // calls handed to the walkers so far; quit: no more calls, `total` were handed over in all
    int claim;                       // next call a free walker takes
    int n_done;                      // walks that have ended
    int early_of[CH_NS], done_of[CH_NS];                  // per slot: 1 + the index of the call whose early answer / whose record is there
    int e_flags[CH_NS], e_last_a[CH_NS], e_last_b[CH_NS]; // the early answer: DevResult::flags, last_a, last_b as the call's record will have them
    int bad;                         // is_good(vector) so far in this attempt: a call that was empty or below 95 % homology
    unsigned long long sum;          // ... and the sum of the alignment lengths
    Tk tk[CH_NS];                    // the call in each scratch slot, as the fill left it
    DevTask dt[CH_NS];
};
__shared__ ChainMail s_mail;
__device__ __forceinline__ int mail_load(int* p) { return __builtin_amdgcn_readfirstlane(__hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP)); }
__device__ __forceinline__ void mail_wait_ge(int* p, const int v) { while (mail_load(p) < v) __builtin_amdgcn_s_sleep(1); }
__device__ __forceinline__ void mail_post(int* p, const int v, const int lane)
{   // (every lane's stores before it are out: the counter is written by lane 0 after the wavefront's waitcnt)
    __builtin_amdgcn_s_waitcnt(0);
    if (lane == 0) __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// whether a task's walk is the OPSRUN instance of finish_walk: the launch's flag and the task's own
__device__ __forceinline__ bool ops_walk_runs(const LaunchParams* pp, const DevTask* dtp)
{
    return (uni((int)pp->flags) & (int)LP_OPS_WALK_RUNS) != 0 && (uni((int)dtp->flags) & (int)TF_LIVE_MASK & (int)TF_WANT_OPS) != 0;
}
// a 64-bit statistics counter in two 32-bit words (the statistics words carry no 8-byte alignment): the carry goes to the high word
__device__ __forceinline__ void stat_add64(u32* lo, const u32 v)
{
    if (v == 0u) return;
    const u32 old = atomicAdd(lo, v);
    if (old + v < old) atomicAdd(lo + 1, 1u);
}

struct WalkCarry {
    int early_seq;                // chain walkers only (finish_walk<..., EARLY>): 1 + the index of this call among the chain's calls
    int status;                   // 0 no end cell (empty alignment), 1 end cell outside a (the reference throws), 2 walk from (x, y, pos)
    int best;                     // score of the end cell
    int x, y, pos, end_pos, end_x;
    u32 len, nm;                  // steps / matches so far
    int la, lb, fa, fb, have;     // last / first match seen so far (have: bit 0 first, bit 1 last)
    int mat_q, mat_lo, mat_hi, old_q, old_lo, old_hi, mat_calls;  // strips whose directions / values exist (see finish_walk)
    int need_q, need_ghi;         // walk_many of the eight-task kernel: the strip this task's walk waits for, down from group need_ghi (the caller makes it)
    int mat_ticks;                // diagnostics (GAMDP_DIAG_COUNT_MAT): 10 ns ticks inside materialise()
};

// ---- phase C: end cell (:174-212), first maximum in scan order wins --------------------------------
template <int C, bool WG2 = false>
__device__ __noinline__ void end_cell(const Tk* tp, const int lane, WalkCarry* wc)
{
    const Tk t = load_uniform(tp);
    const int X = t.X, Y = t.Y, w = t.band;
    if constexpr (!WG2) __syncthreads();   // (WG2: a workgroup of two wavefronts that do different things -- no barriers)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // drop L1 lines cached by the slot's previous task

    int best = NEG, bkey = 0x7fffffff;  // key = scan position
    {
        const giptr lr = (X == 1) ? t.h0row : t.lastrow;
        if (!t.fe) {
            for (int j = lane; j < Y; j += 64) {
                const int64_t pos = (int64_t)t.begin_a + (X - 1) + j - w;
                if (pos >= 0 && pos <= t.end_a) {
                    const int v = (pos < t.alen) ? lr[j] : 0;  // cells outside a keep their zero
                    if (v > best || (v == best && j < bkey)) { best = v; bkey = j; }
                }
            }
        }
        // anti-diagonal pos == end_a: cells (iA + k, jA - k)
        const bool ge = t.end_a >= (int64_t)t.begin_a + w;
        const int64_t jA64 = ge ? (int64_t)2 * w : (int64_t)2 * w - ((int64_t)t.begin_a + w - t.end_a);
        if (jA64 >= 0 && t.iA < X) {
            const int jA = (int)jA64;
            const int cnt = min(X - t.iA, jA + 1);
            for (int k = lane; k < cnt; k += 64) {
                const int i = t.iA + k, j = jA - k;
                bool ok = true;
                if (t.fe) ok = (X >= FORCE_MAXGAP + 1) && (i >= X - 1 - FORCE_MAXGAP);  // unsigned compare in the reference
                if (ok) {
                    int v = 0;
                    if (t.end_a < t.alen) v = (i == 0) ? t.h0row[j] : ((i == X - 1) ? lr[j] : t.adh[k]);
                    const int key = Y + k;
                    if (v > best || (v == best && key < bkey)) { best = v; bkey = key; }
                }
            }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const int ov = __shfl_xor(best, o, 64), ok = __shfl_xor(bkey, o, 64);
            if (ov > best || (ov == best && ok < bkey)) { best = ov; bkey = ok; }
        }
    }
    // after the wave reduction every lane holds the same (best, bkey)
    best = __builtin_amdgcn_readfirstlane(best);
    bkey = __builtin_amdgcn_readfirstlane(bkey);
    WalkCarry r;
    r.early_seq = 0;
    r.status = 0; r.best = best;
    r.x = r.y = r.pos = r.end_pos = r.end_x = 0;
    r.len = r.nm = 0;
    r.la = r.lb = r.fa = r.fb = r.have = 0;
    r.mat_q = -1; r.mat_lo = 0; r.mat_hi = -1; r.old_q = -1; r.old_lo = 0; r.old_hi = -1; r.mat_calls = 0; r.mat_ticks = 0;
    r.need_q = 0; r.need_ghi = 0;
    if (bkey != 0x7fffffff) {
        int x, y;
        if (bkey < Y) { x = X - 1; y = bkey; }
        else {
            const bool ge = t.end_a >= (int64_t)t.begin_a + w;
            const int jA = ge ? 2 * w : (int)((int64_t)2 * w - ((int64_t)t.begin_a + w - t.end_a));
            x = t.iA + (bkey - Y);
            y = jA - (bkey - Y);
        }
        const int64_t pos64 = (int64_t)t.begin_a + x + y - w;
        if (pos64 >= t.alen) r.status = 1;  // reference: a.at(pos) throws in the traceback
        else { r.status = 2; r.x = x; r.y = y; r.pos = (int)pos64; r.end_pos = (int)pos64; r.end_x = x; }
    }
    *wc = r;
}

// ---- phase D: traceback (:217-311), from the state in *wc to the result record -----------------------------------
// Kept out of line (like the slow block) so that its registers -- and the scalar registers holding its many
// compare masks -- are allocated separately from the hot fill loop.
// Four tasks per wavefront: called once per task with lane_base = 16 * (task's position in the wavefront) and *tp holding
// that task's values in every lane; the whole wavefront works on one task at a time here, exactly as with one task per
// wavefront -- only the lanes that own the direction words / strips are offset by lane_base.
// Two tasks per wavefront in packed f16 (PK): the strips' inputs are the packed stores, pk_half_ = which task of the pair.
// SKIP (a second instance, the default one holds none of it): the diagonal test of walk_many<..., SKIP> (kernel_walk.inc has the
// argument) for the walk that has the whole wavefront: before a block without directions costs a strip, lane k tests the k-th
// span below the walk and the walk jumps over the passing prefix.  Two formats of checkpoint row: the two-task kernel's patterns
// (PK, LP_WALK_SKIP_PAIR) and the int32 images of every other direction-free kernel (LP_WALK_SKIP_I32: k_align and k_align_q,
// N-aware or not, LPT == 64 or one DPP row per task).
// OPSRUN (a third instance, the default one holds none of it; LP_OPS_WALK_RUNS, taken per task by the ones with TF_WANT_OPS): the edit
// string a diagonal run at a time.  Interior cells take the run consumer like a task without a string, and the lanes that compared the
// run's bases write its ops: lane da + j owns steps 16 j .. 16 j + 15 from the top of the run (chunk j of the packed windows), the op
// of a step is its bit of `eq` -- MATCH where set (an N on either side too), MISMATCH where not.  Row 0, pos == 0 and the gap steps
// stay single steps.  It never makes the diagonal test and the chain walkers stay without it.
template <bool PK> struct SkipIdx { typedef int64_t T; };   // a base index of the test's loads (the two-task instance keeps its 32-bit ones)
template <> struct SkipIdx<true> { typedef int T; };
template <int C, int CE, bool HASN, int LPT = 64, bool PK = false, bool EARLY = false, bool SKIP = false, bool OPSRUN = false>
__device__ __noinline__ void finish_walk(const Tk* tp, const DevTask* dtp_, const LaunchParams* pp, const int lane, const int lane_base_, const int pk_half_, WalkCarry* wcp)
{
    const int lane_base = (LPT == 64) ? 0 : uni(lane_base_);
    const int pk_half = PK ? uni(pk_half_) : 0;
    typedef Strip<LPT, PK> ST;
    static_assert(!SKIP || (!EARLY && DIRFREE_OK<CE, C, HASN>), "the diagonal test reads checkpoint rows; the chain walkers stay without it");
    static_assert(!SKIP || (PK ? (LPT == 64 && !HASN) : (LPT == 64 || LPT == QL)), "the diagonal test knows the two-task kernel's checkpoint rows (PairFmt<C, 64>) and the int32 images of the one- and four-task kernels");
    static_assert(!OPSRUN || !EARLY, "the chain walkers write their edit strings a step at a time");
    static_assert(!OPSRUN || !SKIP, "a task that wants an edit string never makes the diagonal test");
    const Tk t = load_uniform(tp);
    const DevTask* dtp = unip(dtp_);
    const u32 dt_flags = (u32)uni((int)dtp->flags) & TF_LIVE_MASK, dt_res_idx = (u32)uni((int)dtp->res_idx);
    const u64 dt_ops_off = (u64)uni64((int64_t)dtp->ops_off), dt_ops_cap = (u64)uni64((int64_t)dtp->ops_cap);
    uint8_t* const p_ops_buf = unip(pp->ops_buf);
    DevResult* const p_results = unip(pp->results);
    const int Y = t.Y;
    const int wc_status = uni(wcp->status), best = uni(wcp->best);

    DevResult res;
    res.begin_a = res.begin_b = res.score = 0;
    res.n_match = res.length = 0;
    res.first_a = res.first_b = res.last_a = res.last_b = 0;
    res.flags = ST_EMPTY << 8;
    // EARLY (the walker of a chain workgroup): the call's last match goes to the mailbox the moment the walk meets it
    bool posted = false;
    const int early_seq = EARLY ? uni(wcp->early_seq) : 0;
    auto post_early = [&](const u32 flags, const int a, const int b) {
        if constexpr (EARLY) {
            if (!posted) {
                posted = true;
                const int sl = (early_seq - 1) % CH_NS;
                if (lane == 0) { s_mail.e_flags[sl] = (int)flags; s_mail.e_last_a[sl] = a; s_mail.e_last_b[sl] = b; }
                mail_post(&s_mail.early_of[sl], early_seq, lane);
            }
        }
    };
    if (wc_status != 0) {
        if (wc_status == 1) {
            res.flags = ST_OUT_OF_RANGE << 8;  // reference: a.at(pos) throws in the traceback
        } else {
            int x = uni(wcp->x), y = uni(wcp->y), pos = uni(wcp->pos);
            const int end_pos = uni(wcp->end_pos), end_x = uni(wcp->end_x);
            const bool want_ops = dt_flags & TF_WANT_OPS;
            uint8_t* ops = p_ops_buf + dt_ops_off;
            u32 len = (u32)uni((int)wcp->len), nm = (u32)uni((int)wcp->nm);
            const int have0 = uni(wcp->have);
            bool have_last = have0 & 2, have_first = have0 & 1;
            int la = uni(wcp->la), lb = uni(wcp->lb), fa = uni(wcp->fa), fb = uni(wcp->fb);
            int l = y / C, c = y - l * C;
            // Direction-word cache for the walk: lane k (< TB_DEPTH) holds, for block (cblk0 - k), the 4-column
            // group `cg` of lane-row `cl`.  A diagonal run stays in one (lane-row, column) and walks down the
            // blocks, a gap moves one column sideways (3 times out of 4 inside the same group), so one refill
            // (one 16 B load per lane, all in flight together) serves several dependent steps of the walk.
            constexpr int TB_DEPTH = 16;
            int cblk0 = -1, cl = -1, cg = -1;
            u32 cw = 0;  // lane 4*k + e holds the direction word of block (cblk0 - k), column 4*cg + e
            // Packed-sequence window for the match counting: lane k holds 2-bit word (w0 - k); the walk moves towards
            // lower indices, so one refill (one coalesced 256 B load) covers the next ~1000 bases.
            int64_t sa_w0 = INT64_MIN, sb_w0 = INT64_MIN, san_w0 = INT64_MIN, sbn_w0 = INT64_MIN;
            u32 sa_v = 0, sb_v = 0, san_v = 0, sbn_v = 0;  // (the N-plane windows only exist in the N-aware kernels)
            // strip of direction-free blocks whose directions materialise() has produced: the lanes of strip mat_q (Strip::first_of, width_of), blocks
            // mat_lo .. mat_hi
            int mat_q = uni(wcp->mat_q), mat_lo = uni(wcp->mat_lo), mat_hi = uni(wcp->mat_hi), mat_calls = uni(wcp->mat_calls);
            int old_q = uni(wcp->old_q), old_lo = uni(wcp->old_lo), old_hi = uni(wcp->old_hi);  // the strip materialised before that one
            long long mat_ticks = 0;
            int dg_iters = 0, dg_refills = 0;
            const long long walk_t0 = (dt_flags & TF_DIAG_COUNT_MAT) ? wall_clock64() : 0;
            int cvalid_lo = 0;  // cached blocks below this one are not usable (direction-free, not materialised)
            // SKIP: a test that found no passing span is not repeated before the walk has its strip (sk_fail_at = mat_calls then);
            // what this walk counted (LS_SKIP_*).  Diagnostics that count strips keep their strips.
            [[maybe_unused]] int sk_fail_at = -1;
            [[maybe_unused]] const bool sk_on = !(dt_flags & TF_DIAG_COUNT_MAT);
            [[maybe_unused]] u32 sk_tests = 0, sk_tested = 0, sk_groups = 0, sk_short = 0, sk_held = 0;
            // LP_WALK_SKIP_BACKOFF (gamdp_dev.h has the rule): tests in a row that skipped nothing, and the candidate points that still pass
            // without a test.  A walk that walk_many began goes on from what that left in the carry (0 | 0 from end_cell else).
            [[maybe_unused]] const bool backoff = SKIP && (uni((int)pp->flags) & (int)LP_WALK_SKIP_BACKOFF) != 0;
            [[maybe_unused]] u32 bo_fails = 0, bo_hold = 0;
            // OPSRUN: what this walk counted (LS_OPS_*): the ops its run iterations wrote and how many of those wrote any
            [[maybe_unused]] u32 or_ops = 0, or_runs = 0;
            [[maybe_unused]] const u32 or_len0 = len;
            if constexpr (SKIP) {
                const u32 bo0 = (u32)uni(wcp->early_seq);
                bo_fails = bo0 & 63u; bo_hold = bo0 >> WALK_BACKOFF_HOLD_SHIFT;
            }
            auto get_word = [&](const int blk, const int l_, const int c_) -> u32 {
                const int g = c_ >> 2;
                int k = cblk0 - blk;
                if (l_ != cl || g != cg || k < 0 || k >= TB_DEPTH || blk < cvalid_lo) {
                    cvalid_lo = 0;
                    dg_refills++;
                    if constexpr (DIRFREE_OK<CE, C, HASN>) {
                        if (blk >= t.df_hi) {
                            cvalid_lo = t.df_hi;  // the refill may reach down into direction-free blocks: not usable
                        } else if (blk >= t.df_lo) {
                            if (ST::strip_of(lane_base + l_, t.sshift) == old_q && blk >= old_lo && blk <= old_hi) {
                                // back in the strip the walk came from (a path sitting on a strip border): its words
                                // are still in memory
                                const int tq = mat_q, tl = mat_lo, th = mat_hi;
                                mat_q = old_q; mat_lo = old_lo; mat_hi = old_hi;
                                old_q = tq; old_lo = tl; old_hi = th;
                            } else if (!(ST::strip_of(lane_base + l_, t.sshift) == mat_q && blk >= mat_lo && blk <= mat_hi)) {
                                const int g_hi = blk >> 2;
                                const long long tm0 = (dt_flags & TF_DIAG_COUNT_MAT) ? wall_clock64() : 0;
                                materialise_auto<C, (DIRFREE_OK<CE, C, HASN> ? CE : 0), HASN, LPT, PK>(tp, ST::strip_of(lane_base + l_, t.sshift), g_hi, lane, pk_half, lane_base);
                                if (dt_flags & TF_DIAG_COUNT_MAT) mat_ticks += wall_clock64() - tm0;
                                // the loads below must see those stores: wait until L2 has them, then drop this CU's L1
                                // lines (an agent-scope release would write back the whole L2 of the XCD, far too much)
                                __builtin_amdgcn_s_waitcnt(0);
                                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                                old_q = mat_q; old_lo = mat_lo; old_hi = mat_hi;
                                mat_q = ST::strip_of(lane_base + l_, t.sshift); mat_hi = 4 * g_hi + 3; mat_lo = max(4 * (g_hi - (ST::groups_of(mat_q) - 1)), t.df_lo);
                                mat_calls++;
                            }
                            cvalid_lo = (mat_lo == t.df_lo) ? 0 : mat_lo;  // below df_lo the tagged blocks are all there
                        }
                    }
                    cblk0 = blk; cl = l_; cg = g; k = 0;
                    // one coalesced load: each group of 4 lanes reads the 16 B of one block.  No lane-dependent branch
                    // (it would make the compiler treat the whole walk as divergent): blocks below 0 and columns past
                    // the lane's last one just re-read a valid word
                    const int myblk = max(blk - (lane >> 2), 0);
                    const int myc = min(4 * g + (lane & 3), C - 1);
                    cw = t.dir[dir_index<C, DIRFREE_OK<CE, C, HASN>>(myblk, lane_base + l_, myc)];
                }
                return (u32)__builtin_amdgcn_readlane((int)cw, __builtin_amdgcn_readfirstlane(4 * k + (c_ & 3)));
            };
            if (dt_flags & TF_DIAG_SKIP_TRACEBACK) {
                if constexpr (DIRFREE_OK<CE, C, HASN>) {
                    // timing diagnostics: with GAMDP_DIAG_COUNT_MAT as well, do the strip materialisations a walk down
                    // the middle of the band would ask for, and nothing else
                    if (dt_flags & TF_DIAG_COUNT_MAT)
                        for (int g_hi = (t.df_hi >> 2) - 1; g_hi >= (t.df_lo >> 2); g_hi -= ST::groups_of(ST::strip_of(lane_base + (Y / 2) / C, t.sshift)))
                            materialise_auto<C, (DIRFREE_OK<CE, C, HASN> ? CE : 0), HASN, LPT, PK>(tp, ST::strip_of(lane_base + (Y / 2) / C, t.sshift), g_hi, lane, pk_half, lane_base);
                }
                x = -1;
            }
            int walk_it = 0;
            while (x >= 0 && y >= 0 && pos >= 0) {
                if constexpr (EARLY) {   // (a chain twin nobody waits for any more: its record is never looked at)
                    walk_it = uni(walk_it) + 1;
                    if ((walk_it & 31) == 0 && cancelled(t.cancel)) break;
                }
                // the walk state is wave-uniform by construction; pin it to scalar registers every iteration so
                // the body is selected as SALU code whatever the divergence analysis concluded about the loop
                x = uni(x); y = uni(y); pos = uni(pos); l = uni(l); c = uni(c);
#ifdef GAMDP_DIAG_COUNTERS
                dg_iters = uni(dg_iters) + 1; dg_refills = uni(dg_refills); mat_calls = uni(mat_calls);
#endif
                cblk0 = uni(cblk0); cl = uni(cl); cg = uni(cg);
                mat_q = uni(mat_q); mat_lo = uni(mat_lo); mat_hi = uni(mat_hi); cvalid_lo = uni(cvalid_lo);
                old_q = uni(old_q); old_lo = uni(old_lo); old_hi = uni(old_hi);
                sa_w0 = uni64(sa_w0); sb_w0 = uni64(sb_w0);
                if (HASN) { san_w0 = uni64(san_w0); sbn_w0 = uni64(sbn_w0); }
                if (x == 0 || pos == 0 || (!OPSRUN && want_ops)) {
                    // single step with the reference's exact rules
                    const int pa = HASN ? code_at(t.a2, t.an, t.a_base + pos) : (int)((t.a2[(t.a_base + pos) >> 4] >> (((t.a_base + pos) & 15) * 2)) & 3);
                    const int64_t bi = t.b_base + t.begin_b + x;
                    const int pb = HASN ? code_at(t.b2, t.bn, bi) : (int)((t.b2[bi >> 4] >> ((bi & 15) * 2)) & 3);
                    const bool is_match = (pa == pb) || pa == 4 || pb == 4;
                    int op;  // 0 GAP_A, 1 GAP_B, 2 diag
                    if (pos == 0) {
                        const int s = score_of(pa, pb);
                        const int h = (x == 0) ? t.h0row[y] : t.pos0[x];
                        const bool left_ok = !(t.fs && x > FORCE_MAXGAP);
                        if (h == s) op = 2;
                        else if (y == Y - 1 || (left_ok && h == GAP)) op = 1;
                        else op = 0;
                    } else if (x == 0) {
                        const int s = score_of(pa, pb);
                        const int h = t.h0row[y];
                        const bool up_ok = !(t.fs && pos > FORCE_MAXGAP);
                        if (h == s) op = 2;
                        else if (y < Y - 1 && y > 0 && up_ok && h == GAP) op = 0;
                        else if (y < Y - 1 && y > 0) op = 1;
                        else if (y < Y - 1) op = 0;
                        else op = 1;
                    } else {
                        const int tau = x + l, blk = tau >> 4;
                        const u32 cw = get_word(blk, l, c);
                        const u32 tag = (cw >> ((tau & 15) * 2)) & 3u;
                        op = (tag == 2u) ? 2 : (tag == 1u ? 0 : 1);
                    }
                    if (op == 2) {
                        if (is_match) {
                            nm++;
                            if (!have_last) { have_last = true; la = pos; lb = t.begin_b + x; post_early((ST_OK << 8) | 2u, la, lb); }
                            have_first = true; fa = pos; fb = t.begin_b + x;
                        }
                        if (want_ops && len < dt_ops_cap) ops[len] = is_match ? 2 : 3;
                        x--; pos--;
                    } else if (op == 1) {  // GAP_B: consumes a
                        if (want_ops && len < dt_ops_cap) ops[len] = 1;
                        y--; pos--;
                        if (--c < 0) { c = C - 1; l--; }
                    } else {  // GAP_A: consumes b
                        if (want_ops && len < dt_ops_cap) ops[len] = 0;
                        x--; y++;
                        if (++c == C) { c = 0; l++; }
                    }
                    len++;
                } else {
                    // interior: consume a whole run of diagonal steps in one go, with all 64 lanes: the lanes that hold
                    // this column's words of the cached blocks find where the run ends (ballot), then 16 bases per
                    // lane are compared straight out of the two packed-sequence windows.  A single wavefront issues
                    // about one instruction per 4 cycles, so the walk is bound by its instruction count, not by the
                    // vector ALU: one iteration per run instead of one per direction word.
                    const int tau = x + l, blk = tau >> 4, r = tau & 15;
                    if constexpr (SKIP) {
                        // ---- get_word() would ask for a strip here: are the groups below nothing but diagonal steps?  (kernel_walk.inc,
                        // walk_many<..., SKIP>: the same test, the same validity rules, in the same units -- a diagonal step adds 12 or 21
                        // to G = H + 16 x + 8 y, which is what materialise_impl's unpack() for PK, LPT == 64 yields before its factor 4.)
                        // The walk state is wave-uniform here, so all 64 lanes take a span each: lane k the k-th one below the walk (the
                        // first down to the next checkpoint row, 64 rows each after that), up to 4 096 rows per test.  A test costs one
                        // memory round trip however many lanes take part -- every lane's loads are in flight together -- and the walk of a
                        // lone wavefront is bound by its round trips and its instruction count: an indel-free 50 kb path takes 13 tests.
                        // Int32 images (!PK): the row holds G4 = 4 G itself, so the same equality in units of 4 -- a diagonal step adds
                        // 4 (S + 16) = 84 for equal codes (N-N too), 64 when exactly one side is N, 48 for a mismatch: what enc_b() puts
                        // into the untagged ring of do_block_df.  With four tasks per wavefront the lanes of the row are lane_base + l;
                        // all 64 lanes of the wavefront still take a span each, the walk has the wavefront to itself.
                        const int strip = ST::strip_of(lane_base + l, t.sshift);
                        const bool sk_cand = sk_on && blk >= t.df_lo && blk < t.df_hi && sk_fail_at != mat_calls && !(blk >= mat_lo && blk <= mat_hi) &&
                                             !(strip == old_q && blk >= old_lo && blk <= old_hi);
                        if (sk_cand && backoff && bo_hold != 0u) {   // held: no test, no load -- on as after a failed one
                            bo_hold--; sk_held++;
                            sk_fail_at = mat_calls;
                        } else if (sk_cand) {
                            constexpr int UNIT = PK ? 1 : 4;                                 // what the checkpoint rows count in: G or G4
                            const int gi = blk >> 2, d0 = (tau & 63) + 1;                    // checkpoint gi: d0 steps below the walk
                            const int g_lo = t.df_lo >> 2, g_top = (t.df_hi >> 2) - 1;       // the groups whose checkpoint rows the fill stored
                            const int off = (lane == 0) ? 0 : d0 + 64 * (lane - 1), cnt = (lane == 0) ? d0 : 64;   // this lane's span: steps [off, off + cnt) from the top
                            const int gb = gi - lane;                                        // the checkpoint at its lower end, gb + 1 at its upper end
                            const int ll = min(max(l, 0), LPT - 1), cc = min(max(c, 0), C - 1);
                            // every cell of the span is an else-branch cell of the fill (the cell it ends on keeps x >= 1, pos >= 1: row 0
                            // and pos == 0 stay with the single steps above), its lower checkpoint row exists
                            const bool at_start = len == 0u;
                            const bool up_ok = (lane == 0) ? (at_start || (d0 == 64 && gi + 1 <= g_top)) : true;
                            const bool span_ok = up_ok && gb >= g_lo && x - (off + cnt) >= 1 && pos - (off + cnt) >= 1;
                            auto ck_val = [&](const int gidx) -> int {   // as materialise_impl's unpack(raw[c], ckbase) for PK, LPT == 64, in units of G
                                if constexpr (PK) {
                                    typedef PairFmt<C, LPT> FMT;
                                    gptr ck = t.ckpt + (u64)min(max(gidx, g_lo), g_top) * (u64)FMT::CK_WORDS;
                                    const u32 v = ck[(u32)ll * FMT::CK_LANE + cc];
                                    return pat_decode(pk_half ? v >> 16 : v & 0xFFFFu) + (int)ck[FMT::CK_ROWS + pk_half * 64 + ll];
                                } else {   // ... and its (int)raw[c] for the int32 images: word c of wavefront lane lane_base + l (img_store<C, true> in do_block_df), G4
                                    gptr ck = t.ckpt + (u64)min(max(gidx, g_lo), g_top) * (u64)IMG_WORDS<C, true>;
                                    return (int)ck[(u32)(lane_base + ll) * (u32)LANE_WORDS<C> + (u32)cc];
                                }
                            };
                            const int g_bot = ck_val(gb), g_up = ck_val(gb + 1);
                            // (a lane without a span reads lane 0's bases: nothing in front of the sequences' padding is touched)
                            const int off_ld = span_ok ? off : 0;
                            typedef typename SkipIdx<PK>::T SI;
                            const SI ia_lo = (SI)t.a_base + pos - off_ld - 63, ib_lo = (SI)t.b_base + t.begin_b + x - off_ld - 63;   // base p of the span's 64 (0 = lowest row)
                            u32 aw[5], bw[5];
#pragma unroll
                            for (int k = 0; k < 5; ++k) { aw[k] = t.a2[(ia_lo >> 4) + k]; bw[k] = t.b2[(ib_lo >> 4) + k]; }
                            // N-aware: the N planes of the same 64 bases (32 per word), bit p = base p; a MATCH is equal codes or an N on either
                            // side (the reference's op), the score tells N-N (5, an equal pair) from exactly one N (0)
                            [[maybe_unused]] u32 na[2] = {0u, 0u}, nb[2] = {0u, 0u};
                            if constexpr (HASN) {
                                u32 anw[3], bnw[3];
#pragma unroll
                                for (int k = 0; k < 3; ++k) { anw[k] = t.an[(ia_lo >> 5) + k]; bnw[k] = t.bn[(ib_lo >> 5) + k]; }
#pragma unroll
                                for (int k = 0; k < 2; ++k) {
                                    na[k] = __builtin_amdgcn_alignbit(anw[k + 1], anw[k], (u32)(ia_lo & 31));
                                    nb[k] = __builtin_amdgcn_alignbit(bnw[k + 1], bnw[k], (u32)(ib_lo & 31));
                                }
                            }
                            // the upper value: the score at the end cell, else the checkpoint row the walk stands on (a full span of 64)
                            const int g_top_val = (lane == 0 && at_start) ? UNIT * (best + 16 * x + 8 * y) : g_up;
                            const int p0 = 64 - cnt;                                         // lane 0: the top d0 bases only
                            u32 eq[4];
                            int m = 0;
                            [[maybe_unused]] int n1 = 0;   // pairs with exactly one N
#pragma unroll
                            for (int k = 0; k < 4; ++k) {
                                const u32 a16 = __builtin_amdgcn_alignbit(aw[k + 1], aw[k], (u32)(ia_lo & 15) * 2u), b16 = __builtin_amdgcn_alignbit(bw[k + 1], bw[k], (u32)(ib_lo & 15) * 2u);
                                const u32 xr = a16 ^ b16, ne = (xr | (xr >> 1)) & 0x55555555u;
                                const int q0 = p0 - 16 * k;
                                const u32 msk = (q0 <= 0) ? 0x55555555u : ((q0 >= 16) ? 0u : (0x55555555u << (2 * q0)));
                                if constexpr (HASN) {
                                    auto spread = [](u32 v) -> u32 {   // 16 bits to the even positions
                                        v = (v | (v << 8)) & 0x00FF00FFu;
                                        v = (v | (v << 4)) & 0x0F0F0F0Fu;
                                        v = (v | (v << 2)) & 0x33333333u;
                                        return (v | (v << 1)) & 0x55555555u;
                                    };
                                    const u32 a16n = (na[k >> 1] >> (16 * (k & 1))) & 0xFFFFu, b16n = (nb[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
                                    const u32 any = spread(a16n | b16n), both = spread(a16n & b16n);
                                    const u32 e_k = (both | (~any & ~ne)) & msk, n1_k = any & ~both & msk;
                                    m += __builtin_popcount(e_k);
                                    n1 += __builtin_popcount(n1_k);
                                    eq[k] = e_k | n1_k;
                                } else {
                                    eq[k] = ~ne & msk;
                                    m += __builtin_popcount(eq[k]);
                                }
                            }
                            const int mm = HASN ? m + n1 : m;   // MATCH ops of the span
                            const bool pass = span_ok && g_top_val - g_bot == UNIT * (12 * cnt + 9 * m) + (HASN ? 16 * n1 : 0);
                            const u64 m_pass = __ballot(pass);
                            const int np = (~m_pass == 0ull) ? 64 : __builtin_ctzll(~m_pass);   // the passing prefix
                            sk_tests++; sk_tested += (u32)__builtin_popcountll(__ballot(span_ok));
                            if (np > 0) {
                                const bool inc = lane < np;
                                int cnt_m = inc ? mm : 0;
                                cnt_m += __builtin_amdgcn_update_dpp(0, cnt_m, 0xB1, 0xf, 0xf, true);   // quad_perm:[1,0,3,2]
                                cnt_m += __builtin_amdgcn_update_dpp(0, cnt_m, 0x4E, 0xf, 0xf, true);   // quad_perm:[2,3,0,1]
                                cnt_m += __builtin_amdgcn_update_dpp(0, cnt_m, 0x141, 0xf, 0xf, true);  // row_half_mirror
                                cnt_m += __builtin_amdgcn_update_dpp(0, cnt_m, 0x140, 0xf, 0xf, true);  // row_mirror: every lane = its row's sum
                                nm += (u32)(__builtin_amdgcn_readlane(cnt_m, 0) + __builtin_amdgcn_readlane(cnt_m, 16) +
                                            __builtin_amdgcn_readlane(cnt_m, 32) + __builtin_amdgcn_readlane(cnt_m, 48));
                                const u64 m_eq = __ballot(inc && mm > 0);
                                if (m_eq) {
                                    int ptop = 0, pbot = 0;
#pragma unroll
                                    for (int kk = 0; kk < 4; ++kk) if (eq[kk]) ptop = 16 * kk + ((31 - __builtin_clz(eq[kk])) >> 1);
#pragma unroll
                                    for (int kk = 3; kk >= 0; --kk) if (eq[kk]) pbot = 16 * kk + (__builtin_ctz(eq[kk]) >> 1);
                                    const int off_hi = __builtin_amdgcn_readlane(off + 63 - ptop, __builtin_ctzll(m_eq));        // steps below the walk
                                    const int off_lo = __builtin_amdgcn_readlane(off + 63 - pbot, 63 - __builtin_clzll(m_eq));
                                    if (!have_last) { have_last = true; la = pos - off_hi; lb = t.begin_b + x - off_hi; }
                                    have_first = true; fa = pos - off_lo; fb = t.begin_b + x - off_lo;
                                }
                                const int n = d0 + 64 * (np - 1);
                                x -= n; pos -= n; len += (u32)n;
                                sk_groups += (u32)np; sk_short += (u32)(64 - d0);
                                cblk0 = -1; cl = -1; cg = -1;   // the cached direction words are those of the blocks the walk has left
                                bo_fails = 0u;
                                continue;                       // round again: the next test, directions, or row 0 / pos == 0
                            }
                            sk_fail_at = mat_calls;
                            if (backoff) {
                                bo_fails = bo_fails < WALK_BACKOFF_FAILS_CAP ? bo_fails + 1u : WALK_BACKOFF_FAILS_CAP;
                                bo_hold = walk_backoff_hold(bo_fails);
                            }
                        }
                    }
                    const u32 w_here = get_word(blk, l, c);  // (re)fills the cache / materialises the strip if needed
                    const int k0 = cblk0 - blk, e = c & 3;
                    const int myk = lane >> 2;
                    const bool mine = ((lane & 3) == e) && myk >= k0 && (cblk0 - myk) >= max(cvalid_lo, 0);
                    u32 T = cw ^ 0xAAAAAAAAu;  // a diagonal step reads 00
                    if (myk == k0) T <<= (30 - 2 * r);  // the block the walk stands in: row r on top
                    const int avail = T ? (__builtin_clz(T) >> 1) : ((myk == k0) ? r + 1 : 16);
                    const u64 m_mine = __ballot(mine), m_stop = __ballot(mine && T != 0u);
                    int n, Ls = -1;
                    if (m_stop == 0) {
                        n = (r + 1) + 16 * (((63 - __builtin_clzll(m_mine)) >> 2) - k0);
                    } else {
                        Ls = __builtin_ctzll(m_stop);
                        const int ks = Ls >> 2;
                        const int lead = __builtin_amdgcn_readlane(avail, Ls);
                        n = (ks == k0) ? lead : (r + 1) + 16 * (ks - k0 - 1) + lead;
                    }
                    const int n_run = n;
                    n = min(n, min(x, pos));  // stay in x >= 1, pos >= 1
                    if (n > 0) {
                        // chunk j (from the top of the run) = bases [hi - 16j - 15, hi - 16j] of both sequences
                        const int64_t ia_hi = t.a_base + pos, ib_hi = t.b_base + t.begin_b + x;
                        const int64_t wa = (ia_hi - 15) >> 4, wb = (ib_hi - 15) >> 4;
                        const int64_t wa_bot = (ia_hi - n - 15) >> 4, wb_bot = (ib_hi - n - 15) >> 4;
                        if (wa + 1 > sa_w0 || wa_bot < sa_w0 - 63) { sa_w0 = wa + 1; sa_v = t.a2[sa_w0 - lane]; }
                        if (wb + 1 > sb_w0 || wb_bot < sb_w0 - 63) { sb_w0 = wb + 1; sb_v = t.b2[sb_w0 - lane]; }
                        const int da = (int)(sa_w0 - wa), db = (int)(sb_w0 - wb);  // lane of chunk 0's low word (>= 1)
                        const u32 a16 = __builtin_amdgcn_alignbit((u32)wave_shr1(0, (int)sa_v), sa_v, (u32)((ia_hi - 15) & 15) * 2u);
                        const u32 b16s = __builtin_amdgcn_alignbit((u32)wave_shr1(0, (int)sb_v), sb_v, (u32)((ib_hi - 15) & 15) * 2u);
                        const u32 b16 = (u32)__builtin_amdgcn_ds_bpermute(4 * (lane + db - da), (int)b16s);
                        const int j = lane - da;
                        const u32 xr = a16 ^ b16;
                        u32 ne = (xr | (xr >> 1)) & 0x55555555u;  // bit 2p set: bases p differ
                        if constexpr (HASN) {
                            // a base that is N on either side counts as a MATCH: the 16 mask bits of this lane's chunk
                            // come out of two 64-word windows of the N planes (32 bases per word), fetched per lane
                            const int64_t na_lo = ia_hi - 15 - 16 * (int64_t)j, nb_lo = ib_hi - 15 - 16 * (int64_t)j;
                            const int64_t wna = (ia_hi >> 5) + 1, wnb = (ib_hi >> 5) + 1;  // highest word needed
                            const int64_t wna_bot = (ia_hi - n - 31) >> 5, wnb_bot = (ib_hi - n - 31) >> 5;
                            if (wna > san_w0 || wna_bot < san_w0 - 63) { san_w0 = wna; san_v = t.an[san_w0 - lane]; }
                            if (wnb > sbn_w0 || wnb_bot < sbn_w0 - 63) { sbn_w0 = wnb; sbn_v = t.bn[sbn_w0 - lane]; }
                            auto nbits = [&](const u32 win, const int64_t w0, const int64_t lo) -> u32 {
                                const int src = (int)(w0 - (lo >> 5));  // lane holding the word with base `lo`
                                const u32 wl = (u32)__builtin_amdgcn_ds_bpermute(4 * src, (int)win);
                                const u32 wh = (u32)__builtin_amdgcn_ds_bpermute(4 * (src - 1), (int)win);
                                return __builtin_amdgcn_alignbit(wh, wl, (u32)(lo & 31)) & 0xFFFFu;
                            };
                            u32 nn = nbits(san_v, san_w0, na_lo) | nbits(sbn_v, sbn_w0, nb_lo);
                            nn = (nn | (nn << 8)) & 0x00FF00FFu;  // spread the 16 bits to the even positions
                            nn = (nn | (nn << 4)) & 0x0F0F0F0Fu;
                            nn = (nn | (nn << 2)) & 0x33333333u;
                            nn = (nn | (nn << 1)) & 0x55555555u;
                            ne &= ~nn;
                        }
                        const int p0 = 16 * j + 16 - n;                 // first base of the chunk that still belongs to the run
                        u32 msk = (p0 <= 0) ? 0x55555555u : ((p0 >= 16) ? 0u : (0x55555555u << (2 * p0)));
                        if (j < 0) msk = 0u;
                        u32 eq = ~ne & msk;
                        const u64 m_eq = __ballot(eq != 0u);
                        if (m_eq) {
                            // sum over the wavefront with DPP adds (a butterfly through ds_bpermute costs six LDS round trips)
                            int cnt = __builtin_popcount(eq);
                            cnt += __builtin_amdgcn_update_dpp(0, cnt, 0xB1, 0xf, 0xf, true);   // quad_perm:[1,0,3,2]
                            cnt += __builtin_amdgcn_update_dpp(0, cnt, 0x4E, 0xf, 0xf, true);   // quad_perm:[2,3,0,1]
                            cnt += __builtin_amdgcn_update_dpp(0, cnt, 0x141, 0xf, 0xf, true);  // row_half_mirror
                            cnt += __builtin_amdgcn_update_dpp(0, cnt, 0x140, 0xf, 0xf, true);  // row_mirror: every lane = its row's sum
                            nm += (u32)(__builtin_amdgcn_readlane(cnt, 0) + __builtin_amdgcn_readlane(cnt, 16) +
                                        __builtin_amdgcn_readlane(cnt, 32) + __builtin_amdgcn_readlane(cnt, 48));
                            const int Ltop = __builtin_ctzll(m_eq), Lbot = 63 - __builtin_clzll(m_eq);
                            const u32 eq_top = (u32)__builtin_amdgcn_readlane((int)eq, Ltop), eq_bot = (u32)__builtin_amdgcn_readlane((int)eq, Lbot);
                            const int off_hi = 16 * (Ltop - da) + 15 - ((31 - __builtin_clz(eq_top)) >> 1);  // steps below the top of the run
                            const int off_lo = 16 * (Lbot - da) + 15 - (__builtin_ctz(eq_bot) >> 1);
                            if (!have_last) { have_last = true; la = pos - off_hi; lb = t.begin_b + x - off_hi; post_early((ST_OK << 8) | 2u, la, lb); }
                            have_first = true; fa = pos - off_lo; fb = t.begin_b + x - off_lo;
                        }
                        if constexpr (OPSRUN) {
                            // the run's ops, in traceback order: step s = 16 j + 15 - p from the top of the run is base p of this lane's
                            // chunk, `msk` holds the bases that belong to the run (none for j < 0), `eq` those of them that are a MATCH
#pragma unroll
                            for (int p = 0; p < 16; ++p) {
                                const u64 at = (u64)len + (u64)(16 * j + 15 - p);
                                if (((msk >> (2 * p)) & 1u) && at < dt_ops_cap) ops[at] = (uint8_t)(3u - ((eq >> (2 * p)) & 1u));
                            }
                            or_ops += (u32)n; or_runs++;
                        }
                        x -= n; pos -= n; len += (u32)n;
                        // the run ended at a gap whose direction word is in the cache: take that step right away
                        if (Ls >= 0 && n == n_run && x >= 1 && pos >= 1) {
                            const u32 w2 = (u32)__builtin_amdgcn_readlane((int)cw, Ls);
                            const u32 tag2 = (w2 >> (((x + l) & 15) * 2)) & 3u;
                            if constexpr (OPSRUN) { if (len < dt_ops_cap) ops[len] = (tag2 == 1u) ? 0 : 1; }
                            if (tag2 == 1u) {  // GAP_A
                                x--; y++;
                                if (++c == C) { c = 0; l++; }
                            } else {  // GAP_B
                                y--; pos--;
                                if (--c < 0) { c = C - 1; l--; }
                            }
                            len++;
                        }
                    } else {
                        const u32 tag = (w_here >> (r * 2)) & 3u;
                        if constexpr (OPSRUN) { if (len < dt_ops_cap) ops[len] = (tag == 1u) ? 0 : 1; }
                        if (tag == 1u) {  // GAP_A
                            x--; y++;
                            if (++c == C) { c = 0; l++; }
                        } else {  // GAP_B
                            y--; pos--;
                            if (--c < 0) { c = C - 1; l--; }
                        }
                        len++;
                    }
                }
            }
            res.begin_a = pos + 1;
            res.begin_b = t.begin_b + x + 1;
            res.score = best;
            res.n_match = nm;
            res.length = len;
            // first_match_pos without a MATCH returns the end coordinates, last_match_pos the begin ones
            res.first_a = have_first ? fa : end_pos + 1;
            res.first_b = have_first ? fb : t.begin_b + end_x + 1;
            res.last_a = have_last ? la : res.begin_a;
            res.last_b = have_last ? lb : res.begin_b;
            res.flags = (have_first ? 1u : 0u) | (have_last ? 2u : 0u) | (ST_OK << 8);
            if (pp->stats != nullptr && lane == 0 && mat_calls > 0) atomicAdd(unip(pp->stats) + LS_STRIPS, (u32)mat_calls);   // (gamdp_ctx_launch_info)
            if constexpr (SKIP) {
                if (pp->stats != nullptr && lane == 0 && sk_tests != 0) {   // (gamdp_ctx_walk_skip_pair_stats, gamdp_ctx_walk_skip_i32_stats)
                    atomicAdd(unip(pp->stats) + LS_SKIP_TESTS, sk_tests);
                    atomicAdd(unip(pp->stats) + LS_SKIP_TESTED, sk_tested);
                    atomicAdd(unip(pp->stats) + LS_SKIP_GROUPS, sk_groups);
                    if (sk_short != 0) atomicAdd(unip(pp->stats) + LS_SKIP_SHORT, sk_short);
                }
                if (pp->stats != nullptr && lane == 0 && sk_held != 0) atomicAdd(unip(pp->stats) + LS_SKIP_HELD, sk_held);   // (gamdp_ctx_walk_skip_backoff_stats)
            }
            if constexpr (OPSRUN) {
                if (pp->stats != nullptr && lane == 0) {   // (gamdp_ctx_ops_walk_stats: steps, clipped or not)
                    stat_add64(unip(pp->stats) + LS_OPS_BY_RUN, or_ops);
                    stat_add64(unip(pp->stats) + LS_OPS_BY_STEP, len - or_len0 - or_ops);
                    stat_add64(unip(pp->stats) + LS_OPS_RUNS, or_runs);
                }
            }
            if (dt_flags & TF_DIAG_COUNT_MAT) {  // diagnostics only: result unusable
                res.n_match = (u32)mat_calls;
                res.first_a = (int)mat_ticks + uni(wcp->mat_ticks);
                res.first_b = (int)(wall_clock64() - walk_t0);
                res.last_a = dg_iters; res.last_b = dg_refills;
            }
        }
    }
    if constexpr (OPSRUN) {
        if (pp->stats != nullptr && lane == 0) atomicAdd(unip(pp->stats) + LS_OPS_TASKS, 1u);   // (every status: a task without a walk has no ops)
    }
#ifdef GAMDP_DIAG
    if (uni(t.pos0[-1]) != 0) res.flags = ST_DIAG_RANGE << 8;   // a packed block of this task left the exact f16 range
#endif
    if (lane == 0) p_results[dt_res_idx] = res;
    if constexpr (EARLY) {
        post_early(res.flags, res.last_a, res.last_b);   // (no match on the path, an empty alignment, a call the reference throws on)
        // is_good(vector) (PctgBuilder.cc:1711-1724) as run_chain takes it: homology >= 95 <=> n_match * 100 >= 95 * length
        const u32 status = res.flags >> 8;
        if (lane == 0) {
            if (status == ST_OK) {
                if (res.length == 0 || (u64)res.n_match * 100u < 95ull * (u64)res.length) atomicOr(&s_mail.bad, 1);
                atomicAdd(&s_mail.sum, (unsigned long long)res.length);
            } else atomicOr(&s_mail.bad, 1);
        }
        mail_post(&s_mail.done_of[(early_seq - 1) % CH_NS], early_seq, lane);   // (waits for the record's store as well)
        if (lane == 0) __hip_atomic_fetch_add(&s_mail.n_done, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else __syncthreads();
}

// end cell + walk of one task, the whole wavefront on it
template <int C, int CE, bool HASN, int LPT = 64, bool PK = false>
__device__ __forceinline__ void finish_task(const Tk* tp, const DevTask* dtp, const LaunchParams* pp, const int lane, const int lane_base = 0, const int pk_half = 0)
{
    WalkCarry wc;
    end_cell<C>(tp, lane, &wc);
    // (LP_OPS_WALK_RUNS: the instance that writes the edit string a run at a time -- wave-uniform, per task)
    if (ops_walk_runs(pp, dtp)) { finish_walk<C, CE, HASN, LPT, PK, false, false, true>(tp, dtp, pp, lane, lane_base, pk_half, &wc); return; }
    // (LP_WALK_SKIP_I32: the instance whose walk makes the diagonal test -- wave-uniform, per launch)
    if constexpr (!PK && DIRFREE_OK<CE, C, HASN>) {
        if (pp->flags & LP_WALK_SKIP_I32) { finish_walk<C, CE, HASN, LPT, PK, false, true>(tp, dtp, pp, lane, lane_base, pk_half, &wc); return; }
    }
    finish_walk<C, CE, HASN, LPT, PK>(tp, dtp, pp, lane, lane_base, pk_half, &wc);
}
