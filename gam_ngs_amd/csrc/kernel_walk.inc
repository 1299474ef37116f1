// Part of gamdp_kernel.hip (included inside namespace gamdp::{anonymous}): the interior of the walks of ALL tasks of a wavefront at once.

// ---- four / eight walks side by side ----------------------------------------------------------------------------
// finish_walk (kernel_finish.inc) puts the whole wavefront on one task and keeps the walk state in scalar registers: right
// for one task per wavefront, but the eight walks of an eight-task wavefront then run one after the other, ~300 scalar
// instructions per diagonal run, and when the co-resident wavefronts walk at the same time (equal task lengths: all of
// them do) the one scalar unit of the CU is the bottleneck: 36 of 176 ms on 100 000 x 50 kb at band 150.
// Here every task gets 8 lanes (lane j of a group = block blk0 - j of the task's current column: 128 rows deep), the
// state lives in vector registers, uniform within a group, and one instruction stream advances all tasks: per iteration
// every lane loads its direction word and the packed bases of its 16 steps (all loads of an iteration in flight
// together: one memory latency), the group finds the end of the diagonal run, counts the matches, takes the gap that
// ended the run.  Same steps, same arithmetic as finish_walk's run consumer -- only the lanes are dealt differently.
// A task whose next block has no directions yet gets its strip from materialise() (the whole wavefront on that task, as
// before).  What the reference treats specially (row 0, pos == 0) is left to finish_walk: a task drops out as soon as
// x < 1 or pos < 1, its state goes back into its WalkCarry, and finish_walk takes the last steps and writes the result.
// Tasks with bit set in skip_mask (edit string wanted) are not touched.
// LPT = 64: the two tasks of the packed band-512 kernel (NT = 2: task A and task B of the pair, each owning all 64 lanes of the
// fill; *tap / *tbp hold wave-uniform values), groups 2..7 idle.
// tks (LPT = QL): the wave-uniform values of the NT tasks, one after the other, in LDS (finish_many puts them there once per
// wavefront unit): what a strip call is handed.  (Until round 5 every call built them again with ~60 v_readlane and left them in
// private memory for the callee: 12 KB of scratch written per call -- with the callee's own register saves as many bytes as
// the direction words the call produces, and scratch that is rewritten every ~200 us does reach HBM.)
// Returns the tasks (bit s) whose walks wait for a strip, 0 when every walk has got as far as it can.  With a task per DPP row (LPT =
// QL) the function RETURNS for the strips: every task's state goes back into its carry, a waiting task's carry says which strip
// (need_q) down from which group (need_ghi), the caller -- the kernel itself, finish_many -- makes the strips with materialise()
// inlined and calls again.  Nothing of the walks is in registers while a strip is made, so nobody saves registers around it
// (as a call from in here: 28 callee-saved registers stored and re-loaded per strip call, 14 KB of scratch each time).  The
// two-task kernel (LPT = 64: carries in the caller's frame, one copy per lane) keeps the call in here and always returns 0.
// SKIP (the packed kernels: the eight-task one under LP_WALK_SKIP_DIAG, the two-task one under LP_WALK_SKIP_PAIR; a second instance,
// the default one holds none of it): a walk that stands on a block without directions first asks whether the groups below it hold
// nothing but diagonal steps, and jumps over those that do (the test sits where the inner loop finds `need`) before it is reported as
// waiting for a strip.  skip_stats: the launch's statistics words (LS_SKIP_*), nullptr = not counted.
// SKIP with WM_BACKOFF in skip_mask_ (LP_WALK_SKIP_BACKOFF, gamdp_dev.h has the rule): a task that is held passes its candidate point as
// after a failed test, and an iteration whose candidate tasks are all held does not enter the test at all -- no load, no round trip.
// The two values of a task's walk live in its carry's early_seq between calls (the chain walkers' field: no multi-task walk uses it,
// end_cell zeroes it), as one word (walk_backoff_after_fail).
constexpr int WM_BACKOFF = 1 << 8;   // (above the NT <= 8 task bits of skip_mask_)
template <int C, int CE, bool HASN, bool PK, int NT, int LPT = QL, bool SKIP = false>
__device__ __noinline__ u32 walk_many(const Tk* tap, const Tk* tbp, WalkCarry* wcs, const int skip_mask_, const int lane, const Tk* tks = nullptr, u32* skip_stats = nullptr)
{
    static_assert(!SKIP || (PK && ((LPT == QL && NT == 8) || (LPT == 64 && NT == 2))), "the diagonal test reads the packed kernels' checkpoint rows (PairFmt)");
    static_assert(DIRFREE_OK<CE, C, HASN>, "the multi-task kernels are direction-free kernels");
    static_assert((LPT == QL && (NT == 4 || NT == 8)) || (LPT == 64 && NT == 2 && PK), "one or two quads, or the pair of the two-task kernel");
    static_assert(!HASN, "only the N-free kernels use it (the N planes would be two more word pairs per lane and iteration)");
    typedef Strip<LPT, PK> ST;
    const int g = lane >> 3, j = lane & 7;
    const int gt = min(g, NT - 1);        // the task this lane works on (groups past the last task idle along with it)
    const int half = (LPT == 64) ? gt : gt >> 2, s4 = gt & 3;
    const int lane_base = (LPT == 64) ? 0 : QL * s4;   // the task's lanes of the fill: where its direction words and strips live
    const int src = 4 * lane_base;        // ds_bpermute address of a lane that holds the task's values
    const int skip_mask = uni(skip_mask_);
    // *tap / *tbp: per lane, the values of the task of this lane's DPP row in quad A / quad B.  They stay in memory: only the
    // few the walk needs are picked into registers (a copy of both structs in registers made the loop spill)
    const Tk* const tbq = PK ? tbp : tap;
    auto pick = [&](const int va, const int vb) -> int {
        if constexpr (LPT == 64) return half ? vb : va;   // wave-uniform values: nothing to fetch from another lane
        const int a = __builtin_amdgcn_ds_bpermute(src, va);
        if constexpr (!PK) return a;
        const int b = __builtin_amdgcn_ds_bpermute(src, vb);
        return half ? b : a;
    };
    auto pick64 = [&](const u64 va, const u64 vb) -> u64 {
        const u32 lo = (u32)pick((int)(u32)va, (int)(u32)vb), hi = (u32)pick((int)(u32)(va >> 32), (int)(u32)(vb >> 32));
        return ((u64)hi << 32) | lo;
    };
    gcptr const a2 = (gcptr)pick64((u64)tap->a2, (u64)tbq->a2), b2 = (gcptr)pick64((u64)tap->b2, (u64)tbq->b2);
    // (offsets into a contig: they and every base index derived from them fit 32 bits, gamdp_host.cpp limits the lengths)
    const int a_base = pick((int)tap->a_base, (int)tbq->a_base), begin_b = pick(tap->begin_b, tbq->begin_b);
    const int bb_base = pick((int)tap->b_base, (int)tbq->b_base) + begin_b;   // b index of row 0
    gptr const dir = (gptr)pick64((u64)tap->dir, (u64)tbq->dir);
    const int df_lo = pick(tap->df_lo, tbq->df_lo), df_hi = pick(tap->df_hi, tbq->df_hi);
    const int sshift = uni(tap->sshift);   // the same for every task of the wavefront

    const WalkCarry w0 = wcs[gt];
    int x = w0.x, y = w0.y, pos = w0.pos;
    u32 len = w0.len, nm = w0.nm;
    int la = w0.la, lb = w0.lb, fa = w0.fa, fb = w0.fb, have = w0.have;
    int mat_q = w0.mat_q, mat_lo = w0.mat_lo, mat_hi = w0.mat_hi, old_q = w0.old_q, old_lo = w0.old_lo, old_hi = w0.old_hi;
    int mat_calls = w0.mat_calls;
    int l = y / C, c = y - l * C;
    bool active = g < NT && w0.status == 2 && !((skip_mask >> gt) & 1);
    // SKIP: a task whose test found no passing group waits for its strip (no second test before it has one); what this call counted
    [[maybe_unused]] bool stuck = false;
    [[maybe_unused]] u32 sk_tests = 0, sk_tested = 0, sk_groups = 0, sk_short = 0, sk_held = 0;
    // ... and with WM_BACKOFF the task's fails | hold word (never touched without it)
    [[maybe_unused]] const bool backoff = SKIP && (skip_mask & WM_BACKOFF) != 0;
    [[maybe_unused]] u32 bo = SKIP ? (u32)w0.early_seq : 0u;
    [[maybe_unused]] auto count_skips = [&]() {
        if constexpr (SKIP) {
            if (skip_stats != nullptr && j == 0 && g < NT) {
                if (sk_tests != 0) {
                    atomicAdd(skip_stats + LS_SKIP_TESTS, sk_tests);
                    atomicAdd(skip_stats + LS_SKIP_TESTED, sk_tested);
                    atomicAdd(skip_stats + LS_SKIP_GROUPS, sk_groups);
                    if (sk_short != 0) atomicAdd(skip_stats + LS_SKIP_SHORT, sk_short);
                }
                if (sk_held != 0) atomicAdd(skip_stats + LS_SKIP_HELD, sk_held);
            }
        }
    };

    // Outer loop: strips on demand; inner loop: the walk proper, left as soon as some task stands on a block without
    // directions (the call sits outside the inner loop so that the walk's registers are not spilled around it in there)
    for (;;) {
    u64 m_need = 0;
    int strip = 0, blk0 = 0;
    for (;;) {
        active = active && x >= 1 && pos >= 1 && y >= 0;
        const int ll = min(max(l, 0), LPT - 1);   // (only a task that has dropped out can be outside the band)
        const int tau = x + ll, r = tau & 15;
        blk0 = max(tau, 0) >> 4;
        // ---- are the directions of the block the walk stands in there?
        strip = ST::strip_of(lane_base + ll, sshift);
        int vlo = 0;            // blocks below this one are not usable from here
        bool need = false;
        if (blk0 >= df_hi) vlo = df_hi;   // tagged blocks; the direction-free ones below need a look of their own
        else if (blk0 >= df_lo) {
            if (strip == old_q && blk0 >= old_lo && blk0 <= old_hi) {
                // back in the strip the walk came from (a path sitting on a strip border): its words are still in memory
                const int tq = mat_q, tl = mat_lo, th = mat_hi;
                mat_q = old_q; mat_lo = old_lo; mat_hi = old_hi;
                old_q = tq; old_lo = tl; old_hi = th;
            } else if (!(strip == mat_q && blk0 >= mat_lo && blk0 <= mat_hi)) need = true;
            vlo = (mat_lo == df_lo) ? 0 : mat_lo;   // below df_lo the tagged blocks are all there
        }
        m_need = __ballot(active && need);
        if constexpr (SKIP) {
            // ---- no directions for blk0: are the groups below nothing but diagonal steps?
            // The reference's traceback tests diag first and steps diagonally iff sw[x][y] == sw[x-1][y] + S
            // (banded_smith_waterman.cc:265-285), and its fill makes sw[x][y] >= sw[x-1][y] + S in every cell with pos >= 1, x >= 1
            // (:158-168).  So when H(x, y) - H(x - n, y) equals the sum of S over the n base pairs between them, the sum
            // telescopes into n non-negative terms that add to zero: all n steps are diagonal, no direction word needed.  Both
            // values are in memory: checkpoint G holds every lane's row after row-time 64 G - 1 (materialise_impl starts from it),
            // and a walk runs out of directions exactly there (tau = 64 G - 1: the block below a tagged range or a used-up strip)
            // or at its end cell, whose H is the score.  In the fill's tilt G = H + 16 x + 8 y a diagonal step adds S + 16 (12 or
            // 21), so the stored values are compared as they are.  Lane j of the task's 8 tests the j-th span below the walk (the
            // first one down to the next checkpoint row, 64 rows each after that); the walk jumps over the passing prefix.
            // (A strip change inside materialised groups -- blk0 within [mat_lo, mat_hi] -- is left to the strips.)
            bool cand = active && need && !stuck && !(blk0 >= mat_lo && blk0 <= mat_hi);
            if (backoff) {
                // a held task passes the point as after a failed test; when every candidate task is held nobody enters the test below
                const bool held = cand && (bo >> WALK_BACKOFF_HOLD_SHIFT) != 0u;
                if (held) { bo -= 1u << WALK_BACKOFF_HOLD_SHIFT; stuck = true; sk_held++; cand = false; }
            }
            if (__ballot(cand) != 0) {
                typedef PairFmt<C, LPT> FMT;
                gptr const ckpt = (gptr)pick64((u64)tap->ckpt, (u64)tbq->ckpt);   // the slot's checkpoint rows
                const int gi = blk0 >> 2, d0 = (tau & 63) + 1;             // checkpoint gi: d0 steps below the walk
                const int g_lo = df_lo >> 2, g_top = (df_hi >> 2) - 1;     // the groups whose checkpoint rows the fill stored
                const int off = (j == 0) ? 0 : d0 + 64 * (j - 1), cnt = (j == 0) ? d0 : 64;   // this lane's span: steps [off, off + cnt) from the top
                const int gb = gi - j;                                     // the checkpoint at its lower end, gb + 1 at its upper end
                const int cc = min(max(c, 0), C - 1);
                auto ck_val = [&](const int gidx) -> int {
                    gptr ck = ckpt + (u64)min(max(gidx, g_lo), g_top) * (u64)FMT::CK_WORDS;
                    if constexpr (FMT::GRP) {
                        gptr rp = ck + (u32)(lane_base + ll) * FMT::CK_LANE;
                        const u32 v = rp[cc];
                        return (int)(float)(half ? hi_of(v) : lo_of(v)) + (int)rp[C + half];   // as materialise_impl's unpack(row[c], grp_base), in units of G
                    } else {
                        // the two-task format: lane-major rows of PATTERNS, the bases behind them as [task][lane] -- as materialise_impl's
                        // unpack(raw[c], ckbase) for PK, LPT == 64 (img_load<C, true> + pat_decode), in units of G; the top blocks store
                        // through h2_to_pat, so every row reads the same way
                        const u32 v = ck[(u32)ll * FMT::CK_LANE + cc];
                        return pat_decode(half ? v >> 16 : v & 0xFFFFu) + (int)ck[FMT::CK_ROWS + half * 64 + ll];
                    }
                };
                const int g_bot = ck_val(gb), g_up = ck_val(gb + 1);
                const int ia_lo = a_base + pos - off - 63, ib_lo = bb_base + x - off - 63;   // base p of the span's 64 (0 = lowest row)
                u32 aw[5], bw[5];
#pragma unroll
                for (int k = 0; k < 5; ++k) { aw[k] = a2[(ia_lo >> 4) + k]; bw[k] = b2[(ib_lo >> 4) + k]; }
                // the upper value: the score at the end cell, else the checkpoint row the walk stands on (a full span of 64)
                const bool at_start = len == 0u;
                const bool up_ok = (j == 0) ? (at_start || (d0 == 64 && gi + 1 <= g_top)) : true;
                const int g_top_val = (j == 0 && at_start) ? w0.best + 16 * x + 8 * y : g_up;
                const int p0 = 64 - cnt;                                    // lane 0: the top d0 bases only
                u32 eq[4];
                int m = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const u32 a16 = __builtin_amdgcn_alignbit(aw[k + 1], aw[k], (u32)(ia_lo & 15) * 2u), b16 = __builtin_amdgcn_alignbit(bw[k + 1], bw[k], (u32)(ib_lo & 15) * 2u);
                    const u32 xr = a16 ^ b16, ne = (xr | (xr >> 1)) & 0x55555555u;
                    const int q0 = p0 - 16 * k;
                    const u32 msk = (q0 <= 0) ? 0x55555555u : ((q0 >= 16) ? 0u : (0x55555555u << (2 * q0)));
                    eq[k] = ~ne & msk;
                    m += __builtin_popcount(eq[k]);
                }
                // every cell of the span is an else-branch cell of the fill (x >= 2, pos >= 2 above the cell it ends on, which
                // keeps x >= 1, pos >= 1: row 0 and pos == 0 stay with finish_walk), both checkpoint rows exist
                const bool tested = cand && up_ok && gb >= g_lo && x - (off + cnt) >= 1 && pos - (off + cnt) >= 1;
                const bool pass = tested && g_top_val - g_bot == 12 * cnt + 9 * m;
                const u32 gm_pass = (u32)(__ballot(pass) >> (8 * g)) & 0xFFu, gm_tested = (u32)(__ballot(tested) >> (8 * g)) & 0xFFu;
                const int k = __builtin_ctz(~gm_pass | 0x100u);            // the passing prefix
                const bool inc = j < k;
                {
                    int cnt_m = inc ? m : 0;
                    cnt_m += __builtin_amdgcn_update_dpp(0, cnt_m, 0xB1, 0xf, 0xf, true);
                    cnt_m += __builtin_amdgcn_update_dpp(0, cnt_m, 0x4E, 0xf, 0xf, true);
                    cnt_m += __builtin_amdgcn_update_dpp(0, cnt_m, 0x141, 0xf, 0xf, true);
                    nm += (u32)cnt_m;
                }
                {
                    int ptop = 0, pbot = 0;
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) if (eq[kk]) ptop = 16 * kk + ((31 - __builtin_clz(eq[kk])) >> 1);
#pragma unroll
                    for (int kk = 3; kk >= 0; --kk) if (eq[kk]) pbot = 16 * kk + (__builtin_ctz(eq[kk]) >> 1);
                    const u32 gm_eq = (u32)(__ballot(inc && m > 0) >> (8 * g)) & 0xFFu;
                    const int Ltop = gm_eq ? __builtin_ctz(gm_eq) : 0, Lbot = gm_eq ? 31 - __builtin_clz(gm_eq) : 0;
                    const int off_hi = __builtin_amdgcn_ds_bpermute(4 * (8 * g + Ltop), off + 63 - ptop);   // steps below the walk
                    const int off_lo = __builtin_amdgcn_ds_bpermute(4 * (8 * g + Lbot), off + 63 - pbot);
                    if (gm_eq) {
                        if (!(have & 2)) { have |= 2; la = pos - off_hi; lb = begin_b + x - off_hi; }
                        have |= 1; fa = pos - off_lo; fb = begin_b + x - off_lo;
                    }
                }
                if (cand) {
                    sk_tests++; sk_tested += (u32)__builtin_popcount(gm_tested); sk_groups += (u32)k;
                    if (k > 0) {
                        const int n = d0 + 64 * (k - 1);
                        x -= n; pos -= n; len += (u32)n;
                        sk_short += (u32)(64 - d0);
                        if (backoff) bo = 0u;
                    } else {
                        stuck = true;
                        if (backoff) bo = walk_backoff_after_fail(bo);
                    }
                }
                if (__ballot(cand && k > 0) != 0) continue;   // round again: the next test, directions, or a task that has dropped out
            }
        }
        if (m_need != 0 || __ballot(active) == 0) break;
        // ---- this lane's direction word and the packed bases of its 16 steps: all loads in flight together
        const int myblk = blk0 - j;
        const bool mine = active && myblk >= max(vlo, 0);
        const u32 W = dir[dir_index<C, true>(max(myblk, 0), lane_base + ll, c)];
        const int ia_hi = a_base + pos, ib_hi = bb_base + x;
        const int ia_lo = ia_hi - 15 - 16 * j, ib_lo = ib_hi - 15 - 16 * j;   // steps [16j, 16j + 15] from the top
        const u32 a_w0 = a2[ia_lo >> 4], a_w1 = a2[(ia_lo >> 4) + 1], b_w0 = b2[ib_lo >> 4], b_w1 = b2[(ib_lo >> 4) + 1];
        // ---- length of the diagonal run
        u32 T = W ^ 0xAAAAAAAAu;               // a diagonal step reads 00
        if (j == 0) T <<= (30 - 2 * r);        // the block the walk stands in: row r on top
        const int avail = T ? (__builtin_clz(T) >> 1) : ((j == 0) ? r + 1 : 16);
        const u64 m_mine = __ballot(mine), m_stop = __ballot(mine && T != 0u);
        const u32 gm_mine = (u32)(m_mine >> (8 * g)) & 0xFFu, gm_stop = (u32)(m_stop >> (8 * g)) & 0xFFu;
        const int js = gm_stop ? __builtin_ctz(gm_stop) : -1;   // the lane of the group where the run ends
        const int lead = __builtin_amdgcn_ds_bpermute(4 * (8 * g + max(js, 0)), avail);
        int n;
        if (js < 0) n = (r + 1) + 16 * (gm_mine ? 31 - __builtin_clz(gm_mine) : 0);
        else n = (js == 0) ? lead : (r + 1) + 16 * (js - 1) + lead;
        const int n_run = n;
        n = min(n, min(x, pos));  // stay in x >= 1, pos >= 1
        if (!active) n = 0;
        // ---- matches among the n steps
        const u32 a16 = __builtin_amdgcn_alignbit(a_w1, a_w0, (u32)(ia_lo & 15) * 2u), b16 = __builtin_amdgcn_alignbit(b_w1, b_w0, (u32)(ib_lo & 15) * 2u);
        const u32 xr = a16 ^ b16;
        const u32 ne = (xr | (xr >> 1)) & 0x55555555u;  // bit 2p set: bases p differ
        const int p0 = 16 * j + 16 - n;                 // first base of the chunk that still belongs to the run
        const u32 msk = (p0 <= 0) ? 0x55555555u : ((p0 >= 16) ? 0u : (0x55555555u << (2 * p0)));
        const u32 eq = ~ne & msk;
        const u64 m_eq = __ballot(eq != 0u);
        const u32 gm_eq = (u32)(m_eq >> (8 * g)) & 0xFFu;
        {
            int cnt = __builtin_popcount(eq);
            cnt += __builtin_amdgcn_update_dpp(0, cnt, 0xB1, 0xf, 0xf, true);   // quad_perm:[1,0,3,2]
            cnt += __builtin_amdgcn_update_dpp(0, cnt, 0x4E, 0xf, 0xf, true);   // quad_perm:[2,3,0,1]
            cnt += __builtin_amdgcn_update_dpp(0, cnt, 0x141, 0xf, 0xf, true);  // row_half_mirror: every lane = its group's sum
            nm += (u32)cnt;
        }
        {
            const int Ltop = gm_eq ? __builtin_ctz(gm_eq) : 0, Lbot = gm_eq ? 31 - __builtin_clz(gm_eq) : 0;
            const u32 eq_top = (u32)__builtin_amdgcn_ds_bpermute(4 * (8 * g + Ltop), (int)eq), eq_bot = (u32)__builtin_amdgcn_ds_bpermute(4 * (8 * g + Lbot), (int)eq);
            if (gm_eq) {
                const int off_hi = 16 * Ltop + 15 - ((31 - __builtin_clz(eq_top)) >> 1);  // steps below the top of the run
                const int off_lo = 16 * Lbot + 15 - (__builtin_ctz(eq_bot) >> 1);
                if (!(have & 2)) { have |= 2; la = pos - off_hi; lb = begin_b + x - off_hi; }
                have |= 1; fa = pos - off_lo; fb = begin_b + x - off_lo;
            }
        }
        // ---- advance; then the gap: the one that ended the run (its word is in lane js), or the one the walk stands on
        const u32 w_gap = (u32)__builtin_amdgcn_ds_bpermute(4 * (8 * g + ((n > 0) ? max(js, 0) : 0)), (int)W);
        if (active) {
            bool gap = false;
            if (n > 0) {
                x -= n; pos -= n; len += (u32)n;
                gap = js >= 0 && n == n_run && x >= 1 && pos >= 1;
            } else gap = true;
            if (gap) {
                const u32 tag = (w_gap >> (((x + ll) & 15) * 2)) & 3u;
                if (tag == 1u) {  // GAP_A: consumes b
                    x--; y++;
                    if (++c == C) { c = 0; l++; }
                } else {          // GAP_B: consumes a
                    y--; pos--;
                    if (--c < 0) { c = C - 1; l--; }
                }
                len++;
            }
        }
    }
    if (m_need == 0) break;
    if constexpr (LPT == 64 && SKIP) {
        // back to the caller (walk_pair_skip below) for the strips, as with a task per DPP row: this instance makes no call, so it
        // saves no registers around one and has no frame of its own.  The carries are one copy per lane: every lane stores the same.
#pragma unroll
        for (int s = 0; s < NT; ++s) {
            WalkCarry& w = wcs[s];
            const int L0 = 8 * s;
            w.x = __builtin_amdgcn_readlane(x, L0); w.y = __builtin_amdgcn_readlane(y, L0); w.pos = __builtin_amdgcn_readlane(pos, L0);
            w.len = (u32)__builtin_amdgcn_readlane((int)len, L0); w.nm = (u32)__builtin_amdgcn_readlane((int)nm, L0);
            w.la = __builtin_amdgcn_readlane(la, L0); w.lb = __builtin_amdgcn_readlane(lb, L0);
            w.fa = __builtin_amdgcn_readlane(fa, L0); w.fb = __builtin_amdgcn_readlane(fb, L0); w.have = __builtin_amdgcn_readlane(have, L0);
            w.mat_q = __builtin_amdgcn_readlane(mat_q, L0); w.mat_lo = __builtin_amdgcn_readlane(mat_lo, L0); w.mat_hi = __builtin_amdgcn_readlane(mat_hi, L0);
            w.old_q = __builtin_amdgcn_readlane(old_q, L0); w.old_lo = __builtin_amdgcn_readlane(old_lo, L0); w.old_hi = __builtin_amdgcn_readlane(old_hi, L0);
            w.mat_calls = __builtin_amdgcn_readlane(mat_calls, L0);
            w.need_q = __builtin_amdgcn_readlane(strip, L0); w.need_ghi = __builtin_amdgcn_readlane(blk0 >> 2, L0);
            w.early_seq = __builtin_amdgcn_readlane((int)bo, L0);
        }
        count_skips();
        u32 need = 0;
#pragma unroll
        for (int s = 0; s < NT; ++s) need |= ((m_need >> (8 * s)) & 0xFFull) ? (1u << s) : 0u;
        return need;
    } else
    if constexpr (LPT != 64) {
        // back to the caller for the strips: the first lane of every group stores its task's state (uniform within the group)
        if (j == 0 && g < NT) {
            WalkCarry& w = wcs[gt];
            w.x = x; w.y = y; w.pos = pos; w.len = len; w.nm = nm;
            w.la = la; w.lb = lb; w.fa = fa; w.fb = fb; w.have = have;
            w.mat_q = mat_q; w.mat_lo = mat_lo; w.mat_hi = mat_hi; w.old_q = old_q; w.old_lo = old_lo; w.old_hi = old_hi;
            w.mat_calls = mat_calls;
            w.need_q = strip; w.need_ghi = blk0 >> 2;
            if constexpr (SKIP) w.early_seq = (int)bo;
        }
        count_skips();
        u32 need = 0;
#pragma unroll
        for (int s = 0; s < NT; ++s) need |= ((m_need >> (8 * s)) & 0xFFull) ? (1u << s) : 0u;
        return need;
    }
    // ---- the strips that are asked for, one task at a time with the whole wavefront on it
    if constexpr (!SKIP)
    while (m_need != 0) {
        const int first = __builtin_ctzll(m_need), sel = first >> 3;
        const int q_s = __builtin_amdgcn_readlane(strip, first), ghi_s = __builtin_amdgcn_readlane(blk0 >> 2, first);
        {
            const int hsel = (LPT == 64) ? sel : sel >> 2;
            const Tk* const tsp = (LPT == 64) ? (hsel ? tbq : tap) : tks + sel;
            materialise_auto<C, CE, HASN, LPT, PK>(tsp, q_s, ghi_s, lane, hsel, (LPT == 64) ? 0 : QL * (sel & 3));
        }
        // the loads of the walk must see those stores: wait until L2 has them, then drop this CU's L1 lines
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        if (g == sel) {
            old_q = mat_q; old_lo = mat_lo; old_hi = mat_hi;
            mat_q = q_s; mat_hi = 4 * ghi_s + 3; mat_lo = max(4 * (ghi_s - (ST::groups_of(q_s) - 1)), df_lo);
            mat_calls++;
        }
        m_need &= ~(0xFFull << (8 * sel));
    }
    }
    // every task's state goes back into its carry (one copy per wavefront: in LDS with a task per DPP row, in the caller's frame else)
    if constexpr (LPT != 64) {
        if (j == 0 && g < NT) {
            WalkCarry& w = wcs[gt];
            w.x = x; w.y = y; w.pos = pos; w.len = len; w.nm = nm;
            w.la = la; w.lb = lb; w.fa = fa; w.fb = fb; w.have = have;
            w.mat_q = mat_q; w.mat_lo = mat_lo; w.mat_hi = mat_hi; w.old_q = old_q; w.old_lo = old_lo; w.old_hi = old_hi;
            w.mat_calls = mat_calls;
            if constexpr (SKIP) w.early_seq = (int)bo;
        }
        count_skips();
        return 0u;
    }
    count_skips();
#pragma unroll
    for (int s = 0; s < NT; ++s) {
        WalkCarry& w = wcs[s];
        const int L0 = 8 * s;
        w.x = __builtin_amdgcn_readlane(x, L0); w.y = __builtin_amdgcn_readlane(y, L0); w.pos = __builtin_amdgcn_readlane(pos, L0);
        w.len = (u32)__builtin_amdgcn_readlane((int)len, L0); w.nm = (u32)__builtin_amdgcn_readlane((int)nm, L0);
        w.la = __builtin_amdgcn_readlane(la, L0); w.lb = __builtin_amdgcn_readlane(lb, L0);
        w.fa = __builtin_amdgcn_readlane(fa, L0); w.fb = __builtin_amdgcn_readlane(fb, L0); w.have = __builtin_amdgcn_readlane(have, L0);
        w.mat_q = __builtin_amdgcn_readlane(mat_q, L0); w.mat_lo = __builtin_amdgcn_readlane(mat_lo, L0); w.mat_hi = __builtin_amdgcn_readlane(mat_hi, L0);
        w.old_q = __builtin_amdgcn_readlane(old_q, L0); w.old_lo = __builtin_amdgcn_readlane(old_lo, L0); w.old_hi = __builtin_amdgcn_readlane(old_hi, L0);
        w.mat_calls = __builtin_amdgcn_readlane(mat_calls, L0);
        if constexpr (SKIP) w.early_seq = __builtin_amdgcn_readlane((int)bo, L0);
    }
    return 0u;
}

// The side-by-side walks of the two-task kernel with the diagonal test (LP_WALK_SKIP_PAIR): walk_many<..., 2, 64, SKIP> returns for its
// strips and they are made here, one task at a time with the whole wavefront on it -- what finish_many does in the kernel itself for the
// eight-task kernel.  Out of line: the kernel's own code and frame are what they were without the test, and nothing of the walks is in
// registers while a strip is made.  (pp, not its stats pointer: a value of *pp that the kernel hands over is one more register it
// keeps across its calls.)
template <int C, int CE>
__device__ __noinline__ void walk_pair_skip(const Tk* tap, const Tk* tbp, WalkCarry* wcs, const int skip_mask, const int lane, const LaunchParams* pp)
{
    typedef Strip<64, true> ST;
    u32* const skip_stats = unip(unip(pp)->stats);
    const int mask = skip_mask | ((uni((int)unip(pp)->flags) & (int)LP_WALK_SKIP_BACKOFF) ? WM_BACKOFF : 0);
    for (;;) {
        const u32 need = (u32)uni((int)walk_many<C, CE, false, true, 2, 64, true>(tap, tbp, wcs, mask, lane, nullptr, skip_stats));
        if (need == 0) break;
#pragma unroll 1
        for (u32 rest = need; rest != 0; rest &= rest - 1) {
            const int s = __builtin_ctz(rest);
            const Tk* const tsp = s ? tbp : tap;
            const int q_s = uni(wcs[s].need_q), ghi_s = uni(wcs[s].need_ghi);
            materialise_auto<C, CE, false, 64, true>(tsp, q_s, ghi_s, lane, s, 0);
            // the loads of the walk must see those stores: wait until L2 has them, then drop this CU's L1 lines
            __builtin_amdgcn_s_waitcnt(0);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            WalkCarry& w = wcs[s];   // (one copy per lane, wave-uniform values)
            w.old_q = w.mat_q; w.old_lo = w.mat_lo; w.old_hi = w.mat_hi;
            w.mat_q = q_s; w.mat_hi = 4 * ghi_s + 3; w.mat_lo = max(4 * (ghi_s - (ST::groups_of(q_s) - 1)), uni(tsp->df_lo));
            w.mat_calls++;
        }
    }
}
