// Part of gamdp_kernel.hip (included inside namespace gamdp::{anonymous}): materialise(): the direction words of a strip of 2, 4 or 8 lanes, re-created on demand for the walk.

// ---- directions of a strip (SW = 2, 4 or 8 lanes), on demand ----------------------------------------------------
// Re-enacts the SW lanes of strip q (Strip::first_of(q) - sshift on: SW*q - sshift .. with uniform strips) of the sweep over 64/SW
// groups (64 row-times each) at once -- lanes SW*k .. of this
// wavefront do group g_hi-k -- from what do_block_df / pair_range stored, this time with the tagged cell, and writes the
// direction words of those lanes exactly where the tagged fill would have put them.  The walk (finish_walk, walk_many)
// calls it when it enters direction-free blocks whose strip is not there yet; an alignment path drifts sideways only by
// its net indel count, so nearly every call serves 1 000 (4-lane strips) or 2 000 (2-lane strips) rows of path.
// SW: the width of the strip, a template parameter -- the two-task kernel's strips differ in width (PairStripTable, kernel_fill.inc),
// every other kernel's are Strip::SL wide.  Strips are aligned in the call's own lane space (lane & (SW - 1) = the lane's place in
// its strip), whatever sshift says about the fill's lanes.
// (Four tasks per wavefront: q counts strips across the whole wavefront; the lane geometry inside the task is R & 15.  *tp holds
// the values of the task the walk is in, in every lane.)
// PK = the packed stores of the two-task kernels (kernel_pair.inc): f16 pairs relative to per-lane bases; HALF says
// which task of the pair (0 = low halves).  Converted to the int32 G4 values on the way in; everything after that is
// the same sweep.
// TOP: some of the groups hold packed top blocks (pair_top_range): the pos == -1 cell of a row is forced to H = 0 after it has
// been computed, exactly as do_block<M_TOP> does it (the cells further left hold whatever: they only ever feed each other).
// Strips begin sshift lanes before where Strip::first_of puts them (a multiple of SL with uniform strips): the first and the last strip of a task then have lanes
// that belong to the task next door or to nobody.  lane_base_ = the task's first wavefront lane; such a lane re-enacts its
// neighbour inside the task once more and stores nothing; the task's first lane takes NEG from its left as in the fill (its
// outside neighbour does not stay dead: it takes that lane's column 0 as an `up` source), its last lane may take anything from
// its right (that feeds the columns behind the band's last one only, whose way back is cut at column CE of lane LE).
// HALF (PK only): which task of the pair, compile-time -- the half-word select of every conversion is then part of the conversion.
template <int C, int CE, bool HASN, int LPT = 64, bool PK = false, bool TOP = false, int HALF = 0, int SW = Strip<LPT, PK>::SL>
__device__ __forceinline__ void materialise_impl(const Tk* tp, const int q_, const int g_hi_, const int lane, const int lane_base_ = 0)
{
    static_assert((CE < 0 || CE < C - 1) && C - 1 <= 32, "the edge column inside a lane (tuned kernels) or a runtime one (CE < 0: the generic kernels)");
    // CE == -1: the strip holds the lane with the band's last column (and maybe dead lanes behind it): a select per cell and on the
    // hand-off; CE == -2: every lane of the strip lies left of that lane -- no edge at all in here (materialise_auto picks)
    constexpr bool RT_EDGE = (CE == -1);
    constexpr int HR = 8;  // row-times per unrolled chunk
    typedef Strip<LPT, PK> ST;
    static_assert(SW >= ST::WMIN && SW <= ST::WMAX && (SW == 2 || SW == 4 || SW == 8), "a width this kernel's strips have");
    constexpr int SWLOG = (SW == 8) ? 3 : ((SW == 4) ? 2 : 1);
    constexpr int NB = ST::NB;        // boundary slots per row-time
    constexpr int NG = 64 / SW;       // groups per call
    constexpr u32 BND_WORDS = ST::BND_WORDS;
    const Tk t = load_uniform(tp);
    const int q = uni(q_), g_hi = uni(g_hi_);
    const int lam = lane & (SW - 1);
    const int lane_base = (LPT == 64) ? 0 : uni(lane_base_);
    const int Rw0 = ST::first_of(q) + lam - t.sshift;
    const bool real = Rw0 >= lane_base && Rw0 < lane_base + LPT;
    const int Rw = min(max(Rw0, lane_base), lane_base + LPT - 1);   // the wavefront lane of the fill this lane re-enacts (where its words live)
    const int R = Rw & (LPT - 1);     // ... and its lane within the task (which columns, which rows)
    const int g_first = t.df_lo >> 2;
    const int g = g_hi - (lane >> SWLOG);
    const bool live = g >= g_first;
    const int gg = live ? g : g_first;  // lanes beyond the range redo the first group and store nothing
    const int LE = (t.Y - 1) / C;

    int Lp[C];
    u32 acc[C];
    u32 W[C - 1 + HR];
    u32 sv[HR];
    static_assert(PK || HALF == 0, "HALF is the task of a packed pair");
    constexpr int half = HALF;
    // packed f16 pair -> G4 of this task, branch-free (a branch per row made the loop spill): -inf ("no source": what
    // lane 0 of the band receives, the rows of dead lanes) is clamped to -2^27, which as a G4 value (about -2^29) loses
    // every comparison against a live value just like NEG does; +inf / NaN only ever sit in dead cells.
    // Two-task kernel (LPT == 64): the slot holds patterns (kernel_pair.inc, the pattern format), read as SIGNED 16-bit: a bit-field
    // extract and an add.  A live value decodes exactly.  A "no source" word has the top bit set -- 0xFC00 from the plain ranges,
    // the clamped -inf of the top blocks -- and decodes at least 9 000 below the base of the lane that stored it, when the live
    // values of that lane and of its neighbours lie within ~2 000 of it: it loses every comparison against them, as NEG does.
    // (Where it must lose against everything -- the stream right of the task's last lane -- the base is NEG_BASE.)
    auto unpack = [&](const u32 v, const int base) -> int {
        if constexpr (PK && LPT == 64) {
            return 4 * (pat_decode(HALF ? v >> 16 : v & 0xFFFFu) + base);
        }
        const float f = __builtin_amdgcn_fmed3f((float)(HALF ? hi_of(v) : lo_of(v)), -134217728.0f, 134217728.0f);
        return 4 * ((int)f + base);
    };
    int grp_base = 0, grp_rbase = 0;   // GRP (eight-task kernel): the bases everything this lane's fill lane / its right neighbour stored of the group is relative to
    {
        gptr ck = t.ckpt + (u64)gg * (u64)(PK ? PairFmt<C, LPT>::CK_WORDS : IMG_WORDS<C, true>);
        u32 raw[C];
        if constexpr (PK && PairFmt<C, LPT>::GRP) {
            // the lane's checkpoint row: C packed values, then its bases (A, B) and its right neighbour's (PairFmt): 96 B in one piece
            u32 row[24];
            gptr rp = ck + (u32)Rw * PairFmt<C, LPT>::CK_LANE;
#pragma unroll
            for (int g = 0; g < 6; ++g) {
                const u32x4 q = *(g4ptr)(rp + 4 * g);
                row[4 * g] = q.x; row[4 * g + 1] = q.y; row[4 * g + 2] = q.z; row[4 * g + 3] = q.w;
            }
            grp_base = (int)row[C + half];
            grp_rbase = (int)row[C + 2 + half];
#pragma unroll
            for (int c = 0; c < C; ++c) Lp[c] = unpack(row[c], grp_base);
        } else {
            img_load<C, true>(ck, Rw, raw);
            if constexpr (PK) {
                const int ckbase = (int)ck[PairFmt<C, LPT>::CK_ROWS + half * 64 + Rw];
#pragma unroll
                for (int c = 0; c < C; ++c) Lp[c] = unpack(raw[c], ckbase);
            } else {
#pragma unroll
                for (int c = 0; c < C; ++c) Lp[c] = (int)raw[c];
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 0;
    }
    // quad shifts: lane lam <- lam-1 / lam+1 of the same strip (the strip's outer lanes take the stored values); 8 lanes: a row
    // shift by one (what a strip's outer lanes get from the strip next door, or keep at a row's end, is not used)
    auto from_left = [](int v) { return __builtin_amdgcn_update_dpp(v, v, SW == 8 ? 0x111 : (SW == 4 ? 0x90 : 0xA0), 0xf, 0xf, false); };   // row_shr:1 | quad_perm:[0,0,1,2] | [0,0,2,2]
    auto from_right = [](int v) { return __builtin_amdgcn_update_dpp(v, v, SW == 8 ? 0x101 : (SW == 4 ? 0xF9 : 0xF5), 0xf, 0xf, false); };  // row_shl:1 | quad_perm:[1,2,3,3] | [1,1,3,3]
    int Lin = from_left(Lp[C - 1]);  // what the left neighbour handed over at the end of the previous row-time
    const int tau_g = gg * 64;
    const int64_t iaW = t.a_base + t.begin_a - t.band + (int64_t)(C - 1) * R + tau_g;  // W[k] <-> a[iaW + k]
    // The bases of the call.  Eight-task kernel (round 5): the 32 groups of a call read 2 x ~540 B of a and b between them, eight
    // bases further per chunk -- as global loads that was ~10 lines requested again every chunk, 8.5 us apart, longer than a line
    // survives in L2 under this kernel's traffic: ~80 of a call's ~390 memory-side requests.  Now the two windows go to LDS once
    // (the staging area behind the tasks' values, idle during the walks) and every chunk reads its words from there.
    constexpr bool SEQ_LDS = PK && !HASN && LPT == QL;
    constexpr int SQW = QB_SEQ_WORDS;      // words per window
    u32* const sqa = s_qbnd + QB_SEQ_AT;   // SQW words of a, then SQW words of b (behind them: the walks' carries, gamdp_kernel.hip finish_many)
    int64_t wa0 = 0, wb0 = 0;              // the global word index of sqa[0] / sqa[SQW]
    if constexpr (SEQ_LDS) {
        const int gmin = max(g_hi - (NG - 1), g_first);
        const int Rlo = min(max(ST::first_of(q) - t.sshift, lane_base), lane_base + LPT - 1) & (LPT - 1);
        const int Rhi = min(max(ST::first_of(q) + (SW - 1) - t.sshift, lane_base), lane_base + LPT - 1) & (LPT - 1);
        wa0 = (t.a_base + t.begin_a - t.band + (int64_t)(C - 1) * Rlo + (int64_t)gmin * 64) >> 4;
        wb0 = (t.b_base + t.begin_b + (int64_t)gmin * 64 - Rhi) >> 4;
        static_assert(NG * 64 + 64 + 2 * (C - 1) + 8 + 32 + 16 <= SQW * 16, "the windows of a call fit SQW words each");
        if (lane < SQW / 4) {
            *(u32x4*)(sqa + 4 * lane) = *(g4ptr)(t.a2 + wa0 + 4 * lane);
            *(u32x4*)(sqa + SQW + 4 * lane) = *(g4ptr)(t.b2 + wb0 + 4 * lane);
        }
    }
    auto seq16 = [&](const bool is_b, const int64_t idx) -> u32 {   // fetch16 of a or b
        if constexpr (SEQ_LDS) {
            const int rel = (int)(idx - ((is_b ? wb0 : wa0) << 4));
            const u32* const p = sqa + (is_b ? SQW : 0) + (rel >> 4);
            return __builtin_amdgcn_alignbit(p[1], p[0], (u32)(rel & 15) * 2u);
        } else return fetch16(is_b ? t.b2 : t.a2, idx);
    };
    {
        const u32 aw = seq16(false, iaW), awn = HASN ? fetch16n(t.an, iaW) : 0u;
        const u32 aw2 = (C - 1 > 16) ? seq16(false, iaW + 16) : 0u, awn2 = (HASN && C - 1 > 16) ? fetch16n(t.an, iaW + 16) : 0u;
#pragma unroll
        for (int k = 0; k < C - 1; ++k)
            W[k] = (k < 16) ? enc_a<HASN>((aw >> (2 * k)) & 3u, HASN && ((awn >> k) & 1u))
                            : enc_a<HASN>((aw2 >> (2 * (k - 16))) & 3u, HASN && ((awn2 >> (k - 16)) & 1u));
    }
    const u32 tagK = (R == LE) ? 0x80000001u : 1u;
    const int kill_c = (RT_EDGE && R == LE) ? (t.Y - 1) % C : -1;   // generic kernels: this lane's column without an `up` source (do_block)
    // the stored boundary values this lane consumes: lam 0 the chain value entering the strip from the left (slot q), lam SW-1 the
    // `up` hand-off entering from the right (the slot of strip q+1; none right of lane 63); the lanes between load the left one and ignore it
    const bool right_edge = lam == SW - 1;
    const bool has_left = R != 0, has_right = R != LPT - 1;  // not the task's first / last lane
    constexpr u32 BLK_STRIDE = PK ? PairFmt<C, LPT>::BND_WORDS : BND_WORDS;   // words per block of the boundary store
    const u32 sq = (u32)((right_edge && has_right) ? q + 1 : q) & (u32)(NB - 1);   // the slot of the lane whose stream this lane consumes
    gptr sp = t.bnd + (u64)gg * (4u * BLK_STRIDE) + ST::offset(0u, (right_edge && has_right) ? 1u : 0u, sq);
    // the stream is loaded 4 row-times (16 B) at a time; t0 = row-time inside the group (a multiple of 4)
    // PK: the values stay packed in sv and are converted row by row with the base of their block (svbase)
    auto load_rows4 = [&](const int t0, const int slot4) {
        const u32x4 v = *(g4ptr)(sp + (u32)(t0 >> 4) * BLK_STRIDE + ST::offset((u32)(t0 & 15), 0u, 0u));
        sv[4 * slot4] = v.x; sv[4 * slot4 + 1] = v.y; sv[4 * slot4 + 2] = v.z; sv[4 * slot4 + 3] = v.w;
    };
    // PK: the stream of the task's last lane when it closes a strip (it has no right neighbour) reads as far below every live value
    const bool dead_stream = PK && right_edge && !has_right;
    auto load_base = [&](const int t0) -> int {  // the base, in the block of row-time t0, of the lane that stored this lane's stream
        if constexpr (PK && PairFmt<C, LPT>::GRP) {
            // one per group: the stream of the strip's left edge was stored by this lane's own fill lane, the right edge's by its right neighbour
            return dead_stream ? NEG_BASE : ((right_edge && has_right) ? grp_rbase : grp_base);
        } else if constexpr (PK) {
            const int b = (int)(t.bnd + (u64)gg * (4u * BLK_STRIDE) + (u32)(t0 >> 4) * BLK_STRIDE)[BND_WORDS + half * NB + sq];
            return dead_stream ? NEG_BASE : b;
        } else return 0;
    };
    int svbase = load_base(0), svbase_nx = svbase;
#pragma unroll
    for (int h = 0; h < HR / 4; ++h) load_rows4(4 * h, h);

    // packed words of the chunk after the current one are requested a chunk ahead (nothing here waits on a load it
    // has just issued)
    const int64_t ia_new = iaW + (C - 1), ib_new = t.b_base + t.begin_b + tau_g - R;
    u32 an_nx = seq16(false, ia_new), bw_nx = seq16(true, ib_new);
    u32 ann_nx = HASN ? fetch16n(t.an, ia_new) : 0u, bwn_nx = HASN ? fetch16n(t.bn, ib_new) : 0u;
    for (int ch = 0; ch < 64 / HR; ++ch) {
        const u32 an = an_nx, bw = bw_nx, ann = ann_nx, bwn = bwn_nx;
        const int nx = min(ch + 1, 64 / HR - 1) * HR;  // the last chunk re-reads itself
        an_nx = seq16(false, ia_new + nx);
        bw_nx = seq16(true, ib_new + nx);
        if (HASN) { ann_nx = fetch16n(t.an, ia_new + nx); bwn_nx = fetch16n(t.bn, ib_new + nx); }
        const int svbase_h = svbase;  // every row of a chunk was stored under the same block
        // TOP: cell (r, c) of the chunk is the pos == -1 cell of its row iff r + c == cm1_0 (per lane: the lanes do different groups)
        const int row0 = tau_g + ch * HR - R;
        const int cm1_0 = TOP ? ((real && R <= LE) ? (t.band - t.begin_a - row0 - 1) - C * R : -1) : 0;   // (a lane outside the task or right of the band's last column forces nothing: it must stay dead -- the fill's own condition, pair_top_range)
        bool is_m1[C + HR - 1];
        if constexpr (TOP) {
#pragma unroll
            for (int k = 0; k < C + HR - 1; ++k) is_m1[k] = (cm1_0 == k);
        }
#pragma unroll
        for (int r = 0; r < HR; ++r) {
            W[C - 1 + r] = enc_a<HASN>((an >> (2 * r)) & 3u, HASN && ((ann >> r) & 1u));
            const u32 brow = enc_b<HASN>((bw >> (2 * r)) & 3u, HASN && ((bwn >> r) & 1u));
            const int s = PK ? unpack(sv[r], svbase_h) : (int)sv[r];
            // (the task's first lane: its neighbour outside the task does not stay dead -- it takes this lane's column 0 as its `up` source)
            int L = !has_left ? NEG : ((lam == 0) ? s : Lin);
            int x = NEG;
            const int Zst = TOP ? 32 * (row0 + r) + 32 * (t.band - t.begin_a - 1) : 0;   // G4 of H = 0 at the pos == -1 cell of this row
            const int ZLst = (TOP && t.fs && row0 + r > FORCE_MAXGAP) ? NEG : Zst;           // ... as a `left` source (force_start: none beyond row 10, banded_smith_waterman.cc:150-155)
            auto cell = [&](const int c) __attribute__((always_inline)) {
                const int D = HASN ? (int)__builtin_amdgcn_udot8(W[r + c], brow, (u32)Lp[c], false)
                                   : (int)__builtin_amdgcn_udot4(W[r + c], brow, (u32)Lp[c], false);
                int Uc = (c < C - 1) ? (int)((u32)Lp[(c < C - 1) ? c + 1 : c] | ((CE >= 0 && c == CE) ? tagK : 1u)) : (x | 1);
                if constexpr (RT_EDGE) Uc = (c == kill_c) ? NEG : Uc;
                const int Rv = imax3(D, Uc, L);
                acc[c] = __builtin_amdgcn_alignbit((u32)Rv, acc[c], 2);
                L = Rv & ~3;
                if constexpr (TOP) {
                    Lp[c] = is_m1[r + c] ? Zst : L;
                    L = is_m1[r + c] ? ZLst : L;
                } else Lp[c] = L;
            };
            cell(0);
            x = from_right(Lp[0]);
            if (right_edge) x = s;
            if constexpr (!PK) x = !has_right ? NEG : x;   // (PK: dead_stream; a neighbour outside the task only feeds the columns behind the band's last)
            if constexpr (RT_EDGE) x = (R >= LE) ? NEG : x;
#pragma unroll
            for (int c = 1; c < C; ++c) cell(c);
            Lin = from_left(L);
            // the same rows of the next chunk: in flight while this chunk computes
            if ((r & 3) == 3) load_rows4(nx + 4 * (r >> 2), r >> 2);
            if (PK && r == 3) svbase_nx = load_base(nx);
            if (r == HR - 1) svbase = svbase_nx;
        }
#pragma unroll
        for (int k = 0; k < C - 1; ++k) W[k] = W[k + HR];
        if ((((ch + 1) * HR) & 15) == 0 && live && real) {  // a block of 16 row-times is complete
            img_store<C, true>(t.dir + (u64)(gg * 4 + ((ch * HR) >> 4)) * (u64)IMG_WORDS<C, true>, Rw, acc);
        }
    }
}

// Out of line: called from inside a walk (finish_walk, and walk_many of the two-task kernel), whose state stays in registers across the
// call -- the calling convention has the callee save the 28 callee-saved registers it needs (14 KB of scratch stored and
// re-loaded per call).
template <int C, int CE, bool HASN, int LPT = 64, bool PK = false, bool TOP = false, int HALF = 0, int SW = Strip<LPT, PK>::SL>
__device__ __noinline__ void materialise(const Tk* tp, const int q, const int g_hi, const int lane, const int lane_base = 0)
{
    materialise_impl<C, CE, HASN, LPT, PK, TOP, HALF, SW>(tp, q, g_hi, lane, lane_base);
}

// the strip the walk asks for: the TOP-aware re-enactment when the groups of the call reach into packed top blocks
// INLINE: the body goes where the call is (the eight-task kernel's strip loop sits in the kernel itself, between two entries of
// walk_many, with nothing of the walks in registers: no register saves at all)
template <int C, int CE, bool HASN, int LPT, bool PK, bool INLINE = false>
__device__ __forceinline__ void materialise_auto(const Tk* tp, const int q, const int g_hi, const int lane, const int half, const int lane_base)
{
    typedef Strip<LPT, PK> ST;
    auto run_w = [&](auto top, auto hf, auto sw) __attribute__((always_inline)) {
        constexpr bool T = decltype(top)::value;
        constexpr int H = decltype(hf)::value, W = decltype(sw)::value;
        if constexpr (INLINE) materialise_impl<C, CE, HASN, LPT, PK, T, H, W>(tp, q, g_hi, lane, lane_base);
        else materialise<C, CE, HASN, LPT, PK, T, H, W>(tp, q, g_hi, lane, lane_base);
    };
    // the strip's width is wave-uniform: one instance per width the kernel's strips have
    auto run = [&](auto top, auto hf) __attribute__((always_inline)) {
        if constexpr (ST::TABLE) {
            const int w = uni(ST::width_of(uni(q)));
            if (w == 2) run_w(top, hf, std::integral_constant<int, 2>{});
            else if (w == 4) run_w(top, hf, std::integral_constant<int, 4>{});
            else run_w(top, hf, std::integral_constant<int, 8>{});
        } else run_w(top, hf, std::integral_constant<int, ST::SL>{});
    };
    typedef std::integral_constant<bool, true> Yes;
    typedef std::integral_constant<bool, false> No;
    typedef std::integral_constant<int, 0> H0;
    typedef std::integral_constant<int, 1> H1;
    if constexpr (PK && !HASN) {
        const int df_lo = uni(tp->df_lo), df_top = uni(tp->df_top);
        const bool top = df_top > df_lo && max(4 * (uni(g_hi) - (ST::groups_of(uni(q)) - 1)), df_lo) < df_top;
        if (uni(half) != 0) {
            if (top) run(Yes{}, H1{});
            else run(No{}, H1{});
        } else {
            if (top) run(Yes{}, H0{});
            else run(No{}, H0{});
        }
    } else if constexpr (CE < 0) {
        // generic kernels (one task per wavefront): the runtime edge only where the strip reaches the lane of the band's last column
        const int LEt = (uni(tp->Y) - 1) / C, last = Strip<LPT, PK>::SL * uni(q) + Strip<LPT, PK>::SL - 1 - uni(tp->sshift);
        if (last >= LEt) {
            if constexpr (INLINE) materialise_impl<C, -1, HASN, LPT, PK, false, 0>(tp, q, g_hi, lane, lane_base);
            else materialise<C, -1, HASN, LPT, PK, false, 0>(tp, q, g_hi, lane, lane_base);
        } else {
            if constexpr (INLINE) materialise_impl<C, -2, HASN, LPT, PK, false, 0>(tp, q, g_hi, lane, lane_base);
            else materialise<C, -2, HASN, LPT, PK, false, 0>(tp, q, g_hi, lane, lane_base);
        }
    } else {
        run(No{}, H0{});
    }
}
