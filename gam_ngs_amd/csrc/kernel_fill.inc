// Part of gamdp_kernel.hip (included inside namespace gamdp::{anonymous}): the fill -- tagged and direction-free blocks of 16 row-times, the out-of-line phase functions, row 0.

// ---- one block of 16 row-times --------------------------------------------------------------------
// MODE bit 0 (TOP): lanes may still be before row 1, cells with pos <= 0 exist (the reference's pos==0 rules).
// MODE bit 1 (END): rows of the pos==end_a anti-diagonal and/or the last row are in the block (side captures).
enum { M_FAST = 0, M_TOP = 1, M_END = 2, M_BOTH = 3 };

// which kernel variants run their fast blocks without directions (do_block_df / materialise): the tuned band-512 ones
// strip geometry of the direction-free kernels: SL lanes wide, boundary values stored for every SL-th lane,
// 64/SL groups re-enacted per materialise() call
// The strip width is a per-kernel choice (all measured with the strip-wise memory layout of kernel_common.inc in place; on
// 98 304 x 50 kb pairs at band 150, 40 960 at band 512).  2 lanes in the eight-task band-150 kernel: re-enacting a 76-column
// strip with the 5-instruction tagged cell cost nearly as much as filling all 301 columns with the packed cell, 38-column
// strips halve that (strips 76 -> 48 ms; the doubled boundary store, flushed every 8 row-times, costs the fill 8 %).  4
// lanes in the other three direction-free kernels, whose int32 / wider boundary stores cost their fills more than the
// halved strips save: four-task int32 kernel -6 %, one-task int32 kernel -18 % with 2 lanes; pair kernel: strips 35 -> 22 ms
// but fill 117 -> 124 ms on 40 960 pairs, +1 % in all (+5 % on launches of two rounds): not worth a second format.
#ifndef GAMDP_STRIP_LANES
#define GAMDP_STRIP_LANES 4
#endif
#ifndef GAMDP_QUAD_STRIP_LANES
#define GAMDP_QUAD_STRIP_LANES 4
#endif
#ifndef GAMDP_PAIR_STRIP_LANES
#define GAMDP_PAIR_STRIP_LANES 4
#endif
#ifndef GAMDP_OCTO_STRIP_LANES
#define GAMDP_OCTO_STRIP_LANES 2
#endif
// The two-task packed kernel (round 7) keeps its 16 boundary slots and makes them the edges of strips of DIFFERENT widths: 2 lanes
// where the alignments run (the band's middle: every call starts on column y = band), 4 and 8 lanes towards the band's outer
// lanes, where no path of the workload goes.  A materialise() call on a 2-lane strip re-enacts 32 groups with the instructions the
// 4-lane call spends on 16; the fill stores what it stored (same slots, same bytes, same flush) -- only WHICH lanes are edges
// changes.  (Uniform 2-lane strips, rounds 3 and 4, needed 32 slots: 4 KB per block, a 4 KB staging area, fill +8 %.)
// -DGAMDP_PAIR_STRIP_TABLE=0 brings the uniform 4-lane strips back (A/B: make pvariant).
#ifndef GAMDP_PAIR_STRIP_TABLE
#define GAMDP_PAIR_STRIP_TABLE 1
#endif
// The table, in u = wavefront lane + Tk::sshift (0 .. 64):  strip   0  1 |  2  3 |  4  5  6  7  8  9 10 11 | 12 13 | 14 15 | (16)
//                                                           first u 0  8 | 16 20 | 24 26 28 30 32 34 36 38 | 40 44 | 48 56 | (64)
//                                                           lanes      8 |     4 |                       2 |     4 |     8 |
// (strip 16 exists with sshift = 1 only: the task's last lane, behind the band's last column; it stores what strip 15 consumes
// from its right, in slot 0 -- which strip 0, whose first lane lies outside the task then, does not use -- and is never made.)
struct PairStripTable {
    static constexpr int N = 16;
    static constexpr __host__ __device__ int first_of(const int q)
    {
        return q < 2 ? 8 * q : (q < 4 ? 16 + 4 * (q - 2) : (q < 12 ? 24 + 2 * (q - 4) : (q < 14 ? 40 + 4 * (q - 12) : 48 + 8 * (q - 14))));
    }
    static constexpr __host__ __device__ int width_of(const int q) { return (q < 2 || q >= 14) ? 8 : ((q < 4 || q >= 12) ? 4 : 2); }
    static constexpr __host__ __device__ int strip_of(const int u)
    {
        return u < 16 ? u >> 3 : (u < 24 ? 2 + ((u - 16) >> 2) : (u < 40 ? 4 + ((u - 24) >> 1) : (u < 48 ? 12 + ((u - 40) >> 2) : 14 + ((u - 48) >> 3))));
    }
    static constexpr bool consistent()
    {
        for (int q = 0; q < N; ++q) {
            const int w = width_of(q);
            if (!(w == 2 || w == 4 || w == 8) || first_of(q) % w != 0 || first_of(q + 1) != first_of(q) + w) return false;   // aligned in a call's lane space, no gaps
            for (int u = first_of(q); u < first_of(q) + w; ++u) if (strip_of(u) != q) return false;
        }
        return first_of(0) == 0 && first_of(N) == 64 && strip_of(64) == N;
    }
};
static_assert(PairStripTable::consistent(), "at most 16 strips of 2, 4 and 8 lanes, every lane in exactly one");

template <int LPT, bool PK = false>
struct Strip {
    static constexpr bool TABLE = PK && LPT == 64 && GAMDP_PAIR_STRIP_TABLE;   // strips of different widths (PairStripTable)
    static constexpr int SL = PK ? ((LPT == 64) ? GAMDP_PAIR_STRIP_LANES : GAMDP_OCTO_STRIP_LANES)
                                 : ((LPT == 64) ? GAMDP_STRIP_LANES : GAMDP_QUAD_STRIP_LANES);  // lanes per strip (TABLE: lanes per boundary slot on average)
    static constexpr int SLOG = (SL == 4) ? 2 : 1;
    static constexpr int NB = 64 / SL;                 // boundaries per row-time (slots); uniform strips: also the groups re-enacted per materialise() call
    static constexpr int WMIN = TABLE ? 2 : SL, WMAX = TABLE ? 8 : SL;   // the widths materialise() is instantiated for
    // boundary words per block: [slot NB][received | handed][row-time 16], where slot q holds what strip q consumes: the
    // values its first lane received from its left neighbour and the values the first lane of strip q+1 handed to ITS left neighbour -- one
    // contiguous piece per strip and block (FI = 16 row-times per flush: a block is ONE piece of [slot][received | handed][16]).
    static constexpr int FI = 16;   // (round 5: the eight-task kernel too flushes once per block -- whole 128 B lines per slot; until then its 2 KB staging area went out every 8 row-times and a strip's 16 row-times of a block lay in two lines)
    static constexpr u32 BND_WORDS = 2u * NB * 16u;
    static_assert(SL == 2 || SL == 4, "strips are 2 or 4 lanes wide");
    static_assert(!TABLE || NB == PairStripTable::N, "the table's strips are the 16 boundary slots of the 4-lane format");
    static __device__ __forceinline__ u32* staging() { return (LPT == 64) ? s_bnd_full : s_qbnd; }
    // Where the strips begin (Tk::sshift = sh, wave-uniform): strip q = wavefront lanes first_of(q) - sh .. + width_of(q) - 1 (uniform
    // strips: SL*q - sh .. SL*q - sh + SL-1), so that
    // the middle of the band -- where an alignment that starts at (begin_a, begin_b) runs, give or take its net indels --
    // lies in the middle of a strip and not, as column 150 of 301 did with 19 columns per lane, two columns from a strip's
    // edge (a walk that keeps changing sides there has both strips re-created for every row).  A strip at the edge of a task
    // has lanes that belong to the neighbouring task or to nobody: materialise() leaves those alone.
    static __device__ __forceinline__ int strip_of(const int wlane, const int sh) { return TABLE ? PairStripTable::strip_of(wlane + sh) : (wlane + sh) >> SLOG; }   // 0 .. NB
    static __device__ __forceinline__ int first_of(const int strip) { return TABLE ? PairStripTable::first_of(strip) : SL * strip; }   // its first lane + sh
    static __device__ __forceinline__ int width_of(const int strip) { return TABLE ? PairStripTable::width_of(strip) : SL; }
    static __device__ __forceinline__ int groups_of(const int strip) { return 64 / width_of(strip); }   // groups re-enacted per materialise() call
    static __device__ __forceinline__ bool opens_strip(const int wlane, const int sh) { return TABLE ? first_of(strip_of(wlane, sh)) == wlane + sh : ((wlane + sh) & (SL - 1)) == 0; }
    static __device__ __forceinline__ u32 slot_of(const int wlane, const int sh) { return (u32)(strip_of(wlane, sh) & (NB - 1)); }   // where the lane that opens a strip stores
    // word offset, inside a block's boundary image, of row-time r (0..15) of half h (0 received, 1 handed) of the lane
    // that opens strip `strip` (its handed values are in the slot of the strip to its left; strip 0's wrap to a slot
    // half nobody reads)
    static __device__ __forceinline__ u32 offset(const u32 r, const u32 h, const u32 strip)
    {
        return (r / FI) * (2u * NB * FI) + ((strip - h) & (u32)(NB - 1)) * (2u * FI) + h * FI + (r % FI);
    }
    // the inverse for the flush: word w of a piece's image lies in the staging area ([received | handed][row-time FI][lane/SL]) at
    static __device__ __forceinline__ u32 staging_index(const u32 w)
    {
        const u32 slot = w / (2u * FI), h = (w % (2u * FI)) / FI, r0 = w % FI;
        return h * (NB * FI) + r0 * NB + ((slot + h) & (u32)(NB - 1));
    }
};
// the shift that puts the band's middle column (y = band, lane band / C) nearest to the middle of its strip
template <int C, int SL>
__device__ __forceinline__ int strip_shift(const int band)
{
    const int cl = band / C, cc = band - cl * C;
    int best = 0, best_d = 1 << 30;
#pragma unroll
    for (int sh = 0; sh < SL; ++sh) {
        const int o = ((cl + sh) & (SL - 1)) * C + cc;      // the middle column's offset inside its strip
        const int d = abs(2 * o - (SL * C - 1));
        if (d < best_d) { best_d = d; best = sh; }
    }
    return best;
}
// ... and for the strips of Strip<LPT, PK>: the table's middle strips are 2 lanes wide, the shift is what puts the middle column mid-strip there
template <int C, int LPT, bool PK>
__device__ __forceinline__ int strip_shift_of(const int band)
{
    typedef Strip<LPT, PK> ST;
    if constexpr (ST::TABLE) {
        static_assert(C == 17, "the table is laid out for band 512 at 17 columns per lane: the middle column in lane 30, strips 2 lanes wide from lane 23 to 38");
        return strip_shift<C, 2>(band);
    } else return strip_shift<C, ST::SL>(band);
}
// (5 columns per lane -- band 150, one task per wavefront -- keeps a direction per cell: a direction-free variant was built and measured
// in round 3 and is not worth a second kernel instance; tools/experiments/instrumentation/ has it as a patch.)
template <int CE, int C, bool HASN>
constexpr bool DIRFREE_OK = (CE < 0 || CE < C - 1) && C - 1 <= 32 && C >= 9;
// (CE < 0: the generic kernels with 9 and 17 columns per lane -- every band from 129 to 543 other than the two tuned ones -- fill
// their fast blocks without directions too since round 5: the band's last column is a runtime (lane, column) pair there, one
// select per cell on a hoisted compare instead of the tuned kernels' free kill in the tag constant.)

// a task's pos0 (0) / adh (1) / lastrow (2) buffer as a capture of do_block addresses it: the pointer itself with one task per
// wavefront (scalar registers); with several, the task's ckpt pointer made uniform + the word offset slow_block left in LDS (s_captab)
template <int LPT>
__device__ __forceinline__ void side_table(const Tk& t, const int wlane)
{
    if constexpr (LPT != 64) {
        if ((wlane & (LPT - 1)) == 0) {
            giptr const base = (giptr)t.ckpt;
            const int4 e = {(int)(t.pos0 - base), (int)(t.adh - base), (int)(t.lastrow - base), 0};
            *reinterpret_cast<int4*>(s_captab[wlane >> 4][0]) = e;
        }
    }
}
template <int LPT>
__device__ __forceinline__ giptr side_buf(const Tk& t, const int wlane, const int which)
{
    if constexpr (LPT == 64) return which == 0 ? t.pos0 : (which == 1 ? t.adh : t.lastrow);
    else return (giptr)unip(t.ckpt) + s_captab[wlane >> 4][0][which];
}

template <int C, int CE, bool HASN, int MODE, int LPT>
__device__ __forceinline__ void do_block(int (&Lp)[C], u32 (&acc)[C], u32 (&W)[C + 15], int& Lin, int& Lout, const Tk& t,
                                         const int blk, const int wlane, const int LE, const int kill_c)
{
    const int tau0 = blk * ROWS;
    const int lane = wlane & (LPT - 1);  // lane within the task: owns band columns [C*lane, C*lane + C)
    typedef Ring<C, LPT, HASN> RG;

    // operands come from the LDS rings: one per-lane address per ring and block, the 16 rows are immediate offsets
    const typename RG::APtr ringA_lane = RG::a_lane(tau0, wlane);  // k = tau0 + r + (C-1)*(lane+1)
    const u32* ringB_lane = RG::b_lane(tau0, wlane);               // k = tau0 + r - lane
    int (*const capbuf)[2][20] = RG::cap(wlane >> 4);

    int xkeep = NEG;  // lane 63's `up` hand-off source does not exist
    const u32 tagK = (CE >= 0 && CE < C - 1 && lane == LE) ? 0x80000001u : 1u;
    // TOP: the pos == -1 cell of a lane moves one column to the left per row, so cell (r, c) is that cell iff r + c
    // equals one per-lane number for the whole block: 32 compares whose lane masks stay in scalar registers, instead
    // of one compare per cell
    bool is_m1[C + ROWS - 1];
    if (MODE & M_TOP) {
        const int cm1_0 = (t.band - t.begin_a - (tau0 - lane) - 1) - C * lane;  // column whose pos == -1 in the block's first row
#pragma unroll
        for (int k = 0; k < C + ROWS - 1; ++k) is_m1[k] = (cm1_0 == k);
    }
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        W[C - 1 + r] = RG::a_read(ringA_lane, r);
        const u32 brow = ringB_lane[r] + (DIRFREE_OK<CE, C, HASN> ? RING_TAG<HASN> : 0u);

        // per-row values of the special modes
        constexpr bool TOP = (MODE & M_TOP) != 0, END = (MODE & M_END) != 0;
        const int row = tau0 + r - lane;
        bool act = true;  // lanes before their row 1 (TOP) or past their last row (END) sit the row out
        int cm1 = 0, Zst = 0, ZL = 0;
        if (END) act = row <= t.X - 1;
        if (TOP) {
            act = act && row >= 1;
            cm1 = (t.band - t.begin_a - row - 1) - C * lane;  // column whose pos == -1
            Zst = 32 * row + 32 * (t.band - t.begin_a - 1);   // G4 of H = 0 at the pos == -1 cell
            ZL = (t.fs && row > FORCE_MAXGAP) ? NEG : Zst;    // ... as a `left` source (:150-155)
        }

        int L = Lin;
        int x;
        // (Computing all diag candidates of the row up front, ahead of the max3 chain, removes the s_nops the
        // compiler pads the dot4 -> VALU hazard with, but measured 3 % slower: the interleaved form below gives
        // each wave independent work between the dependent max3 -> and -> max3 steps.)
        auto cell = [&](const int c) __attribute__((always_inline)) {
            int D;
            if (HASN) D = (int)__builtin_amdgcn_udot8(W[r + c], brow, (u32)Lp[c], false);
            else D = (int)__builtin_amdgcn_udot4(W[r + c], brow, (u32)Lp[c], false);
            // tag the `up` source; the tuned kernels drop the `up` of the last band column (static position CE of
            // lane LE) in the same v_or: tagK also sets the sign bit there (all live G4 values are >= 0)
            int Uc = (c < C - 1) ? (int)((u32)Lp[(c < C - 1) ? c + 1 : c] | ((CE >= 0 && c == CE) ? tagK : 1u)) : (x | 1);
            if (CE < 0) Uc = (c == kill_c) ? NEG : Uc;
            const int R = imax3(D, Uc, L);
            acc[c] = __builtin_amdgcn_alignbit((u32)R, acc[c], 2);
            const int Lc = R & ~3;
            if (TOP) {
                const bool m1 = is_m1[r + c];  // the pos == -1 cell holds H = 0 (the reference's zero-initialised matrix)
                Lp[c] = m1 ? Zst : Lc;
                L = m1 ? ZL : Lc;
            } else {
                Lp[c] = Lc;
                L = Lc;
            }
        };

        if (MODE == M_FAST || act) cell(0);
        x = lane_shl1<LPT>(xkeep, Lp[0]);
        xkeep = x;
        // The last band column has no `up` source.  When it is the last column of lane LE the value arriving
        // from lane LE+1 must be dropped; otherwise (tuned kernels with CE < C-1) column C-1 of lane LE lies
        // outside the band and whatever arrives only feeds dead cells.
        if (CE < 0 || CE == C - 1) x = (lane >= LE) ? NEG : x;
        if (MODE == M_FAST || act) {
#pragma unroll
            for (int c = 1; c < C; ++c) cell(c);
            Lout = L;
        }
        // a lane that sits the row out hands over its last real chain value (its right neighbour is one row behind)
        Lin = lane_shr1<LPT>(Lin, (MODE == M_FAST) ? L : Lout);

        // Side captures.  Every lane works on its own row, and the column of that row's pos==0 (pos==end_a) cell
        // moves by C-1 from lane to lane, so at any row-time at most two ADJACENT lanes hold such a cell.  Those
        // lanes drop their row values into a tiny LDS buffer (one per lane parity) and pick the one they need by
        // index (a dynamic register index would cost a compare + select per cell for every lane).
        if (TOP) {
            const int c0 = cm1 + 1;  // column of the pos == 0 cell
            if (act && row <= t.X - 1 && c0 >= 0 && c0 < C) {
#pragma unroll
                for (int c = 0; c < C; ++c) capbuf[0][lane & 1][c] = Lp[c];
                const int j0 = C * lane + c0;
                if (j0 < t.Y) side_buf<LPT>(t, wlane, 0)[row] = (capbuf[0][lane & 1][c0] >> 2) - 16 * row - 8 * j0;
            }
        }
        if (END) {
            const int cE = (t.eaRel - row) - C * lane;  // column whose pos == end_a
            if (row >= 1 && row <= t.X - 1 && cE >= 0 && cE < C) {
#pragma unroll
                for (int c = 0; c < C; ++c) capbuf[1][lane & 1][c] = Lp[c];
                const int jE = C * lane + cE;
                if (jE < t.Y) side_buf<LPT>(t, wlane, 1)[row - t.iA] = (capbuf[1][lane & 1][cE] >> 2) - 16 * row - 8 * jE;
            }
        }
    }
    if (MODE & M_END) {
        // lanes stopped updating after their last row, so the registers still hold row X-1 when it fell in this block
        const int rX = t.X - 1 - (tau0 - lane);  // position of the lane's last row in this block
        if (t.X > 1 && rX >= 0 && rX < ROWS) {
            giptr const lastrow = side_buf<LPT>(t, wlane, 2);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int j = C * lane + c;
                if (j < t.Y) lastrow[j] = (Lp[c] >> 2) - 16 * (t.X - 1) - 8 * j;
            }
            // the direction words were shifted in from the top one row at a time: a lane that stopped at row rX
            // has its rows 2*(15-rX) bits too high
            const u32 sh = 2u * (u32)(ROWS - 1 - rX);
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] >>= sh;
        }
    }

    // direction words of this block: 16 B / lane coalesced (lane major in the direction-free kernels, whose few tagged
    // blocks share the image layout of their strips)
    {
        constexpr bool LM = DIRFREE_OK<CE, C, HASN>;
        img_store<C, LM>(t.dir + (u64)blk * (u64)IMG_WORDS<C, LM>, wlane, acc);
    }
    // slide the a window
#pragma unroll
    for (int k = 0; k < C - 1; ++k) W[k] = W[k + ROWS];
}

// ---- a tagged fast block as ONE software-pipelined stream -----------------------------------------------------
// do_block<M_FAST> written cell by cell is a chain in which every instruction waits for the one before it (dot4 -> max3 ->
// and -> next cell's max3 ...): a wavefront alone on its SIMD -- a merge-block round, the tail of a short launch -- then issues
// one instruction per ~7.7 cycles instead of ~5.5 (tools/valu_rate6.hip).  Here the two instructions of a cell that do not
// sit on the chain (its dot4 and the `or` that tags its `up` source, both read the PREVIOUS row only) run two cells ahead,
// and the chain (max3, and) and the direction append of cell g are interleaved with them, so that nothing waits for its
// predecessor; sched_barrier keeps the compiler from undoing it.  Same instructions, same operands, same results.
// Tuned kernels only (compile-time edge column); the generic variants keep do_block.
template <int C, int CE, bool HASN, int LPT>
__device__ __forceinline__ void do_block_fast_sp(int (&Lp)[C], u32 (&acc)[C], u32 (&W)[C + 15], int& Lin, int& Lout, const Tk& t,
                                                 const int blk, const int wlane, const int LE)
{
    static_assert(CE >= 0 && C >= 4, "tuned kernels only (the look-ahead of two cells reads columns the current cell has not written: C >= 4)");
    const int tau0 = blk * ROWS;
    const int lane = wlane & (LPT - 1);
    typedef Ring<C, LPT, HASN> RG;
    const typename RG::APtr ringA_lane = RG::a_lane(tau0, wlane);
    const u32* ringB_lane = RG::b_lane(tau0, wlane);
    const u32 tagK = (CE < C - 1 && lane == LE) ? 0x80000001u : 1u;
    constexpr u32 RTAG = DIRFREE_OK<CE, C, HASN> ? RING_TAG<HASN> : 0u;
    // With the edge column inside lane LE (CE < C - 1) the lanes right of LE are dead: what the task's last lane takes in as the
    // `up` source of its last column only ever feeds dead cells, so the hand-off DPP may leave it zero (bound_ctrl) instead of
    // carrying NEG along -- the compiler re-materialised that constant in front of every such DPP, a move and a hazard nop per
    // row-time, and a lone wavefront pays ~5 cycles for every instruction of any kind.
    constexpr bool DEAD_TAIL = CE < C - 1 && LPT == 64;
    int xkeep = NEG;
    u32 brow[4];           // score row of b for row r in [r & 3]; the two LDS operands of rows r + 2, r + 3 are requested at the end of (even) row r
    int D[3], U[3];        // candidates in flight: cell g in [g % 3]
    int L = Lin, Ux = NEG | 1, R = 0;   // Ux: the tagged `up` source of the lane's last column (the neighbour's column 0)
    W[C - 1] = RG::a_read(ringA_lane, 0); W[C] = RG::a_read(ringA_lane, 1);
    brow[0] = ringB_lane[0] + RTAG; brow[1] = ringB_lane[1] + RTAG;
    auto ahead = [&](const int g) __attribute__((always_inline)) {   // dot4 + tag of cell g: previous row's values only (x for a lane's last column comes later)
        const int r = g / C, c = g % C;
        D[g % 3] = HASN ? (int)__builtin_amdgcn_udot8(W[r + c], brow[r & 3], (u32)Lp[c], false) : (int)__builtin_amdgcn_udot4(W[r + c], brow[r & 3], (u32)Lp[c], false);
        if (c < C - 1) U[g % 3] = (int)((u32)Lp[c + 1] | ((c == CE) ? tagK : 1u));
    };
    ahead(0); ahead(1);
    __builtin_amdgcn_sched_barrier(0);
    static_for<ROWS>([&](auto rc) __attribute__((always_inline)) {
        constexpr int r = decltype(rc)::value;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int g = r * C + c;
            if (c == 0) L = Lin;
            const int Uc = (c < C - 1) ? U[g % 3] : Ux;
            R = imax3(D[g % 3], Uc, L);
            if (g + 2 < ROWS * C) ahead(g + 2);
            L = R & ~3;
            Lp[c] = L;
            acc[c] = __builtin_amdgcn_alignbit((u32)R, acc[c], 2);
            if (c == 1) {   // the hand-off of column 0 (the DPP read needs two wait states after the write)
                int x;
                if constexpr (DEAD_TAIL) x = __builtin_amdgcn_update_dpp(0, Lp[0], 0x130, 0xf, 0xf, true);   // wave_shl:1, lane 63 <- 0
                else {
                    x = lane_shl1<LPT>(xkeep, Lp[0]);
                    xkeep = x;
                    if (CE == C - 1) x = (lane >= LE) ? NEG : x;
                }
                Ux = x | 1;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        Lout = L;
        // (between the last cell and the DPP that needs its value: the operand reads of the rows after next)
        if constexpr ((r & 1) == 0 && r + 2 < ROWS) {
            W[C + 1 + r] = RG::a_read(ringA_lane, r + 2); W[C + 2 + r] = RG::a_read(ringA_lane, r + 3);
            brow[(r + 2) & 3] = ringB_lane[r + 2] + RTAG; brow[(r + 3) & 3] = ringB_lane[r + 3] + RTAG;
        }
        Lin = lane_shr1<LPT>(Lin, L);
        __builtin_amdgcn_sched_barrier(0);
    });
    {
        constexpr bool LM = DIRFREE_OK<CE, C, HASN>;
        img_store<C, LM>(t.dir + (u64)blk * (u64)IMG_WORDS<C, LM>, wlane, acc);
    }
#pragma unroll
    for (int k = 0; k < C - 1; ++k) W[k] = W[k + ROWS];
}

// ---- a fast block that keeps no directions ------------------------------------------------------------------
// The traceback reads the directions of the cells on the path only, so the fast blocks of the tuned kernels compute
// plain values -- v_dot4 + v_max3 per cell, no tag, no direction word -- and store what materialise() below needs to
// re-enact a 4-lane strip of the sweep later, with directions, around the path:
//   ckpt: at the start of every 4th block (a "group" = 64 row-times) the live row of every lane;
//   bnd:  every row-time, for every 4th lane, the chain value it received from its left neighbour and the value it
//         hands to that neighbour (its new column 0): [block][received | handed][lane/4 16][row-time 16], written 16 B
//         (four row-times) at a time so that a strip later reads its 16 row-times of a block as one 64 B line.
// Values stay multiples of 4 (what the tagged blocks keep after stripping), so fast and slow blocks mix freely.
template <int C, int CE, bool HASN, bool END, int LPT>
__device__ __forceinline__ void do_block_df(int (&Lp)[C], u32 (&W)[C + 15], int& Lin, int& Lout, const Tk& t, const int blk, const int wlane, const int LE, const int kill_c = -1)
{
    static_assert(CE < 0 || CE < C - 1, "the edge column inside a lane, or a runtime one (kill_c: the lane's column without an `up` source, -1 in every lane but LE)");
    const int tau0 = blk * ROWS;
    const int lane = wlane & (LPT - 1);  // lane within the task
    typedef Ring<C, LPT, HASN> RG;
    const typename RG::APtr ringA_lane = RG::a_lane(tau0, wlane);
    const u32* ringB_lane = RG::b_lane(tau0, wlane);
    if ((blk & 3) == 0) img_store<C, true>(t.ckpt + (u64)(blk >> 2) * (u64)IMG_WORDS<C, true>, wlane, Lp);
    // boundary values go through LDS and leave as one coalesced 2 KB (4 KB with 2-lane strips) store per block: scattered
    // 16 B stores from the edge lanes cost the fill 8 %.  In LDS they lie [received | handed][row-time 16][lane/SL], so the
    // edge lanes of a row-time write consecutive words (the [lane/SL][row-time] order, 64 B apart, was 8- to 16-way bank
    // conflicted); the block-end readout transposes into the order a strip reads, [received | handed][lane/SL][row-time].
    typedef Strip<LPT> ST;
    constexpr int NB = ST::NB;
    constexpr u32 BND_WORDS = ST::BND_WORDS;
    u32* const s_bnd = ST::staging();
    u32* const sb = s_bnd + ST::slot_of(wlane, t.sshift);
    const bool edge = ST::opens_strip(wlane, t.sshift);
    const u32 killK = (lane == LE) ? 0x80000000u : 0u;  // the last band column has no `up` source
    int xkeep = NEG;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        W[C - 1 + r] = RG::a_read(ringA_lane, r);
        const u32 brow = ringB_lane[r];  // untagged in these kernels
        const int Lrecv = Lin;
        int L = Lin, x = NEG;
        auto cell = [&](const int c) __attribute__((always_inline)) {
            const int D = HASN ? (int)__builtin_amdgcn_udot8(W[r + c], brow, (u32)Lp[c], false)
                               : (int)__builtin_amdgcn_udot4(W[r + c], brow, (u32)Lp[c], false);
            int Uc = (c < C - 1) ? Lp[(c < C - 1) ? c + 1 : c] : x;
            if constexpr (CE >= 0) { if (c == CE) Uc = (int)((u32)Uc | killK); }
            else Uc = (c == kill_c) ? NEG : Uc;
            L = imax3(D, Uc, L);
            Lp[c] = L;
        };
        cell(0);
        x = lane_shl1<LPT>(xkeep, Lp[0]);
        xkeep = x;
        if constexpr (CE < 0) x = (lane >= LE) ? NEG : x;   // (the last band column as a lane's last column, and the dead lanes behind it: do_block)
        if (edge) { sb[r * NB] = (u32)Lrecv; sb[16 * NB + r * NB] = (u32)Lp[0]; }
#pragma unroll
        for (int c = 1; c < C; ++c) cell(c);
        Lout = L;
        Lin = lane_shr1<LPT>(Lin, L);
        if (END) {
            // the blocks that hold the last rows / the pos==end_a anti-diagonal: nothing is masked here -- rows past
            // X-1 compute on padding and only ever feed rows past X-1 -- but the values phase C scans are taken as
            // they pass: the last row of this lane, and the anti-diagonal cell (at most two adjacent lanes per
            // row-time, same LDS trick as in do_block)
            const int row = tau0 + r - lane;
            const int cE = (t.eaRel - row) - C * lane;
            if (row >= 1 && row <= t.X - 1 && cE >= 0 && cE < C) {
                int (*const capbuf)[2][20] = RG::cap(wlane >> 4);
#pragma unroll
                for (int c = 0; c < C; ++c) capbuf[1][lane & 1][c] = Lp[c];
                const int jE = C * lane + cE;
                if (jE < t.Y) t.adh[row - t.iA] = (capbuf[1][lane & 1][cE] >> 2) - 16 * row - 8 * jE;
            }
            if (row == t.X - 1) {
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const int j = C * lane + c;
                    if (j < t.Y) t.lastrow[j] = (Lp[c] >> 2) - 16 * (t.X - 1) - 8 * j;
                }
            }
        }
    }
    {
        constexpr u32 PER = BND_WORDS / 64u;  // words per lane: 8 (4-lane strips) or 16 (2-lane strips)
        // lane L sends words [L*PER, L*PER + PER) of the block's image (Strip::offset): consecutive row-times of one
        // slot half
        const u32 w0 = (u32)wlane * PER;
        const u32* src = s_bnd + ST::staging_index(w0);
        gptr bp = t.bnd + (u64)blk * BND_WORDS + w0;
#pragma unroll
        for (u32 k = 0; k < PER; k += 4) {
            const u32x4 v = {src[k * NB], src[(k + 1) * NB], src[(k + 2) * NB], src[(k + 3) * NB]};
            *(g4ptr)(bp + k) = v;
        }
    }
#pragma unroll
    for (int k = 0; k < C - 1; ++k) W[k] = W[k + ROWS];
}

template <int C>
struct BlockState {
    int Lp[C];
    u32 acc[C];
    u32 W[C + 15];
    int Lin;
    int Lout;  // last chain value of the lane's last column (what it hands to its right neighbour)
};

// The fill is driven through three out-of-line functions that hand the per-lane register state over in a
// BlockState (private memory): init_row0 (phase A), slow_block (one block of the top-left triangle / ramp-up /
// anti-diagonal and last-row capture region: 2 % of the blocks of a 50 kb pair) and fast_range (a run of
// consecutive plain blocks -- the hot loop).  Keeping them separate functions gives the hot loop its own
// register allocation: nothing live in the other phases can force a spill (and with it a full
// `s_waitcnt vmcnt(0)` drain of the outstanding direction stores) into it.
template <int C>
__device__ __forceinline__ void load_state(const BlockState<C>* st, int (&Lp)[C], u32 (&acc)[C], u32 (&W)[C + 15], int& Lin, int& Lout)
{
#pragma unroll
    for (int c = 0; c < C; ++c) { Lp[c] = st->Lp[c]; acc[c] = st->acc[c]; }
#pragma unroll
    for (int k = 0; k < C - 1; ++k) W[k] = st->W[k];
#pragma unroll
    for (int k = C - 1; k < C + 15; ++k) W[k] = 0;
    Lin = st->Lin;
    Lout = st->Lout;
}
template <int C>
__device__ __forceinline__ void store_state(BlockState<C>* st, const int (&Lp)[C], const u32 (&acc)[C], const u32 (&W)[C + 15], const int Lin, const int Lout)
{
#pragma unroll
    for (int c = 0; c < C; ++c) { st->Lp[c] = Lp[c]; st->acc[c] = acc[c]; }
#pragma unroll
    for (int k = 0; k < C - 1; ++k) st->W[k] = W[k];
    st->Lin = Lin;
    st->Lout = Lout;
}

// (blk_end_: a run of blocks of one mode in one call -- the state crosses private memory once per call, and what it loads
// waits behind the direction words the block before has just stored)
template <int C, int CE, bool HASN, int MODE, int LPT = 64>
__device__ __noinline__ void slow_block(BlockState<C>* st, const Tk* tp, const int blk_, const int lane, const int blk_end_ = -1)
{
    const Tk t = load_tk<LPT>(tp);
    const int blk_first = uni(blk_), blk_stop = (MODE != M_TOP || blk_end_ < 0) ? blk_first + 1 : uni(blk_end_);   // (runs of top blocks: the ramp of every unit; the END instances spill with a loop around them)
    const int LE = (t.Y - 1) / C;
    const int kill_c = (CE < 0 && (lane & (LPT - 1)) == LE) ? (t.Y - 1) % C : -1;
    int Lp[C];
    u32 acc[C];
    u32 W[C + 15];
    int Lin, Lout;
    load_state<C>(st, Lp, acc, W, Lin, Lout);
    side_table<LPT>(t, lane);
#pragma unroll 1
    for (int blk = blk_first; blk < blk_stop; ++blk) {
    {
        // operands of this block are already in the LDS rings; expand the next block's 16 new bases
        const int T = (blk + 1) * ROWS;
        // four tasks per wavefront: a task that is shorter than its companions keeps stepping until the longest is
        // done; its rows past the last one are never looked at, but what they fetch must stay inside the padding
        const int Tf = (LPT == 64) ? T : min(T, (t.X + 3 * ROWS) & ~(ROWS - 1));
        const int64_t ia = t.a_base + t.begin_a - t.band + Tf + (C - 1) * LPT, ib = t.b_base + t.begin_b + Tf;
        ring_produce<C, HASN, DIRFREE_OK<CE, C, HASN>, LPT>(T, lane, fetch16(t.a2, ia), HASN ? fetch16n(t.an, ia) : 0u, fetch16(t.b2, ib),
                              HASN ? fetch16n(t.bn, ib) : 0u);
    }
    do_block<C, CE, HASN, MODE, LPT>(Lp, acc, W, Lin, Lout, t, blk, lane, LE, kill_c);
    }
    store_state<C>(st, Lp, acc, W, Lin, Lout);
}

// blocks [blk_begin, blk_end) are all "fast": every lane is past row 0, no pos <= 0 cell, no capture row
template <int C, int CE, bool HASN, bool DF, bool END = false, int LPT = 64>
__device__ __noinline__ void fast_range(BlockState<C>* st, const Tk* tp, const int blk_begin_, const int blk_end_, const int lane)
{
    const Tk t = load_tk<LPT>(tp);
    const int blk_begin = uni(blk_begin_), blk_end = uni(blk_end_);
    const int LE = (t.Y - 1) / C;
    const int kill_c = (CE < 0 && (lane & (LPT - 1)) == LE) ? (t.Y - 1) % C : -1;
    int Lp[C];
    u32 acc[C];
    u32 W[C + 15];
    int Lin, Lout;
    load_state<C>(st, Lp, acc, W, Lin, Lout);
    // Invariant: on entry of block T the LDS rings hold everything block T reads; the top of block T expands the 16
    // new bases of block T+16 from packed words that were requested one block earlier (so the hot loop never waits
    // on a load it just issued, and never drains the direction stores in flight).
    const int64_t iA0 = t.a_base + t.begin_a - t.band + (C - 1) * LPT, iB0 = t.b_base + t.begin_b;
    gcptr pa = t.a2 + (iA0 >> 4), pb = t.b2 + (iB0 >> 4);  // one stream per task (wave-uniform with one task), one word per block
    const u32 sha = (u32)(iA0 & 15) * 2u, shb = (u32)(iB0 & 15) * 2u;
    u32 a_lo = pa[blk_begin + 1], a_hi = pa[blk_begin + 2], b_lo = pb[blk_begin + 1], b_hi = pb[blk_begin + 2];
    u32 an_lo = 0, an_hi = 0, bn_lo = 0, bn_hi = 0;
    if (HASN) {
        const int64_t ia = iA0 + (int64_t)(blk_begin + 1) * ROWS, ib = iB0 + (int64_t)(blk_begin + 1) * ROWS;
        an_lo = t.an[ia >> 5]; an_hi = t.an[(ia >> 5) + 1];
        bn_lo = t.bn[ib >> 5]; bn_hi = t.bn[(ib >> 5) + 1];
    }
    asm volatile("" : "+v"(a_lo), "+v"(a_hi), "+v"(b_lo), "+v"(b_hi), "+v"(Lin));
    if (HASN) asm volatile("" : "+v"(an_lo), "+v"(an_hi), "+v"(bn_lo), "+v"(bn_hi));
#pragma unroll
    for (int c = 0; c < C; ++c) asm volatile("" : "+v"(Lp[c]), "+v"(acc[c]));
#pragma unroll
    for (int k = 0; k < C - 1; ++k) asm volatile("" : "+v"(W[k]));
    const int prio_R = uni(t.prio_R), prio_nblk = uni(t.prio_nblk);
    for (int blk = blk_begin; blk < blk_end; ++blk) {
        const int T = (blk + 1) * ROWS;
        if (prio_R != 0 && (blk & 7) == 0) set_prio_by_remaining(prio_nblk - blk, prio_R);
        if ((blk & 7) == 0 && cancelled(t.cancel)) break;   // (a chain twin whose first attempt has settled the chain)
        const u32 a_nx = pa[blk + 3], b_nx = pb[blk + 3];  // words of block blk+2, used at the next iteration
        u32 an_lo_nx = 0, an_hi_nx = 0, bn_lo_nx = 0, bn_hi_nx = 0;
        if (HASN) {
            const int64_t ia = iA0 + T + ROWS, ib = iB0 + T + ROWS;
            an_lo_nx = t.an[ia >> 5]; an_hi_nx = t.an[(ia >> 5) + 1];
            bn_lo_nx = t.bn[ib >> 5]; bn_hi_nx = t.bn[(ib >> 5) + 1];
        }
        u32 anw = 0, bnw = 0;
        if (HASN) {
            anw = __builtin_amdgcn_alignbit(an_hi, an_lo, (u32)((iA0 + T) & 31)) & 0xFFFFu;
            bnw = __builtin_amdgcn_alignbit(bn_hi, bn_lo, (u32)((iB0 + T) & 31)) & 0xFFFFu;
        }
        ring_produce<C, HASN, DIRFREE_OK<CE, C, HASN>, LPT>(T, lane, __builtin_amdgcn_alignbit(a_hi, a_lo, sha), anw,
                              __builtin_amdgcn_alignbit(b_hi, b_lo, shb), bnw);
        if constexpr (DF) {
            do_block_df<C, CE, HASN, END, LPT>(Lp, W, Lin, Lout, t, blk, lane, LE, kill_c);
        }
        else if constexpr (CE >= 0 && C >= 4) do_block_fast_sp<C, CE, HASN, LPT>(Lp, acc, W, Lin, Lout, t, blk, lane, LE);
        else do_block<C, CE, HASN, M_FAST, LPT>(Lp, acc, W, Lin, Lout, t, blk, lane, LE, kill_c);
        a_lo = a_hi; a_hi = a_nx; b_lo = b_hi; b_hi = b_nx;
        if (HASN) { an_lo = an_lo_nx; an_hi = an_hi_nx; bn_lo = bn_lo_nx; bn_hi = bn_hi_nx; }
    }
    store_state<C>(st, Lp, acc, W, Lin, Lout);
}

// ---- phase A: row 0 -----------------------------------------------------------------------------------
template <int C, bool HASN, bool UNTAGGED, int LPT = 64>
__device__ __noinline__ void init_row0(BlockState<C>* st, const Tk* tp, const int wlane)
{
    const Tk t = load_tk<LPT>(tp);
    const int lane = wlane & (LPT - 1);  // lane within the task
    const int Y = t.Y, w = t.band;
    const int LE = (Y - 1) / C;
#ifdef GAMDP_DIAG
    if (lane == 0) t.pos0[-1] = 0;   // the range-assertion mark of this task (the spare word behind the row-0 buffer, kernel_pair.inc)
#endif
    // row 0 (:112-132): running max without gap penalty along j
    int Lp[C];
    u32 acc[C];
    u32 W[C + 15];
    int Lin = NEG, Lout = NEG;
    {
        const int cb0 = code_at(t.b2, t.bn, t.b_base + t.begin_b);
        int e[C];
        bool q[C];
        int run = NEG;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int j = C * lane + c;
            const int pos = t.begin_a - w + j;
            q[c] = (j < Y) && pos >= 0 && pos < t.alen;  // host guarantees force_start never needs pos >= alen
            int v = NEG;
            if (q[c]) {
                const int d = score_of(code_at(t.a2, t.an, t.a_base + pos), cb0);
                v = (t.fs && pos > FORCE_MAXGAP) ? d : max(d, GAP);
            }
            run = max(run, v);
            e[c] = run;
        }
        // exclusive max-scan of lane totals
        int incl = run;
#pragma unroll
        for (int o = 1; o < LPT; o <<= 1) {
            const int up = __shfl_up(incl, o, LPT);
            if (lane >= o) incl = max(incl, up);
        }
        int pre = __shfl_up(incl, 1, LPT);
        if (lane == 0) pre = NEG;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int j = C * lane + c;
            const int h = q[c] ? max(pre, e[c]) : 0;
            if (j < Y) t.h0row[j] = h;
            Lp[c] = (j < Y) ? 4 * (h + 8 * j) : NEG;
            acc[c] = 0;
        }
        if (lane > LE) {
#pragma unroll
            for (int c = 0; c < C; ++c) Lp[c] = NEG;
        }
        // a window for row-time 0: W[k] <-> a index begin_a - band + (C-1)*lane + k , k < C-1
        const int64_t s0 = t.a_base + t.begin_a - w + (int64_t)(C - 1) * lane;
        const u32 ab = fetch16(t.a2, s0), ab2 = (C - 1 > 16) ? fetch16(t.a2, s0 + 16) : 0u;
        const u32 an = HASN ? fetch16n(t.an, s0) : 0u, an2 = (HASN && C - 1 > 16) ? fetch16n(t.an, s0 + 16) : 0u;
#pragma unroll
        for (int k = 0; k < C - 1; ++k) {
            W[k] = (k < 16) ? enc_a<HASN>((ab >> (2 * k)) & 3u, HASN && ((an >> k) & 1u))
                            : enc_a<HASN>((ab2 >> (2 * (k - 16))) & 3u, HASN && ((an2 >> (k - 16)) & 1u));
        }
#pragma unroll
        for (int k = C - 1; k < C + 15; ++k) W[k] = 0;
    }

    {
        // everything block 0 reads: ring A entries k < 16 + LPT*(C-1), ring B entries k < 16
        typedef Ring<C, LPT, HASN> RG;
        const int64_t A0 = t.a_base + t.begin_a - w, BB = t.b_base + t.begin_b;
        for (int k = lane; k < ROWS + (C - 1) * LPT; k += LPT) {
            const int64_t ia = A0 + k;
            const u32 code = (t.a2[ia >> 4] >> ((ia & 15) * 2)) & 3u;
            const bool isn = HASN && ((t.an[ia >> 5] >> (ia & 31)) & 1u);
            RG::put_a(wlane >> 4, k, code, isn);
        }
        if (lane < ROWS) {
            const int64_t ib = BB + lane;
            const u32 brow = enc_b<HASN>((t.b2[ib >> 4] >> ((ib & 15) * 2)) & 3u, HASN && ((t.bn[ib >> 5] >> (ib & 31)) & 1u)) -
                             (UNTAGGED ? RING_TAG<HASN> : 0u);
            RG::put_b(wlane >> 4, lane, brow);
        }
    }
    store_state<C>(st, Lp, acc, W, Lin, Lout);
}
