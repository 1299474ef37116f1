// Part of gamdp_kernel.hip (included inside namespace gamdp::{anonymous}): TWO tasks per wavefront in packed f16.
//
// The direction-free cell is two vector instructions that each issue once per quad-cycle (v_dot4_u32_u8, v_max3_i32),
// and the vector ALU is the binding resource.  gfx950 has a packed three-way maximum, v_pk_maximum3_f16, and integers up
// to 2048 are exact in f16: so the fast blocks of a PAIR of tasks run in one register set -- task A in the low halves,
// task B in the high halves -- with
//       v_perm_b32          one byte look-up per task: 4.0 (mismatch) or 7.0 (match) as the high byte of an f16
//       v_pk_fma_f16        diag candidate  = previous row + 3 * that  (+12 / +21: the tilted scores, without the x4)
//                           (two-task kernel: the look-up is 12 or 21 itself, the candidate a v_add_u32 on bit patterns, see below)
//       v_pk_maximum3_f16   max(diag, up, left)
// per cell PAIR: 1.5 instructions per cell instead of 2 (measured 20.4 against 13.9 Tcell/s, tools/valu_rate5.hip).
// Values are kept relative to a per-lane, per-task base (an int32) that is re-centred every group of four blocks, so they stay
// far inside the exact range: a lane's 19 columns span at most 18*21, 64 row-times add at most 64*21.  Hand-offs between
// neighbouring lanes add the (small, exact) difference of the two bases.  What the reference treats specially has packed forms of
// its own: the top blocks (pair_top_range: cells with pos <= 0) and the blocks with the last rows and the pos == end_a
// anti-diagonal (pair_range<END>, whose side captures go through side_capture); only the ramp of a task and what two tasks do not
// have in common stays in the int32 tagged code of kernel_fill.inc, one task (or quad) after the other.  What the strips need is
// stored packed as well: the live row of every 4th block and the per-row boundary values of every 2nd / 4th lane as f16 pairs
// (half the bytes of the int32 kernels) plus the bases they are relative to; materialise() converts back to int32 and re-enacts
// exactly the same tagged sweep as for the int32 kernels, so results are bit-identical.
// The TWO-task kernel (LPT == 64) goes one step further in its plain and END ranges (pair_range): a half is not an f16 NUMBER but
// the integer bit PATTERN of one ("the pattern format", below), so that the diag candidate of both tasks is one 32-bit integer add
// (v_add_u32 issues faster than v_pk_fma_f16: tools/valu_rate7.hip) while v_pk_maximum3_f16 still takes the three-way maximum.  Its
// top blocks compute in f16 (the NaN marker needs it) and convert what they store, so that a slot holds one layout.  The eight-task
// kernel (LPT == 16) is f16-numeric throughout.
#ifndef GAMDP_PACKED_TOP
#define GAMDP_PACKED_TOP 1
#endif
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ h2 as_h2(u32 x) { return __builtin_bit_cast(h2, x); }
__device__ __forceinline__ u32 as_u(h2 x) { return __builtin_bit_cast(u32, x); }
constexpr u32 PK_NINF = 0xFC00FC00u;   // (-inf, -inf): "no source"
constexpr u32 PK_PINF = 0x7C007C00u;

__device__ __forceinline__ u32 pk(const _Float16 lo, const _Float16 hi) { const h2 v = {lo, hi}; return as_u(v); }
__device__ __forceinline__ _Float16 lo_of(const u32 v) { return as_h2(v).x; }
__device__ __forceinline__ _Float16 hi_of(const u32 v) { return as_h2(v).y; }

// G4 value (multiple of 4, or NEG) -> f16 relative to `base` (units of G = G4 / 4)
__device__ __forceinline__ _Float16 g4_to_h(const int g4, const int base)
{
    if (g4 <= NEG / 2) return lo_of(PK_NINF);
    return (_Float16)(float)((g4 >> 2) - base);
}
__device__ __forceinline__ int h_to_g4(const _Float16 h, const int base)
{
    const float f = (float)h;
    if (!(f > -60000.0f)) return NEG;          // -inf (or garbage of a dead cell)
    if (!(f < 60000.0f)) return 0;             // garbage of a dead cell
    return 4 * ((int)f + base);
}

// ---- the PATTERN format of the two-task kernel (LPT == 64) ---------------------------------------------------------------------
// The bit patterns of the non-negative finite f16 numbers, 0x0000 ... 0x7BFF, are ordered exactly like the unsigned integers they
// are, and v_pk_maximum3_f16 hands back one of its operands bit for bit while they are normal numbers (patterns >= 0x0400;
// tools/valu_rate7.hip checks both on the device).  So the plain and END ranges of the two-task kernel keep a half-word as the
// INTEGER pattern PAT_OFF + (G - base): the three-way maximum is unchanged, and the diag candidate "+12 / +21 on both tasks" is one
// 32-bit integer add of (sB << 16) | sA -- nothing is rounded, nothing depends on a binade.  A live value stays inside
// [PAT_MIN, PAT_MAX] (pair_range has the bound), so the add of the low half never carries into the high half.  "No source" stays
// 0xFC00 (-inf), which the maximum orders below every pattern; it never passes through an add: an add would make it a NaN.
// Everything else that touches a half -- the base differences of the hand-offs, the re-centring -- is packed 16-bit integer
// arithmetic (no carry between the tasks).  The stored layout (checkpoint rows, boundary words) holds the same patterns, read as
// SIGNED 16-bit: value = (int16)pattern - PAT_OFF + base, so that every pattern with the top bit set (0xFC00, and whatever a dead
// lane holds) decodes far below the live values around it.
typedef unsigned short us2 __attribute__((ext_vector_type(2)));
constexpr u32 PAT_OFF2 = PAT_OFF * 0x00010001u;   // (PAT_OFF, PAT_MIN, PAT_MAX, pat_encode, pat_decode: gamdp_dev.h)
__device__ __forceinline__ u32 pat_add(const u32 a, const u32 b) { return __builtin_bit_cast(u32, __builtin_bit_cast(us2, a) + __builtin_bit_cast(us2, b)); }
__device__ __forceinline__ u32 pat_sub(const u32 a, const u32 b) { return __builtin_bit_cast(u32, __builtin_bit_cast(us2, a) - __builtin_bit_cast(us2, b)); }
__device__ __forceinline__ u32 pk16(const int lo, const int hi) { return ((u32)lo & 0xFFFFu) | ((u32)hi << 16); }
__device__ __forceinline__ u32 pat_lo(const u32 v) { return v & 0xFFFFu; }
__device__ __forceinline__ u32 pat_hi(const u32 v) { return v >> 16; }
// G4 value (multiple of 4, or NEG) -> pattern relative to `base`, and back (a pattern with the top bit set: "no source", or what a
// dead cell holds)
__device__ __forceinline__ u32 g4_to_pat(const int g4, const int base)
{
    if (g4 <= NEG / 2) return 0xFC00u;
    return pat_encode((g4 >> 2) - base);
}
__device__ __forceinline__ int pat_to_g4(const u32 p, const int base)
{
    if (p & 0x8000u) return NEG;
    return 4 * (pat_decode(p) + base);
}
// a packed f16 pair of the top blocks -> the stored patterns.  Clamped to +-16 000 first (a live value is an integer inside
// +-2 048 and converts exactly; -inf and the garbage of dead cells become a pattern that decodes to -16 000 or +16 000)
__device__ __forceinline__ u32 h2_to_pat(const u32 v)
{
    const h2 lim = {(_Float16)16000.0f, (_Float16)16000.0f};
    const h2 c = __builtin_elementwise_min(__builtin_elementwise_max(as_h2(v), -lim), lim);
    return pat_add(pk16((int)(short)c.x, (int)(short)c.y), PAT_OFF2);
}

// layout of the packed row / boundary stores inside a slot (words)
// GRP (the eight-task kernel, round 5): bases per GROUP of 4 blocks.  The lanes re-centre at group starts only (a lane's 19
// columns span at most 18 x 21, 64 row-times add at most 64 x 21: 1 722 < 2 048), so everything a group stores is relative to the
// bases of its checkpoint row, and a lane's checkpoint row carries them -- its own and its right neighbour's, whose hand-offs a
// strip's right edge consumes -- behind its 19 values: 24 words per lane, 192 B per 2-lane strip, no per-block base words.  What a
// strip call fetches of a group is then its 192 B of checkpoint and one whole 128 B line of boundary values per block (it was: 160 B
// across two or three lines + two base words in lines of their own, and per block two 64 B half lines + a base word in a third).
template <int C, int LPT>
struct PairFmt {
    typedef Strip<LPT, true> ST;
    static constexpr bool GRP = (LPT == QL);
    static constexpr u32 CK_LANE = GRP ? 24u : (u32)LANE_WORDS<C>;      // words per lane of a checkpoint row
    static_assert(!GRP || C + 4 <= 24, "checkpoint row of the eight-task kernel");
    static constexpr u32 CK_ROWS = 64u * CK_LANE;                       // per group: the packed live rows (lane major) ...
    static constexpr u32 CK_WORDS = GRP ? CK_ROWS : CK_ROWS + 128;      // ... + [task][lane] bases (GRP: inside the rows)
    static constexpr u32 BND_VALS = ST::BND_WORDS;                      // per block: the packed boundary values (Strip::offset) ...
    static constexpr u32 BND_WORDS = GRP ? ST::BND_WORDS : ST::BND_WORDS + 2u * ST::NB;   // ... + [task][lane/SL] bases (GRP: none)
    static constexpr int RC = 4;                                        // blocks between re-centrings of the plain packed range (round 5: a group, for both kernels)
};
__shared__ u32 s_ringB2[RING_B + ROWS];   // task B's look-up bytes (task A's are in s_ringB)
// side-capture scratch of the packed blocks of the eight-task kernel: [task row][lane parity][column], both quads' halves
// (a capture drops the lane's packed row and picks one column back by index; PRing::cap_pick)
__shared__ u32 s_pcap[QT][2][20];

// the per-row operands of a pair: ring A entry = v_perm selector for both tasks, ring B entries = the look-up bytes
__device__ __forceinline__ u32 pk_sel(const u32 codeA, const u32 codeB) { return 0x000C000Cu | (codeA << 8) | ((4u + codeB) << 24); }
__device__ __forceinline__ u32 pk_tab(const u32 codeb) { return 0x44444444u + (0x03u << (codeb * 8u)); }  // high byte of 4.0 / 7.0
// the pattern format: the looked-up byte is the score itself, 12 or 21, in the LOW byte of each half, zero above it
__device__ __forceinline__ u32 pat_sel(const u32 codeA, const u32 codeB) { return 0x0C000C00u | codeA | ((4u + codeB) << 16); }
__device__ __forceinline__ u32 pat_tab(const u32 codeb) { return 0x0C0C0C0Cu + (0x09u << (codeb * 8u)); }

__device__ __forceinline__ u32 code2_at(gcptr p2, int64_t idx) { return (p2[idx >> 4] >> ((idx & 15) * 2)) & 3u; }

// The operand rings of the packed sweep.  LPT = 64 (two tasks per wavefront): the transposed dword ring A of the
// band-512 kernels holds the selectors, s_ringB / s_ringB2 the look-up bytes of task A / B.  LPT = 16 (two QUADS of tasks
// per wavefront, band 150): one set of rings per DPP row; ring A entries are 16 bit (code of A's base, 4 + code of B's
// base) and become the selector with one v_perm + one v_or per row and lane -- dword rings for four rows do not fit.
__shared__ u32 s_oB2[QT][64 + ROWS];   // (s_oA16: kernel_common.inc, shared with the int32 phases' byte ring)
// PAT: the entries are in the pattern format's forms (pair_range of the two-task kernel; the rings are primed per range)
template <int C, int LPT, bool PAT = false>
struct PRing {
    static_assert(!PAT || LPT == 64, "the pattern format is the two-task kernel's");
    static __device__ __forceinline__ u32 sel(const u32 codeA, const u32 codeB) { return PAT ? pat_sel(codeA, codeB) : pk_sel(codeA, codeB); }
    static __device__ __forceinline__ u32 tab(const u32 codeb) { return PAT ? pat_tab(codeb) : pk_tab(codeb); }
    typedef typename std::conditional<LPT == 64, const u32*, const uint16_t*>::type APtr;
    static constexpr int SZ = QRing<C>::SZ;
    static __device__ __forceinline__ void put_a(const int sub, const int k, const u32 codeA, const u32 codeB)
    {
        if constexpr (LPT == 64) RingA<C>::put(k, sel(codeA, codeB));
        else {
            const u32 pos = (u32)k % (u32)SZ;
            const uint16_t v = (uint16_t)(codeA | ((4u + codeB) << 8));
            s_oA16[sub][pos] = v;
            if (pos < ROWS) s_oA16[sub][pos + SZ] = v;
        }
    }
    static __device__ __forceinline__ void put_b(const int sub, const int k, const u32 ta, const u32 tb)
    {
        if constexpr (LPT == 64) {
            const int pb = k & (RING_B - 1);
            s_ringB[pb] = ta; s_ringB2[pb] = tb;
            if (pb < ROWS) { s_ringB[pb + RING_B] = ta; s_ringB2[pb + RING_B] = tb; }
        } else {
            const int pb = k & 63;
            s_qB[sub][pb] = ta; s_oB2[sub][pb] = tb;
            if (pb < ROWS) { s_qB[sub][pb + 64] = ta; s_oB2[sub][pb + 64] = tb; }
        }
    }
    static __device__ __forceinline__ APtr a_lane(const int tau0, const int lane)
    {
        if constexpr (LPT == 64) return s_ringA + (u32)((tau0 + (C - 1) * (lane + 1)) >> 4) % (u32)RingA<C>::COLS;
        else return s_oA16[lane >> 4] + (u32)(tau0 + (C - 1) * ((lane & (QL - 1)) + 1)) % (u32)SZ;
    }
    static __device__ __forceinline__ u32 a_read(APtr p, const int r)
    {
        if constexpr (LPT == 64) return p[r * RingA<C>::COLS];
        else return __builtin_amdgcn_perm(0x0C0C0C0Cu, (u32)p[r], 0x01040004u);  // bytes [hi, 0x0C, lo, 0x0C]: 0x0C = the "zero" selector
    }
    static __device__ __forceinline__ const u32* b_lane(const int tau0, const int lane, const int half)
    {
        if constexpr (LPT == 64) return (half ? s_ringB2 : s_ringB) + ((tau0 - lane) & (RING_B - 1));
        else return (half ? s_oB2[lane >> 4] : s_qB[lane >> 4]) + ((tau0 - (lane & (QL - 1))) & 63);
    }
    // side captures (the pos == end_a / pos == 0 cell of a row: at most two adjacent lanes per row-time and task): the lane's packed
    // row goes to a small LDS buffer per task and lane parity, the cell is picked up by index; returns that task's half of it.
    // Eight-task kernel: the row is dropped as it is (dwords, both halves: ten ds_write2 instead of nineteen 16-bit stores) into ONE
    // buffer per task row and parity that the two halves use one after the other -- LDS instructions of a wavefront execute in order,
    // so half A's read is done before a lane of the same parity drops its row for half B.
    template <int C2>
    static __device__ __forceinline__ _Float16 cap_pick(const int wlane, const int half, const u32 (&Lp)[C2], const int idx)
    {
        const int lane = wlane & (LPT - 1);
        if constexpr (LPT == 64) {
            u32* const cb = (u32*)s_cap[half][lane & 1];
#pragma unroll
            for (int c = 0; c < C2; ++c) cb[c] = Lp[c];
            const u32 v = cb[idx];
            return half ? hi_of(v) : lo_of(v);
        } else {
            u32* const cb = s_pcap[wlane >> 4][lane & 1];
#pragma unroll
            for (int c = 0; c < C2; ++c) cb[c] = Lp[c];
            return __builtin_bit_cast(_Float16, reinterpret_cast<const uint16_t*>(cb)[2 * idx + half]);
        }
    }
    // the same for a row of patterns (two-task kernel, pair_range): the 16 bits as they are
    template <int C2>
    static __device__ __forceinline__ u32 cap_pick_pat(const int wlane, const int half, const u32 (&Lp)[C2], const int idx)
    {
        static_assert(LPT == 64, "the pattern format is the two-task kernel's");
        u32* const cb = (u32*)s_cap[half][wlane & 1];
#pragma unroll
        for (int c = 0; c < C2; ++c) cb[c] = Lp[c];
        const u32 v = cb[idx];
        return half ? pat_hi(v) : pat_lo(v);
    }
    // the producers expand the 16 new entries of the block whose first row-time is T (lanes 0..15, or every lane for its row)
    // MARK (the top blocks): the entry of a task's base -1 -- ring index km1A / km1B -- is not a look-up but the NaN marker
    // (code 13 / 9: the selector byte 0x0D, which v_perm turns into 0xFF; pair_top_range)
    static constexpr u32 MARK_A = 13u, MARK_B = 9u;
    template <bool MARK = false>
    static __device__ __forceinline__ void produce(const int T, const int lane, const u32 awA, const u32 awB, const u32 bwA, const u32 bwB, const int km1A = 0, const int km1B = 0)
    {
        const int r = lane & (QL - 1);
        if (LPT == QL || lane < ROWS) {
            const int k = T + (C - 1) * LPT + r;
            u32 cA = (awA >> (2 * r)) & 3u, cB = (awB >> (2 * r)) & 3u;
            if constexpr (MARK) { cA = (k == km1A) ? MARK_A : cA; cB = (k == km1B) ? MARK_B : cB; }
            put_a(lane >> 4, k, cA, cB);
            put_b(lane >> 4, T + r, tab((bwA >> (2 * r)) & 3u), tab((bwB >> (2 * r)) & 3u));
        }
    }
    // everything block `blk` of the packed sweep reads from the rings
    template <bool MARK = false>
    static __device__ __forceinline__ void prime(const Tk& ta, const Tk& tb, const int blk, const int lane, const int km1A = 0, const int km1B = 0)
    {
        const int T0 = blk * ROWS, tl = lane & (LPT - 1), sub = lane >> 4;
        const int64_t A0a = ta.a_base + ta.begin_a - ta.band, A0b = tb.a_base + tb.begin_a - tb.band;
        for (int k = T0 + tl; k < T0 + ROWS + (C - 1) * LPT; k += LPT) {
            u32 cA = code2_at(ta.a2, A0a + k), cB = code2_at(tb.a2, A0b + k);
            if constexpr (MARK) { cA = (k == km1A) ? MARK_A : cA; cB = (k == km1B) ? MARK_B : cB; }
            put_a(sub, k, cA, cB);
        }
        const int64_t Ba = ta.b_base + ta.begin_b, Bb = tb.b_base + tb.begin_b;
        for (int k = T0 - (LPT - 1) + tl; k <= T0 + ROWS - 1; k += LPT) put_b(sub, k, tab(code2_at(ta.b2, Ba + k)), tab(code2_at(tb.b2, Bb + k)));
    }
};

// the same for the int32 code of ONE task that continues at block `blk` (its rings were overwritten meanwhile), plus
// the a-window of the lane
template <int C, bool HASN, bool UNTAGGED, int LPT>
__device__ __forceinline__ void single_prime(const Tk& t, const int blk, const int wlane, u32 (&W)[C + 15])
{
    typedef Ring<C, LPT, HASN> RG;
    const int T0 = blk * ROWS, lane = wlane & (LPT - 1), sub = wlane >> 4;
    const int64_t A0 = t.a_base + t.begin_a - t.band, BB = t.b_base + t.begin_b;
    for (int k = T0 + lane; k < T0 + ROWS + (C - 1) * LPT; k += LPT) RG::put_a(sub, k, code2_at(t.a2, A0 + k), false);
    for (int k = T0 - (LPT - 1) + lane; k <= T0 + ROWS - 1; k += LPT)
        RG::put_b(sub, k, enc_b<HASN>(code2_at(t.b2, BB + k), false) - (UNTAGGED ? RING_TAG<HASN> : 0u));
    const int64_t s0 = A0 + (int64_t)(C - 1) * lane + T0;
    const u32 ab = fetch16(t.a2, s0), ab2 = (C - 1 > 16) ? fetch16(t.a2, s0 + 16) : 0u;
#pragma unroll
    for (int k = 0; k < C - 1; ++k) W[k] = (k < 16) ? enc_a<HASN>((ab >> (2 * k)) & 3u, false) : enc_a<HASN>((ab2 >> (2 * (k - 16))) & 3u, false);
#pragma unroll
    for (int k = C - 1; k < C + 15; ++k) W[k] = 0;
}

// the packed live rows of a group start and the bases they are relative to
template <int C, int LPT>
__device__ __forceinline__ void ck_store(gptr ck, const int wlane, const u32 (&Lp)[C], const int baseA, const int baseB)
{
    typedef PairFmt<C, LPT> FMT;
    if constexpr (FMT::GRP) {
        // the right neighbour's bases (the task's last lane keeps its own: nobody consumes its right stream)
        const u32 rA = (u32)lane_shl1<LPT>(baseA, baseA), rB = (u32)lane_shl1<LPT>(baseB, baseB);
        gptr row = ck + (u32)wlane * FMT::CK_LANE;
#pragma unroll
        for (int g = 0; g < 6; ++g) {
            auto w = [&](const int i) -> u32 { return i < C ? Lp[i < C ? i : 0] : (i == C ? (u32)baseA : (i == C + 1 ? (u32)baseB : (i == C + 2 ? rA : (i == C + 3 ? rB : 0u)))); };
            const u32x4 q = {w(4 * g), w(4 * g + 1), w(4 * g + 2), w(4 * g + 3)};
            *(g4ptr)(row + 4 * g) = q;
        }
    } else {
        img_store<C, true>(ck, wlane, Lp);
        ck[FMT::CK_ROWS + wlane] = (u32)baseA;
        ck[FMT::CK_ROWS + 64 + wlane] = (u32)baseB;
    }
}

// ---- side captures of the packed blocks --------------------------------------------------------------------------------
// The cells the end-cell search and the walk read off the fill: the pos == end_a cell of every row (END blocks -> adh), the
// pos == 0 cell of every row (top blocks -> pos0), and a task's last row (END blocks -> lastrow), converted back to H.
// What a capture needs of a task -- four numbers -- lives in LDS, one entry per task of the wavefront, and is read afresh in
// every row (round 5: held in registers -- end_a, X, Y, iA and two pointers per half -- they pushed these instances into
// private memory, and every reload of a spilled value waits behind the boundary stores of the block before: vmcnt counts
// loads and stores in one queue; an END block took eight times a plain one).  With T = tau0 + r, the row-time, and word
// offsets from the slot's first word, an entry {E0, R0, P0, L0} says:
//   the lane's column on the anti-diagonal    cE = E0 - (C-1) lane - T,  inside the band for cE < cap_max
//                                              (E0 = end_a - begin_a + band for pos == end_a, band - begin_a for pos == 0)
//   its row T - lane is a row of the task      T <= R0 + lane  (R0 = X - 1);  the last one: T == R0 + lane
//   the cell's slot in adh / pos0               slot[P0 - lane + T];  H = value + base - 16 row - 8 (C lane + cE) = value + base + 8 (lane - E0 - T)
//   lastrow[j] = slot[L0 + j]
// (row >= 1 needs no test: the packed ranges begin behind the ramp and a tagged block, tau0 >= 64 > lane + 1.)
// (s_captab[task row (one with two tasks per wavefront)][half]: kernel_common.inc)
template <int C, int LPT>
__device__ __forceinline__ int cap_limit(const Tk& t, const int lane) { return max(0, min(C, t.Y - C * lane)); }   // (one band per launch of a packed kernel: CE is a constant)
template <int LPT>
__device__ __forceinline__ void cap_table(const int wlane, const int half, const int E0, const int R0, const int P0, const int L0)
{
    if ((wlane & (LPT - 1)) == 0) {
        const int4 e = {E0, R0, P0, L0};
        *reinterpret_cast<int4*>(s_captab[LPT == 64 ? 0 : wlane >> 4][half]) = e;
    }
}
// PAT: the row holds patterns (pair_range of the two-task kernel): value = pattern - PAT_OFF + base
template <int C, int CE, int LPT, bool LAST, bool PAT = false>
__device__ __forceinline__ void side_capture(const int wlane, const int half, const int T, const int base, const u32 (&Lp)[C], const int cap_max, giptr const cap_slot)
{
    const int lane = wlane & (LPT - 1);
    const int4 e = *reinterpret_cast<const int4*>(s_captab[LPT == 64 ? 0 : wlane >> 4][half]);
    const int cE = e.x - (C - 1) * lane - T;
    if ((u32)cE < (u32)cap_max && T <= e.y + lane) {
        if constexpr (PAT) {
            const u32 vE = PRing<C, LPT>::cap_pick_pat(wlane, half, Lp, cE);
            cap_slot[e.z - lane + T] = pat_decode(vE) + base + 8 * (lane - e.x - T);
        } else {
            const _Float16 vE = PRing<C, LPT>::cap_pick(wlane, half, Lp, cE);
            cap_slot[e.z - lane + T] = (int)(float)vE + base + 8 * (lane - e.x - T);
        }
    }
    if constexpr (LAST) {
        if (T == e.y + lane && cap_max > 0) {   // the lane's last row (cap_max: C, CE + 1 in the band's last lane, 0 behind it)
            giptr const lp = cap_slot + (e.w + C * lane);
            const int k1 = base - 16 * e.y - 8 * C * lane;
            auto put = [&](const int c) __attribute__((always_inline)) {
                if constexpr (PAT) lp[c] = pat_decode(half ? pat_hi(Lp[c]) : pat_lo(Lp[c])) + (k1 - 8 * c);
                else lp[c] = (int)(float)(half ? hi_of(Lp[c]) : lo_of(Lp[c])) + (k1 - 8 * c);
            };
#pragma unroll
            for (int c = 0; c <= CE; ++c) put(c);
            if (cap_max == C) {
#pragma unroll
                for (int c = CE + 1; c < C; ++c) put(c);
            }
        }
    }
}

// ---- blocks [blk_begin, blk_end) of both tasks, packed -------------------------------------------------------
// In: the int32 states of the two tasks at the start of block blk_begin (both in fast blocks from here to blk_end).
// Out: their int32 states at the start of block blk_end; the rings then hold nothing the int32 code can use.
// END: the range may hold blocks with the last rows / the pos==end_a anti-diagonal of either task.  As in the int32
// direction-free end blocks nothing is masked -- rows past X-1 compute on padding and only ever feed rows past X-1 --
// but the values the end-cell search scans are taken as they pass, converted back to H: the last row of a lane, and
// the anti-diagonal cell (at most two adjacent lanes per row-time and task: the lane's packed row goes through a small
// LDS buffer per task and lane parity and is picked up by index).
// LPT = 16: the two "tasks" are two QUADS of tasks (band 150, one task per DPP row of 16 lanes x 19 columns each): *tpa / *tpb
// then hold, in every lane, the values of the lane's own task of quad A / quad B.
template <int C, int CE, bool END, int LPT = 64>
__device__ __noinline__ void pair_range(BlockState<C>* sta, BlockState<C>* stb, const Tk* tpa, const Tk* tpb, const int blk_begin_, const int blk_end_, const int wlane)
{
    static_assert(CE >= 0 && CE < C - 1 && (LPT == QL || (C - 1) % 16 == 0), "band 512 on 64 lanes (transposed ring A) or band 150 on 16");
    // PAT: the two-task kernel keeps its halves as integer patterns (the pattern format, above); the eight-task kernel as f16 numbers
    constexpr bool PAT = (LPT == 64);
    typedef PRing<C, LPT, PAT> PR;
    const Tk ta = load_tk<LPT>(tpa), tb = load_tk<LPT>(tpb);
    const int blk_begin = uni(blk_begin_), blk_end = uni(blk_end_);
    const int lane = wlane & (LPT - 1);  // lane within the task: owns band columns [C*lane, C*lane + C)
    const int LE = (ta.Y - 1) / C;
    u32 Lp[C], W[C + 15];
    int baseA, baseB;
    u32 Lin, dL, dR;
    {
        // bases: the lane's own column 0; dead lanes (NEG everywhere) get 0
        baseA = (sta->Lp[0] <= NEG / 2) ? 0 : (sta->Lp[0] >> 2);
        baseB = (stb->Lp[0] <= NEG / 2) ? 0 : (stb->Lp[0] >> 2);
        // what has to be added to a value that arrives from the left / right neighbour: its base minus mine
        const int lA = __shfl_up(baseA, 1, LPT), lB = __shfl_up(baseB, 1, LPT), rA = __shfl_down(baseA, 1, LPT), rB = __shfl_down(baseB, 1, LPT);
        const bool hasL = lane >= 1 && lane <= LE, hasR = lane < LE;
        if constexpr (PAT) {
            // NEG -> 0xFC00: lane 0's Lin (it stays that: the DPP shift leaves lane 0 alone, its dL is 0 and the re-centring skips
            // it) and the cells of the dead lanes and columns, which an add turns into garbage that only dead cells ever see (below)
#pragma unroll
            for (int c = 0; c < C; ++c) Lp[c] = g4_to_pat(sta->Lp[c], baseA) | (g4_to_pat(stb->Lp[c], baseB) << 16);
            Lin = g4_to_pat(sta->Lin, baseA) | (g4_to_pat(stb->Lin, baseB) << 16);
            // signed differences as 16-bit two's complement: added per half (pat_add), never with a 32-bit add
            dL = hasL ? pk16(lA - baseA, lB - baseB) : 0u;
            dR = hasR ? pk16(rA - baseA, rB - baseB) : 0u;
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) Lp[c] = pk(g4_to_h(sta->Lp[c], baseA), g4_to_h(stb->Lp[c], baseB));
            Lin = pk(g4_to_h(sta->Lin, baseA), g4_to_h(stb->Lin, baseB));
            dL = hasL ? pk((_Float16)(float)(lA - baseA), (_Float16)(float)(lB - baseB)) : 0u;
            dR = hasR ? pk((_Float16)(float)(rA - baseA), (_Float16)(float)(rB - baseB)) : 0u;
        }
        // selector window of row-time blk_begin*16: W[k] <-> a index begin_a - band + (C-1)*lane + T0 + k
        const int T0 = blk_begin * ROWS;
        const int64_t sa = ta.a_base + ta.begin_a - ta.band + (int64_t)(C - 1) * lane + T0, sb = tb.a_base + tb.begin_a - tb.band + (int64_t)(C - 1) * lane + T0;
        const u32 wa = fetch16(ta.a2, sa), wb = fetch16(tb.a2, sb);
        const u32 wa2 = (C - 1 > 16) ? fetch16(ta.a2, sa + 16) : 0u, wb2 = (C - 1 > 16) ? fetch16(tb.a2, sb + 16) : 0u;
#pragma unroll
        for (int k = 0; k < C - 1; ++k)
            W[k] = (k < 16) ? PR::sel((wa >> (2 * k)) & 3u, (wb >> (2 * k)) & 3u) : PR::sel((wa2 >> (2 * (k - 16))) & 3u, (wb2 >> (2 * (k - 16))) & 3u);
#pragma unroll
        for (int k = C - 1; k < C + 15; ++k) W[k] = 0;
    }
    PR::prime(ta, tb, blk_begin, wlane);

    const int64_t iAa = ta.a_base + ta.begin_a - ta.band + (C - 1) * LPT, iBa = ta.b_base + ta.begin_b;
    const int64_t iAb = tb.a_base + tb.begin_a - tb.band + (C - 1) * LPT, iBb = tb.b_base + tb.begin_b;
    gcptr paA = ta.a2 + (iAa >> 4), pbA = ta.b2 + (iBa >> 4), paB = tb.a2 + (iAb >> 4), pbB = tb.b2 + (iBb >> 4);
    const u32 shaA = (u32)(iAa & 15) * 2u, shbA = (u32)(iBa & 15) * 2u, shaB = (u32)(iAb & 15) * 2u, shbB = (u32)(iBb & 15) * 2u;
    u32 aA_lo = paA[blk_begin + 1], aA_hi = paA[blk_begin + 2], bA_lo = pbA[blk_begin + 1], bA_hi = pbA[blk_begin + 2];
    u32 aB_lo = paB[blk_begin + 1], aB_hi = paB[blk_begin + 2], bB_lo = pbB[blk_begin + 1], bB_hi = pbB[blk_begin + 2];
    // The eight words above must have ARRIVED before the loop is entered.  Left pending, the compiler has to wait for them at
    // the top of the loop body -- and vmcnt counts loads and stores in one queue, in order: in every later iteration that same
    // s_waitcnt then sits behind the boundary stores the previous block issued a moment ago and drains them (SQ_WAIT_ANY 21 %
    // of a lone wavefront's time, ~1 500 cycles per block; hidden behind the other wavefronts only when a SIMD has four).
    asm volatile("" : "+v"(aA_lo), "+v"(aA_hi), "+v"(bA_lo), "+v"(bA_hi), "+v"(aB_lo), "+v"(aB_hi), "+v"(bB_lo), "+v"(bB_hi));
    [[maybe_unused]] const h2 three = {(_Float16)3.0f, (_Float16)3.0f};
    const bool no_up = lane == LE;  // the last band column (column CE of this lane) has no `up` source
    typedef Strip<LPT, true> ST;
    typedef PairFmt<C, LPT> FMT;
    // PAT, the range argument: the lanes re-centre on column 0 at group ends, a column grows by at most 21 per row and a lane's C
    // columns span at most (C - 1) x 21, so between two re-centrings a live value of a lane -- its columns, the chain value from the
    // left (which may lie below column 0), the hand-off from the right (above column C - 1), each a neighbour of one of the lane's
    // own cells -- stays within SPAN + 21 of the lane's base on either side: 1 701 for 17 columns, where 7 168 are free below
    // PAT_OFF and 23 509 above it.
    constexpr int SPAN = (C - 1) * 21 + FMT::RC * ROWS * 21;
    static_assert(!PAT || ((int)PAT_OFF - (SPAN + 21) >= (int)PAT_MIN && (int)PAT_OFF + SPAN + 21 <= (int)PAT_MAX), "the live patterns of a group stay normal, finite f16 numbers");
    constexpr int NB = ST::NB, FI = ST::FI;
    const int sshift = uni(ta.sshift);
    const bool edge = ST::opens_strip(wlane, sshift);
    const u32 my_slot = ST::slot_of(wlane, sshift);
    const u64 edge_mask = __ballot(edge);
    u32* const s_bnd = ST::staging();
    u32* const sb = s_bnd + my_slot;
    gptr const ckpt = ta.ckpt, bnd = ta.bnd;  // shared by the pair
    int xkeep = (int)PK_NINF;
    const int prio_R = uni(ta.prio_R), prio_nblk = uni(ta.prio_nblk);
    // END: the side captures (side_capture above)
    const int cap_max = END ? cap_limit<C, LPT>(ta, lane) : 0;
    giptr const cap_slot = (giptr)unip(ta.dir);   // (quad / task A's direction image is the slot's first word)
    if constexpr (END) {
        cap_table<LPT>(wlane, 0, ta.eaRel, ta.X - 1, (int)(ta.adh - cap_slot) - ta.iA, (int)(ta.lastrow - cap_slot));
        cap_table<LPT>(wlane, 1, tb.eaRel, tb.X - 1, (int)(tb.adh - cap_slot) - tb.iA, (int)(tb.lastrow - cap_slot));
    }
    // The selector window slides by 16 entries per block.  With 17 columns per lane it holds exactly 32: two copies of the block
    // body, the second with every window index turned by 16, spare the 16 register moves per block that slide it (ROT).
    constexpr bool ROT = (C + 15 == 32);
    auto block_body = [&](auto phase, const int blk) __attribute__((always_inline)) {
        constexpr int WO = ROT ? 16 * decltype(phase)::value : 0;
#define WX(i) (ROT ? (((i) + WO) & 31) : (i))
        const int T = (blk + 1) * ROWS, tau0 = blk * ROWS;
        if (prio_R != 0 && (blk & 7) == 0) set_prio_by_remaining(prio_nblk - blk, prio_R);
        const u32 aA_nx = paA[blk + 3], bA_nx = pbA[blk + 3], aB_nx = paB[blk + 3], bB_nx = pbB[blk + 3];
        PR::produce(T, wlane, __builtin_amdgcn_alignbit(aA_hi, aA_lo, shaA), __builtin_amdgcn_alignbit(aB_hi, aB_lo, shaB),
                    __builtin_amdgcn_alignbit(bA_hi, bA_lo, shbA), __builtin_amdgcn_alignbit(bB_hi, bB_lo, shbB));
        if ((blk & 3) == 0) ck_store<C, LPT>(ckpt + (u64)(blk >> 2) * FMT::CK_WORDS, wlane, Lp, baseA, baseB);  // the live rows of this group start, packed, and the bases they are relative to
        if constexpr (!FMT::GRP) {
            if (edge) {  // bases of the boundary lanes for this block
                gptr bb = bnd + (u64)blk * FMT::BND_WORDS + FMT::BND_VALS;
                bb[my_slot] = (u32)baseA;
                bb[NB + my_slot] = (u32)baseB;
            }
        }
        const typename PR::APtr ringA_lane = PR::a_lane(tau0, wlane);
        const u32* const rbA = PR::b_lane(tau0, wlane, 0);
        const u32* const rbB = PR::b_lane(tau0, wlane, 1);
        // The 16 x C cells of the block as ONE software-pipelined stream.  Written cell by cell (perm -> fma -> max3) every
        // instruction depends on the one before it and the compiler leaves it that way (padding the hazards with s_nop): a
        // wavefront then issues one instruction per ~7.7 cycles whatever else the SIMD could do, which is what a SIMD with
        // one or two resident wavefronts -- the last round of a short launch -- delivers (tools/valu_rate6.hip: 12.6 against
        // 17.8 Tcell/s at one wavefront per SIMD).  Here cell g = r * C + c is spread over three scheduling groups: its
        // look-up (v_perm) two groups ahead, its diag candidate (v_pk_fma) one group ahead, its v_pk_maximum3 in its own
        // group, so that nothing waits for its predecessor; sched_barrier keeps the compiler from undoing it.  The hand-off
        // of column 0 (DPP needs two wait states after the write) trails its cell by two groups, and the first cell of a
        // row runs its group's look-ahead work BEFORE its max3, behind the DPP + base correction of the left chain value.
        {
            u32 tA[2], tB[2];     // look-up bytes of row r in [r & 1], requested at the end of row r - 2
            u32 m[3], D[2];       // look-ups / diag candidates in flight: cell g in m[g % 3], D[g % 2]
            u32 L = Lin, x = PK_NINF, Lrecv = Lin;
            W[WX(C - 1)] = PR::a_read(ringA_lane, 0);
            tA[0] = rbA[0]; tB[0] = rbB[0];
            W[WX(C)] = PR::a_read(ringA_lane, 1);
            tA[1] = rbA[1]; tB[1] = rbB[1];
            auto do_perm = [&](const int g) __attribute__((always_inline)) {
                const int r = g / C, c = g % C;
                m[g % 3] = __builtin_amdgcn_perm(tB[r & 1], tA[r & 1], W[WX(r + c)]);
            };
            // PAT: the looked-up word is (sB << 16) | sA with s = 12 or 21, the diag candidate one 32-bit add (v_add_u32) -- the low
            // half of a live cell cannot carry (PAT_MAX).  A dead cell's can: into the other task's half of the SAME register, which
            // is the same column of the same lane and dead as well, because the two tasks of a unit share Y (LE, CE).  Dead are the
            // lanes behind LE and the columns behind CE in lane LE; what they hold reaches no live cell: the one `up` source that
            // could is cut off in do_max (no_up), the chain value runs left to right, away from the band, and lane LE + 1 hands its
            // column 0 to column C - 1 of lane LE, a dead one.  Rows past a task's X - 1 (END) are ordinary cells on padding.
            auto do_fma = [&](const int g) __attribute__((always_inline)) {
                if constexpr (PAT) D[g % 2] = m[g % 3] + Lp[g % C];
                else D[g % 2] = as_u(__builtin_elementwise_fma(as_h2(m[g % 3]), three, as_h2(Lp[g % C])));
            };
            auto do_max = [&](const int g) __attribute__((always_inline)) {
                const int c = g % C;
                h2 U = as_h2((c < C - 1) ? Lp[(c < C - 1) ? c + 1 : c] : x);
                if (c == CE) U = as_h2(no_up ? PK_NINF : as_u(U));
                L = as_u(__builtin_elementwise_maximum(__builtin_elementwise_maximum(as_h2(D[g % 2]), U), as_h2(L)));
                Lp[c] = L;
            };
            do_perm(0); do_perm(1); do_fma(0);
            __builtin_amdgcn_sched_barrier(0);
            static_for<ROWS>([&](auto rc) __attribute__((always_inline)) {
                constexpr int r = decltype(rc)::value;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const int g = r * C + c;
                    if (c == 0) {
                        L = Lin; Lrecv = Lin;
                        do_fma(g + 1);
                        do_max(g);
                        do_perm(g + 2);   // (between this maximum and the next cell's, which depends on it: back to back they cost a hazard nop)
                    } else {
                        do_max(g);
                        if (g + 1 < ROWS * C) do_fma(g + 1);
                        if (g + 2 < ROWS * C) do_perm(g + 2);
                    }
                    if (c == 2) xkeep = lane_shl1<LPT>(xkeep, (int)Lp[0]);   // lane l <- lane l+1 of the same task
                    if (c == 3) {
                        // (PAT: lanes >= LE have dR = 0 and take their neighbour's word as it is -- 0xFC00 in lane 63, a dead lane's
                        // column 0 otherwise --: it feeds column C - 1 of a lane whose columns behind CE are dead)
                        x = PAT ? pat_add((u32)xkeep, dR) : as_u(as_h2((u32)xkeep) + as_h2(dR));
                        lds_store2_masked<4 * (r % FI) * NB, 4 * (NB * FI + (r % FI) * NB)>(sb, Lrecv, Lp[0], edge_mask);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                // operands of the row after next (this row's look-up bytes are done with: the look-ups run two cells ahead), in
                // flight for a whole row before their first use -- and here they fill the two wait states the DPP below needs
                // after the row's last maximum (a hazard nop per row-time otherwise)
                if constexpr (r + 2 < ROWS) { W[WX(C + 1 + r)] = PR::a_read(ringA_lane, r + 2); tA[r & 1] = rbA[r + 2]; tB[r & 1] = rbB[r + 2]; }
                Lin = (u32)lane_shr1<LPT>((int)Lin, (int)L);  // lane l <- lane l-1 ; lane 0 of a task keeps -inf
                // (lane 0's own previous Lin is -inf relative to any base: adding dL = 0 leaves it -- as a pattern, 0xFC00 + 0)
                Lin = PAT ? pat_add(Lin, dL) : as_u(as_h2(Lin) + as_h2(dL));
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (END) {
                    side_capture<C, CE, LPT, true, PAT>(wlane, 0, tau0 + r, baseA, Lp, cap_max, cap_slot);
                    side_capture<C, CE, LPT, true, PAT>(wlane, 1, tau0 + r, baseB, Lp, cap_max, cap_slot);
                }
                if ((r % FI) == FI - 1) {
                    // the staging area is full: its [slot][received | handed][FI row-times] image (Strip::offset) leaves as one
                    // coalesced store of whole lines, PER words per lane (2 KB with 4-lane strips, 4 KB with 2-lane strips)
                    constexpr u32 PER = 2u * NB * FI / 64u;
                    const u32 w0 = (u32)wlane * PER;
                    const u32* src = s_bnd + ST::staging_index(w0);
                    gptr bp = bnd + (u64)blk * FMT::BND_WORDS + (u32)(r / FI) * (u32)(2 * NB * FI) + w0;
#pragma unroll
                    for (u32 k = 0; k < PER; k += 4) {
                        const u32x4 v = {src[k * NB], src[(k + 1) * NB], src[(k + 2) * NB], src[(k + 3) * NB]};
                        *(g4ptr)(bp + k) = v;
                    }
                }
            });
        }
#ifdef GAMDP_DIAG
        {   // Diagnostics build only: the assertion behind the range argument.  Integers are exact in f16 up to 2048; the
            // values of a lane grow monotonically down a block (every row adds at least a mismatch's +12 to a column) and
            // along a row, so their extremes are what the block ends with: every value of this lane that lies inside the
            // band -- its columns, the chain value it received, the hand-off it took from its right neighbour -- must lie
            // inside +-2040 BEFORE the re-centring brings them back.  (Inside the band every cell of the packed range is
            // live, hence finite; the columns behind the last band column in lane LE and the lanes behind it compute on
            // garbage that never reaches a live cell -- the one `up` source that could is cut off above -- and do not
            // count.)  Kept cheap -- a packed maximum of magnitudes, ~45 instructions per block -- so that the diagnostics
            // build stays usable for timing.  A violation marks the task(s): finish_walk reports GAMDP_ST_DIAG_RANGE.
            // PAT: the same cells, integer compares on the patterns, both bounds: [PAT_MIN, PAT_MAX]
            if constexpr (PAT) {
                auto mn = [](const u32 a, const u32 b) { return __builtin_bit_cast(u32, __builtin_elementwise_min(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b))); };
                auto mx = [](const u32 a, const u32 b) { return __builtin_bit_cast(u32, __builtin_elementwise_max(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b))); };
                u32 nIn = 0xFFFFFFFFu, xIn = 0, nOut = 0xFFFFFFFFu, xOut = 0;   // packed min / max over the columns inside the band in every lane / only in lanes < LE
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    if (c <= CE) { nIn = mn(nIn, Lp[c]); xIn = mx(xIn, Lp[c]); }
                    else { nOut = mn(nOut, Lp[c]); xOut = mx(xOut, Lp[c]); }
                }
                if (lane >= 1) { nIn = mn(nIn, Lin); xIn = mx(xIn, Lin); }
                const u32 xv = pat_add((u32)xkeep, dR);
                if (blk > blk_begin) { nOut = mn(nOut, xv); xOut = mx(xOut, xv); }
                if (lane < LE) { nIn = mn(nIn, nOut); xIn = mx(xIn, xOut); }
                if (lane <= LE) {
                    if (pat_lo(nIn) < PAT_MIN || pat_lo(xIn) > PAT_MAX) ta.pos0[-1] = 1;
                    if (pat_hi(nIn) < PAT_MIN || pat_hi(xIn) > PAT_MAX) tb.pos0[-1] = 1;
                }
            } else {
            u32 mIn = 0, mOut = 0;   // packed max |value| over the columns that are inside the band in every lane / only in lanes < LE
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const u32 a = Lp[c] & 0x7FFF7FFFu;
                if (c <= CE) mIn = as_u(__builtin_elementwise_max(as_h2(mIn), as_h2(a)));
                else mOut = as_u(__builtin_elementwise_max(as_h2(mOut), as_h2(a)));
            }
            if (lane >= 1) mIn = as_u(__builtin_elementwise_max(as_h2(mIn), as_h2(Lin & 0x7FFF7FFFu)));
            const u32 xv = as_u(as_h2((u32)xkeep) + as_h2(dR)) & 0x7FFF7FFFu;
            if (blk > blk_begin) mOut = as_u(__builtin_elementwise_max(as_h2(mOut), as_h2(xv)));
            if (lane < LE) mIn = as_u(__builtin_elementwise_max(as_h2(mIn), as_h2(mOut)));
            if (lane <= LE) {
                if (!((float)lo_of(mIn) < 2040.0f)) ta.pos0[-1] = 1;
                if (!((float)hi_of(mIn) < 2040.0f)) tb.pos0[-1] = 1;
            }
            }
        }
#endif
        // Re-centre on column 0 (both tasks at once) at GROUP ends only (FMT::RC = 4 blocks): a column grows by at most 21 per row
        // (a match's 5 + the tilt's 16) and a lane's C columns span at most (C - 1) x 21, so 64 row-times stay below 378 + 1 344 =
        // 1 722 < 2 048 (the diagnostics build asserts 2 040 above).  In the eight-task kernel everything a group stores is then
        // relative to ONE pair of bases per lane, the ones in its checkpoint row (PairFmt::GRP); its packed ranges begin and end at
        // group boundaries (run_octo), so "the last block of the range" is a group end too.  The two-task kernel keeps its per-block
        // base words (they simply repeat within a group).
        // PAT: integer arithmetic per half.  What the f16 form got from -inf / NaN being absorbing is said outright: a lane behind LE
        // holds garbage and shifts nothing (its base stays what it was), a live lane's column 0 is a live cell, lane 0's Lin stays
        // 0xFC00, and only the lanes that take a hand-off adjust its base difference.
        if constexpr (PAT) {
            if ((blk & (FMT::RC - 1)) == FMT::RC - 1 || blk + 1 == blk_end) {
                const u32 d = (lane <= LE) ? pat_sub(Lp[0], PAT_OFF2) : 0u;
                baseA += (int)(short)pat_lo(d);
                baseB += (int)d >> 16;
#pragma unroll
                for (int c = 0; c < C; ++c) Lp[c] = pat_sub(Lp[c], d);
                if (lane != 0) Lin = pat_sub(Lin, d);
                const u32 dl = (u32)lane_shr1<LPT>((int)d, (int)d);  // left neighbour's shift (a task's lane 0: its own)
                const u32 dr = (u32)lane_shl1<LPT>((int)d, (int)d);  // right neighbour's (its last lane: its own)
                if (lane >= 1 && lane <= LE) dL = pat_sub(pat_add(dL, dl), d);
                if (lane < LE) dR = pat_sub(pat_add(dR, dr), d);
            }
        } else
        if ((blk & (FMT::RC - 1)) == FMT::RC - 1 || blk + 1 == blk_end) {
            const float fa = (float)lo_of(Lp[0]), fb = (float)hi_of(Lp[0]);
            const bool oka = fa > -60000.0f && fa < 60000.0f, okb = fb > -60000.0f && fb < 60000.0f;
            const u32 d = pk(oka ? lo_of(Lp[0]) : (_Float16)0.0f, okb ? hi_of(Lp[0]) : (_Float16)0.0f);
            baseA += oka ? (int)fa : 0;
            baseB += okb ? (int)fb : 0;
#pragma unroll
            for (int c = 0; c < C; ++c) Lp[c] = as_u(as_h2(Lp[c]) - as_h2(d));
            Lin = as_u(as_h2(Lin) - as_h2(d));
            const u32 dl = (u32)lane_shr1<LPT>((int)d, (int)d);  // left neighbour's shift (a task's lane 0: its own)
            const u32 dr = (u32)lane_shl1<LPT>((int)d, (int)d);  // right neighbour's (its last lane: its own)
            if (lane >= 1 && lane <= LE) dL = as_u(as_h2(dL) + as_h2(dl) - as_h2(d));
            if (lane < LE) dR = as_u(as_h2(dR) + as_h2(dr) - as_h2(d));
            // xkeep holds the neighbour's column 0 relative to ITS base: no change needed, dR carries the difference
        }
        if constexpr (!ROT) {
#pragma unroll
            for (int k = 0; k < C - 1; ++k) W[k] = W[k + ROWS];
        }
        aA_lo = aA_hi; aA_hi = aA_nx; bA_lo = bA_hi; bA_hi = bA_nx;
        aB_lo = aB_hi; aB_hi = aB_nx; bB_lo = bB_hi; bB_hi = bB_nx;
#undef WX
    };
    if constexpr (ROT) {
        int blk = blk_begin;
        for (; blk + 1 < blk_end; blk += 2) {
            block_body(std::integral_constant<int, 0>{}, blk);
            block_body(std::integral_constant<int, 1>{}, blk + 1);
        }
        if (blk < blk_end) block_body(std::integral_constant<int, 0>{}, blk);
    } else {
        for (int blk = blk_begin; blk < blk_end; ++blk) block_body(std::integral_constant<int, 0>{}, blk);
    }
    // back to the int32 states (direction words empty, rings and a-window to be primed by the caller's next step)
    // PAT: a lane behind LE goes back to NEG, as it came (its words are garbage by now); a pattern with the top bit set -- lane 0's
    // Lin, or what a dead column of lane LE may hold -- is NEG too
    const bool dead_lane = PAT && lane > LE;
    auto back = [&](const u32 v, const int half, const int base) -> int {
        if constexpr (PAT) return dead_lane ? NEG : pat_to_g4(half ? pat_hi(v) : pat_lo(v), base);
        else return h_to_g4(half ? hi_of(v) : lo_of(v), base);
    };
#pragma unroll
    for (int c = 0; c < C; ++c) {
        sta->Lp[c] = back(Lp[c], 0, baseA); stb->Lp[c] = back(Lp[c], 1, baseB);
        sta->acc[c] = 0; stb->acc[c] = 0;
    }
    sta->Lin = back(Lin, 0, baseA); stb->Lin = back(Lin, 1, baseB);
    sta->Lout = sta->Lp[C - 1]; stb->Lout = stb->Lp[C - 1];
}

// ---- the TOP blocks of both tasks, packed ---------------------------------------------------------------------------------
// Blocks [blk_begin, blk_end) still hold cells with pos <= 0 (the band's left triangle: rows < band + 1 - begin_a), but every
// lane is past its row 1.  What the reference's rules there (banded_smith_waterman.cc:111-133,143-155) come to, once the
// matrix is zero-initialised, is one thing: the cell with pos == -1 holds H = 0 when the pos == 0 cell of the next row takes
// it as its diag source and the pos == 0 cell of the same row as its left source (a gap from 0: -8, never -inf).  Everything
// further left can be -inf: as a left or diag source it would lose to those two anyway, and -inf is closed under the packed
// recurrences.  So a top block is a packed block plus
//   * one v_pk_max per cell (round 5, second form; it was a select on per-lane masks): the ring entry of a task's base -1 is
//     no look-up selector but a marker that v_perm turns into NaN, so every cell on the pos == -1 anti-diagonal computes NaN
//     (v_pk_fma and v_pk_maximum3 hand it on) and the maxNum with the row's tilted zero Z that follows makes it Z -- while a cell
//     right of it is unchanged, because it is >= Z anyway: left costs nothing in this tilt and the pos == 0 cell takes Z + 12 or
//     more from its diag source.  The cells LEFT of pos == -1 become Z or more instead of -inf: they only ever feed each other and
//     the marked cell.  No masks, no per-lane bookkeeping: the tasks of a wavefront may differ in begin_a at no cost (alignBlocks
//     starts every call at last match + gap, PctgBuilder.cc:1662-1669; the tails start at a seed, :1535-1611), and a task whose
//     band has left the triangle has no marker in range and no Z (its blocks here are plain packed blocks + a maxNum with -inf).
//     Z is relative to each task's base; a row without a pos == -1 cell inside the band, and the lanes behind the band, get -inf.
//   * a base that follows the tilted zero (16 per row) while a lane's column 0 is still left of pos == -1, so that the first
//     forced value of the lane is a small number;
//   * the pos == 0 cell of every row captured for the walk's side buffer, as the end blocks capture the pos == end_a cells.
// Written in source order (not the software-pipelined stream of pair_range).  In: the int32 states of the two tasks at the start of
// block blk_begin; out: their int32 states at the start of blk_end, where no cell left of pos == 0 is left in any lane's row
// (pair_range takes over from there).
// FS: some task is a force_start call -- beyond row 10 its pos == -1 cell is still H = 0 as a diag source but NO left source
// (banded_smith_waterman.cc:150-155): the chain takes maxNum(NaN, -inf) there while the stored row keeps the zero, a second
// v_pk_max per cell.
template <int C, int CE, int LPT = 64, bool FS = false>
__device__ __noinline__ void pair_top_range(BlockState<C>* sta, BlockState<C>* stb, const Tk* tpa, const Tk* tpb, const int blk_begin_, const int blk_end_, const int wlane)
{
    static_assert(CE >= 0 && CE < C - 1 && (LPT == QL || (C - 1) % 16 == 0), "band 512 on 64 lanes (transposed ring A) or band 150 on 16");
    typedef PRing<C, LPT> PR;
    const Tk ta = load_tk<LPT>(tpa), tb = load_tk<LPT>(tpb);
    const int blk_begin = uni(blk_begin_), blk_end = uni(blk_end_);
    const int lane = wlane & (LPT - 1);
    const int LE = (ta.Y - 1) / C;
    const int T0 = blk_begin * ROWS;
    const int km1A = ta.band - ta.begin_a - 1, km1B = tb.band - tb.begin_a - 1;   // ring index of a task's base -1 = the last row with a pos == -1 cell inside the band
    const int zk = 8 * km1A, zkB = 8 * km1B;   // tilted zero of the pos == -1 cell of row i: 8 * i + zk (task A; task B: zkB)
    u32 Lp[C], W[C + 15];
    int baseA, baseB;
    u32 Lin, dL, dR;
    {
        // the lane holds row rp; column c has pos = p0 + c
        const int rp = T0 - lane - 1, p0 = ta.begin_a + rp + C * lane - ta.band;
        const int p0B = tb.begin_a + rp + C * lane - tb.band;
        const bool dead0 = p0 < -1 && lane <= LE;   // column 0 (and the chain value about to arrive) still left of pos == -1
        const bool dead0B = p0B < -1 && lane <= LE;
        baseA = (sta->Lp[0] <= NEG / 2) ? 0 : (sta->Lp[0] >> 2);
        baseB = (stb->Lp[0] <= NEG / 2) ? 0 : (stb->Lp[0] >> 2);
        if (dead0) baseA = 16 * rp + 8 * C * lane;   // the tilted zero of column 0
        if (dead0B) baseB = 16 * rp + 8 * C * lane;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const bool dead = p0 + c < -1 && lane <= LE, deadB = p0B + c < -1 && lane <= LE;
            Lp[c] = pk(dead ? lo_of(PK_NINF) : g4_to_h(sta->Lp[c], baseA), deadB ? lo_of(PK_NINF) : g4_to_h(stb->Lp[c], baseB));
        }
        Lin = pk(dead0 ? lo_of(PK_NINF) : g4_to_h(sta->Lin, baseA), dead0B ? lo_of(PK_NINF) : g4_to_h(stb->Lin, baseB));
        const int lA = __shfl_up(baseA, 1, LPT), lB = __shfl_up(baseB, 1, LPT), rA = __shfl_down(baseA, 1, LPT), rB = __shfl_down(baseB, 1, LPT);
        const bool hasL = lane >= 1 && lane <= LE, hasR = lane < LE;
        dL = hasL ? pk((_Float16)(float)(lA - baseA), (_Float16)(float)(lB - baseB)) : 0u;
        dR = hasR ? pk((_Float16)(float)(rA - baseA), (_Float16)(float)(rB - baseB)) : 0u;
        const int64_t sa = ta.a_base + ta.begin_a - ta.band + (int64_t)(C - 1) * lane + T0, sb = tb.a_base + tb.begin_a - tb.band + (int64_t)(C - 1) * lane + T0;
        const u32 wa = fetch16(ta.a2, sa), wb = fetch16(tb.a2, sb);
        const u32 wa2 = (C - 1 > 16) ? fetch16(ta.a2, sa + 16) : 0u, wb2 = (C - 1 > 16) ? fetch16(tb.a2, sb + 16) : 0u;
        const int w0k = (C - 1) * lane + T0;   // ring index of W[0]
#pragma unroll
        for (int k = 0; k < C - 1; ++k) {
            const u32 cA = (k < 16) ? (wa >> (2 * k)) & 3u : (wa2 >> (2 * (k - 16))) & 3u, cB = (k < 16) ? (wb >> (2 * k)) & 3u : (wb2 >> (2 * (k - 16))) & 3u;
            W[k] = pk_sel((w0k + k == km1A) ? PR::MARK_A : cA, (w0k + k == km1B) ? PR::MARK_B : cB);
        }
#pragma unroll
        for (int k = C - 1; k < C + 15; ++k) W[k] = 0;
    }
    PR::template prime<true>(ta, tb, blk_begin, wlane, km1A, km1B);
    const int64_t iAa = ta.a_base + ta.begin_a - ta.band + (C - 1) * LPT, iBa = ta.b_base + ta.begin_b;
    const int64_t iAb = tb.a_base + tb.begin_a - tb.band + (C - 1) * LPT, iBb = tb.b_base + tb.begin_b;
    gcptr paA = ta.a2 + (iAa >> 4), pbA = ta.b2 + (iBa >> 4), paB = tb.a2 + (iAb >> 4), pbB = tb.b2 + (iBb >> 4);
    const u32 shaA = (u32)(iAa & 15) * 2u, shbA = (u32)(iBa & 15) * 2u, shaB = (u32)(iAb & 15) * 2u, shbB = (u32)(iBb & 15) * 2u;
    u32 aA_lo = paA[blk_begin + 1], aA_hi = paA[blk_begin + 2], bA_lo = pbA[blk_begin + 1], bA_hi = pbA[blk_begin + 2];
    u32 aB_lo = paB[blk_begin + 1], aB_hi = paB[blk_begin + 2], bB_lo = pbB[blk_begin + 1], bB_hi = pbB[blk_begin + 2];
    const h2 three = {(_Float16)3.0f, (_Float16)3.0f};
    const bool no_up = lane == LE;
    typedef Strip<LPT, true> ST;
    typedef PairFmt<C, LPT> FMT;
    constexpr int NB = ST::NB, FI = ST::FI;
    const int sshift = uni(ta.sshift);
    const bool edge = ST::opens_strip(wlane, sshift);
    const u32 my_slot = ST::slot_of(wlane, sshift);
    const u64 edge_mask = __ballot(edge);
    u32* const s_bnd = ST::staging();
    u32* const sb = s_bnd + my_slot;
    gptr const ckpt = ta.ckpt, bnd = ta.bnd;
    int xkeep = (int)PK_NINF;
    auto hf = [](const int v) -> _Float16 { return (_Float16)(float)v; };
    int g0A = baseA, g0B = baseB;   // GRP: the bases of the current group's checkpoint row (blk_begin is a group start)
    const int cap_max = cap_limit<C, LPT>(ta, lane);
    giptr const cap_slot = (giptr)unip(ta.dir);
    cap_table<LPT>(wlane, 0, ta.band - ta.begin_a, ta.X - 1, (int)(ta.pos0 - cap_slot), 0);
    cap_table<LPT>(wlane, 1, tb.band - tb.begin_a, tb.X - 1, (int)(tb.pos0 - cap_slot), 0);
    for (int blk = blk_begin; blk < blk_end; ++blk) {
        const int T = (blk + 1) * ROWS, tau0 = blk * ROWS;
        const u32 aA_nx = paA[blk + 3], bA_nx = pbA[blk + 3], aB_nx = paB[blk + 3], bB_nx = pbB[blk + 3];
        PR::template produce<true>(T, wlane, __builtin_amdgcn_alignbit(aA_hi, aA_lo, shaA), __builtin_amdgcn_alignbit(aB_hi, aB_lo, shaB),
                                   __builtin_amdgcn_alignbit(bA_hi, bA_lo, shbA), __builtin_amdgcn_alignbit(bB_hi, bB_lo, shbB), km1A, km1B);
        if ((blk & 3) == 0) {
            if constexpr (LPT == 64) {
                // the two-task kernel's slot holds ONE layout, the pattern format: the top blocks compute in f16 (the NaN marker
                // needs it) and convert what they store -- checkpoint rows here, boundary words below; the bases are the same
                u32 Pp[C];
#pragma unroll
                for (int c = 0; c < C; ++c) Pp[c] = h2_to_pat(Lp[c]);
                ck_store<C, LPT>(ckpt + (u64)(blk >> 2) * FMT::CK_WORDS, wlane, Pp, baseA, baseB);
            } else ck_store<C, LPT>(ckpt + (u64)(blk >> 2) * FMT::CK_WORDS, wlane, Lp, baseA, baseB);
            g0A = baseA; g0B = baseB;
        }
        if constexpr (!FMT::GRP) {
            if (edge) {
                gptr bb = bnd + (u64)blk * FMT::BND_WORDS + FMT::BND_VALS;
                bb[my_slot] = (u32)baseA;
                bb[NB + my_slot] = (u32)baseB;
            }
        }
        // GRP: the top blocks re-centre every block, but what a group stores is relative to the bases of its checkpoint row: the
        // boundary values leave with the (small, exact) difference added (-inf stays -inf)
        const u32 Kpk = FMT::GRP ? pk(hf(baseA - g0A), hf(baseB - g0B)) : 0u;
        const typename PR::APtr ringA_lane = PR::a_lane(tau0, wlane);
        const u32* const rbA = PR::b_lane(tau0, wlane, 0);
        const u32* const rbB = PR::b_lane(tau0, wlane, 1);
        static_for<ROWS>([&](auto rc) __attribute__((always_inline)) {
            constexpr int r = decltype(rc)::value;
            W[C - 1 + r] = PR::a_read(ringA_lane, r);
            const u32 tabA = rbA[r], tabB = rbB[r];
            const int row = tau0 + r - lane;
            // the tilted zero of this row's pos == -1 cell relative to the two bases: a small number in the lane that holds the cell
            // and in the dead lanes left of it, far below every value of the lanes right of it; -inf when the row has no such
            // cell inside the band (row > band - begin_a - 1) and in the lanes behind the band
            const int zg = 8 * row + zk, zgB = 8 * row + zkB;
            const bool zA = row <= km1A && lane <= LE, zB = row <= km1B && lane <= LE;
            const u32 Z = pk(zA ? hf(min(max(zg - baseA, -60000), 60000)) : lo_of(PK_NINF), zB ? hf(min(max(zgB - baseB, -60000), 60000)) : lo_of(PK_NINF));
            // FS: what the pos == -1 cell hands on as a LEFT source: nothing beyond row 10 of a force_start call
            u32 ZL = Z;
            if constexpr (FS) {
                const bool gA = ta.fs && row > FORCE_MAXGAP, gB = tb.fs && row > FORCE_MAXGAP;
                ZL = (gA ? 0x0000FC00u : (Z & 0x0000FFFFu)) | (gB ? 0xFC000000u : (Z & 0xFFFF0000u));
            }
            const u32 Lrecv = Lin;
            u32 L = Lin, x = PK_NINF;
            auto cell = [&](const int c) __attribute__((always_inline)) {
                const u32 m = __builtin_amdgcn_perm(tabB, tabA, W[r + c]);
                const h2 D = __builtin_elementwise_fma(as_h2(m), three, as_h2(Lp[c]));
                h2 U = as_h2((c < C - 1) ? Lp[(c < C - 1) ? c + 1 : c] : x);
                if (c == CE) U = as_h2(no_up ? PK_NINF : as_u(U));
                L = as_u(__builtin_elementwise_maximum(__builtin_elementwise_maximum(D, U), as_h2(L)));   // NaN on the pos == -1 anti-diagonal (m is)
                // H = 0 at pos == -1 (the reference's zero-initialised matrix): maxNum(NaN, Z) = Z
                Lp[c] = as_u(__builtin_elementwise_max(as_h2(L), as_h2(Z)));
                L = FS ? as_u(__builtin_elementwise_max(as_h2(L), as_h2(ZL))) : Lp[c];
            };
            cell(0);
            xkeep = lane_shl1<LPT>(xkeep, (int)Lp[0]);
            x = as_u(as_h2((u32)xkeep) + as_h2(dR));
            lds_store2_masked<4 * (r % FI) * NB, 4 * (NB * FI + (r % FI) * NB)>(sb, FMT::GRP ? as_u(as_h2(Lrecv) + as_h2(Kpk)) : h2_to_pat(Lrecv),
                                                                               FMT::GRP ? as_u(as_h2(Lp[0]) + as_h2(Kpk)) : h2_to_pat(Lp[0]), edge_mask);
#pragma unroll
            for (int c = 1; c < C; ++c) cell(c);
            Lin = (u32)lane_shr1<LPT>((int)Lin, (int)L);
            Lin = as_u(as_h2(Lin) + as_h2(dL));
            // the pos == 0 cell of this row, for the walk (side_capture above)
            side_capture<C, CE, LPT, false>(wlane, 0, tau0 + r, baseA, Lp, cap_max, cap_slot);
            side_capture<C, CE, LPT, false>(wlane, 1, tau0 + r, baseB, Lp, cap_max, cap_slot);
            if ((r % FI) == FI - 1) {
                constexpr u32 PER = 2u * NB * FI / 64u;
                const u32 w0 = (u32)wlane * PER;
                const u32* src = s_bnd + ST::staging_index(w0);
                gptr bp = bnd + (u64)blk * FMT::BND_WORDS + (u32)(r / FI) * (u32)(2 * NB * FI) + w0;
#pragma unroll
                for (u32 k = 0; k < PER; k += 4) {
                    const u32x4 v = {src[k * NB], src[(k + 1) * NB], src[(k + 2) * NB], src[(k + 3) * NB]};
                    *(g4ptr)(bp + k) = v;
                }
            }
        });
        {   // re-centre on column 0 after every block; a lane whose column 0 is still left of pos == -1 follows the tilted zero
            // (what such a lane holds meanwhile is no longer -inf but Z or more, growing by up to 13 per row: not a value to centre on)
            const float fa = (float)lo_of(Lp[0]), fb = (float)hi_of(Lp[0]);
            const int rpn = T - lane - 1;   // the row the lane holds now; its column 0 has pos = begin_a + rpn + C lane - band
            const bool followA = lane <= LE && ta.begin_a + rpn + C * lane - ta.band < -1, followB = lane <= LE && tb.begin_a + rpn + C * lane - tb.band < -1;
            const bool oka = !followA && fa > -60000.0f && fa < 60000.0f, okb = !followB && fb > -60000.0f && fb < 60000.0f;
            const _Float16 step = (_Float16)(float)(16 * ROWS);
            const u32 d = pk(oka ? lo_of(Lp[0]) : (followA ? step : (_Float16)0.0f), okb ? hi_of(Lp[0]) : (followB ? step : (_Float16)0.0f));
            baseA += oka ? (int)fa : (followA ? 16 * ROWS : 0);
            baseB += okb ? (int)fb : (followB ? 16 * ROWS : 0);
#pragma unroll
            for (int c = 0; c < C; ++c) Lp[c] = as_u(as_h2(Lp[c]) - as_h2(d));
            Lin = as_u(as_h2(Lin) - as_h2(d));
            const u32 dl = (u32)lane_shr1<LPT>((int)d, (int)d);
            const u32 dr = (u32)lane_shl1<LPT>((int)d, (int)d);
            if (lane >= 1 && lane <= LE) dL = as_u(as_h2(dL) + as_h2(dl) - as_h2(d));
            if (lane < LE) dR = as_u(as_h2(dR) + as_h2(dr) - as_h2(d));
        }
#pragma unroll
        for (int k = 0; k < C - 1; ++k) W[k] = W[k + ROWS];
        aA_lo = aA_hi; aA_hi = aA_nx; bA_lo = bA_hi; bA_hi = bA_nx;
        aB_lo = aB_hi; aB_hi = aB_nx; bB_lo = bB_hi; bB_hi = bB_nx;
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        sta->Lp[c] = h_to_g4(lo_of(Lp[c]), baseA); stb->Lp[c] = h_to_g4(hi_of(Lp[c]), baseB);
        sta->acc[c] = 0; stb->acc[c] = 0;
    }
    sta->Lin = h_to_g4(lo_of(Lin), baseA); stb->Lin = h_to_g4(hi_of(Lin), baseB);
    sta->Lout = sta->Lp[C - 1]; stb->Lout = stb->Lp[C - 1];
}

// re-prime one task's rings and a-window at block `blk` (after the packed range)
template <int C, bool HASN, bool UNTAGGED, int LPT = 64>
__device__ __noinline__ void single_resume(BlockState<C>* st, const Tk* tp, const int blk_, const int lane)
{
    const Tk t = load_tk<LPT>(tp);
    u32 W[C + 15];
    single_prime<C, HASN, UNTAGGED, LPT>(t, uni(blk_), lane, W);
#pragma unroll
    for (int k = 0; k < C - 1; ++k) st->W[k] = W[k];
}
