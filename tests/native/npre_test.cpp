// Test of npre_window_has_n / call_touches_n (gam_ngs_amd/csrc/gamdp_dev.h: the host's and the chain kernels' choice between the
// N-aware and the N-free cells, by the window a call touches on a VIEW of a sequence) against brute force on an explicitly built
// view; built with g++ under ASan + UBSan and run by tests/test_views_cpu.py.  For lengths around multiples of 256 and every
// (rc, off, lo, hi) of a grid with negative lo, hi past the end and off == len:
//   never `false` when bases [lo, hi] of the view hold an N (what the kernels' correctness rests on);
//   `false` when no N lies within the 256-base blocks of the stored sequence the window touches (so "always true" does not pass).
#include <cstdio>
#include <vector>

#include "gamdp_dev.h"

using namespace gamdp;

static uint64_t rnd(uint64_t& s) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }

struct Seq {
    std::vector<uint8_t> fwd;   // stored, forward orientation (4 = N)
    std::vector<u32> pre;       // as SeqSet::upload builds it; empty: no N
    void finish()
    {
        bool any = false;
        for (uint8_t c : fwd) any |= c == 4;
        pre.clear();
        if (!any) return;
        pre.assign((fwd.size() + 255) / 256 + 1, 0);
        for (size_t k = 0; k < fwd.size(); k++) pre[k / 256 + 1] += fwd[k] == 4;
        for (size_t k = 1; k < pre.size(); k++) pre[k] += pre[k - 1];
    }
    const u32* p() const { return pre.empty() ? nullptr : pre.data(); }
    // the view, explicitly: reverse complement first (N stays N), then the suffix
    std::vector<uint8_t> view(bool rc, size_t off) const
    {
        std::vector<uint8_t> x(fwd);
        if (rc) { for (size_t i = 0; i < x.size(); i++) x[i] = fwd[fwd.size() - 1 - i] == 4 ? 4 : (uint8_t)(fwd[fwd.size() - 1 - i] ^ 1); }
        return std::vector<uint8_t>(x.begin() + (long)off, x.end());
    }
};

// truth on the view `v`; and the conservative bound: an N within the 256-blocks of the stored sequence that [lo, hi] of the view touches
static void brute(const Seq& s, const std::vector<uint8_t>& v, const std::vector<uint8_t>& blk_n, bool rc, size_t off, int64_t lo, int64_t hi,
                  bool* truth, bool* blocks)
{
    *truth = *blocks = false;
    const int64_t n = (int64_t)s.fwd.size();
    for (int64_t p = lo < 0 ? 0 : lo; p <= hi && p < (int64_t)v.size(); p++) {
        if (v[(size_t)p] == 4) *truth = true;
        const int64_t o = (int64_t)off + p, f = rc ? n - 1 - o : o;   // where base p of the view lies in the stored sequence
        if (blk_n[(size_t)(f / 256)]) *blocks = true;
    }
}
static std::vector<uint8_t> blocks_with_n(const Seq& s)
{
    std::vector<uint8_t> r(s.fwd.size() / 256 + 1, 0);
    for (size_t k = 0; k < s.fwd.size(); k++) if (s.fwd[k] == 4) r[k / 256] = 1;
    return r;
}

int main()
{
    long bad = 0, n_true = 0, n_false = 0, n_cons = 0, checked = 0;
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    const int lens[] = {0, 1, 255, 256, 257, 300, 511, 512, 513, 768, 1000, 1281};
    for (int len : lens) {
        for (int pattern = 0; pattern < 6; pattern++) {
            Seq s;
            s.fwd.resize((size_t)len);
            for (auto& c : s.fwd) c = (uint8_t)(rnd(seed) & 3);
            // N patterns: none; one at the first / last base; one at a block edge; a few single N; a run across a block edge
            if (len > 0) {
                if (pattern == 1) s.fwd[0] = 4;
                if (pattern == 2) s.fwd[(size_t)len - 1] = 4;
                if (pattern == 3) s.fwd[(size_t)((len > 256 ? 256 : len / 2) - (len > 256 && (rnd(seed) & 1) ? 1 : 0))] = 4;
                if (pattern == 4) for (int k = 0; k < 3; k++) s.fwd[(size_t)(rnd(seed) % (uint64_t)len)] = 4;
                if (pattern == 5 && len > 260) for (int k = 250; k < 260; k++) s.fwd[(size_t)k] = 4;
            }
            s.finish();
            std::vector<int64_t> grid = {-400, -64, -1, 0, 1, 63, 64, 255, 256, 257, 300, 511, 512};
            for (int64_t d : {-257, -256, -255, -65, -64, -2, -1, 0, 1, 64, 400}) grid.push_back(len + d);
            std::vector<size_t> offs = {0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257};
            for (int d : {-257, -256, -65, -2, -1, 0}) if (len + d >= 0) offs.push_back((size_t)(len + d));
            const std::vector<uint8_t> blk_n = blocks_with_n(s);
            for (int rc = 0; rc < 2; rc++)
                for (size_t off : offs) {
                    if (off > (size_t)len) continue;   // (prepare_task settles off > len as INVALID before any window is looked at)
                    const std::vector<uint8_t> v = s.view(rc != 0, off);
                    for (int64_t lo : grid)
                        for (int64_t hi : grid) {
                            bool truth, blocks;
                            brute(s, v, blk_n, rc != 0, off, lo, hi, &truth, &blocks);
                            const bool got = npre_window_has_n(s.p(), len, rc != 0, off, lo, hi);
                            checked++;
                            if (truth && !got) { if (bad++ < 10) std::printf("MISSED N: len %d pattern %d rc %d off %zu lo %ld hi %ld\n", len, pattern, rc, off, (long)lo, (long)hi); }
                            if (!blocks && got) { if (bad++ < 10) std::printf("N WHERE NONE IS NEAR: len %d pattern %d rc %d off %zu lo %ld hi %ld\n", len, pattern, rc, off, (long)lo, (long)hi); }
                            n_true += truth; n_false += !blocks; n_cons += blocks && !truth;
                        }
                }
        }
    }
    // call_touches_n: the two windows of a call (pos = begin_a - band + x + y on a, the rows on b), `margin` on either side
    {
        Seq a, b;
        a.fwd.resize(1500); b.fwd.resize(1300);
        for (int round = 0; round < 400; round++) {
            for (auto& c : a.fwd) c = (uint8_t)(rnd(seed) & 3);
            for (auto& c : b.fwd) c = (uint8_t)(rnd(seed) & 3);
            if (round % 4 != 3) (round % 2 ? a : b).fwd[(size_t)(rnd(seed) % 1300)] = 4;
            if (round % 8 == 0) a.fwd[(size_t)(rnd(seed) % 1500)] = 4;
            a.finish(); b.finish();
            const bool arc = rnd(seed) & 1, brc = rnd(seed) & 1;
            const size_t aoff = (size_t)(rnd(seed) % 700), boff = (size_t)(rnd(seed) % 600);
            const int64_t band = (int64_t)(rnd(seed) % 200), begin_a = (int64_t)(rnd(seed) % 800), begin_b = (int64_t)(rnd(seed) % 700);
            const int64_t X = 1 + (int64_t)(rnd(seed) % 600), margin = 64;
            bool ta, ba_, tb, bb;
            brute(a, a.view(arc, aoff), blocks_with_n(a), arc, aoff, begin_a - band - margin, begin_a + X - 1 + band + margin, &ta, &ba_);
            brute(b, b.view(brc, boff), blocks_with_n(b), brc, boff, begin_b - margin, begin_b + X - 1 + margin, &tb, &bb);
            const bool got = call_touches_n(a.p(), 1500, arc, aoff, b.p(), 1300, brc, boff, band, begin_a, begin_b, X, margin);
            checked++;
            if ((ta || tb) && !got) { if (bad++ < 10) std::printf("call_touches_n MISSED N: round %d\n", round); }
            if (!(ba_ || bb) && got) { if (bad++ < 10) std::printf("call_touches_n: N WHERE NONE IS NEAR: round %d\n", round); }
            n_true += ta || tb; n_false += !(ba_ || bb);
        }
    }
    std::printf("checked %ld windows: %ld hold an N, %ld have none near, %ld only near; bad %ld\n", checked, n_true, n_false, n_cons, bad);
    return bad != 0 || n_true < 1000 || n_false < 1000 || n_cons < 1000;
}
