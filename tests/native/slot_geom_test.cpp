// Test of the rules gamdp_dev.h states once for the host and the kernels (gam_ngs_amd/csrc/gamdp_dev.h): band_cols / gen_kernel_id
// (the instantiation a band takes) and dir_words_for / slot_geom (the layout of a scratch slot, shared by the launch planner and the
// merge-block driver's chain slots).  Built with g++ under ASan + UBSan and run by tests/test_slot_geom.py; no HIP.
// The KernelInfo rows are the test's own (the word counts of the real table come from the kernels' headers); the expected numbers are
// literals.  One of them by hand: 5 columns, 320 words per block, a direction per cell, one task, 1000 rows at band 150 -- LE = 300 / 5
// = 60, (999 + 60) / 16 + 1 = 67 blocks of 320 = 21440 direction words (a multiple of 64), side buffers of (302 + 63) / 64 * 64 = 320,
// so 21440 + 4 * 320 = 22720 words and no live-row or boundary store.
#include <cstdio>

#include "gamdp_dev.h"

using namespace gamdp;

static int bad = 0;
#define CHECK(c) do { if (!(c)) { bad++; std::printf("line %d: %s\n", __LINE__, #c); } } while (0)

static_assert(band_cols(0) == 2 && band_cols(150) == 5 && band_cols(543) == 17, "band_cols is a constant expression");

//                            id         name         C   band tasks waves N      dirfree two-img dir-block ckpt  bnd   kernel
static const KernelInfo ONE_DIR = {K_C5_CE0, "one_dir", 5, 150, 1, 20, false, false, false, 320, 320, 512, nullptr};     // K_C5_CE0-shaped
static const KernelInfo ONE_DIR3 = {K_GEN_C3, "one_dir3", 3, 0, 1, 20, true, false, false, 192, 192, 512, nullptr};      // K_GEN_C3-shaped
static const KernelInfo ONE_DF9 = {K_GEN_C9, "one_df9", 9, 0, 1, 20, true, true, false, 768, 768, 512, nullptr};         // K_GEN_C9-shaped
static const KernelInfo PAIR17 = {K_P17_CE4, "pair17", 17, 512, 2, 16, false, true, true, 1280, 2304, 1088, nullptr};    // K_P17_CE4-shaped
static const KernelInfo OCTO19 = {K_O19_CE15, "octo19", 19, 150, 8, 16, false, true, true, 1280, 2432, 640, nullptr};    // K_O19_CE15-shaped

struct Case { const KernelInfo* ki; u64 X; u32 band; SlotGeom want; };   // want: dir_words, ypad, slot_words, ckpt_off, bnd_off
static const Case CASES[] = {
    {&ONE_DIR, 1u, 150u, {1280u, 320u, 2560u, 0u, 0u}},
    {&ONE_DIR, 17u, 150u, {1600u, 320u, 2880u, 0u, 0u}},
    {&ONE_DIR, 1000u, 150u, {21440u, 320u, 22720u, 0u, 0u}},   // (the one worked out above)
    {&ONE_DIR, 499999u, 150u, {10001280u, 320u, 10002560u, 0u, 0u}},
    {&ONE_DIR3, 1u, 90u, {768u, 192u, 1536u, 0u, 0u}},
    {&ONE_DIR3, 17u, 90u, {960u, 192u, 1728u, 0u, 0u}},
    {&ONE_DIR3, 1000u, 90u, {12864u, 192u, 13632u, 0u, 0u}},
    {&ONE_DIR3, 499999u, 90u, {6000768u, 192u, 6001536u, 0u, 0u}},
    {&ONE_DF9, 1u, 287u, {3072u, 576u, 12288u, 5376u, 7680u}},
    {&ONE_DF9, 17u, 287u, {3840u, 576u, 13568u, 6144u, 8448u}},
    {&ONE_DF9, 1000u, 287u, {51456u, 576u, 105216u, 53760u, 68352u}},
    {&ONE_DF9, 499999u, 287u, {24003072u, 576u, 46011904u, 24005376u, 30007296u}},
    {&PAIR17, 1u, 512u, {8960u, 1088u, 48896u, 26624u, 35840u}},
    {&PAIR17, 17u, 512u, {10240u, 1088u, 52544u, 29184u, 38400u}},
    {&PAIR17, 1000u, 512u, {89600u, 1088u, 313280u, 187904u, 231680u}},
    {&PAIR17, 499999u, 512u, {40008960u, 1088u, 132047744u, 80026624u, 98034688u}},
    {&OCTO19, 1u, 150u, {5120u, 320u, 33536u, 20480u, 27776u}},
    {&OCTO19, 17u, 150u, {6400u, 320u, 36736u, 23040u, 30336u}},
    {&OCTO19, 1000u, 150u, {85760u, 320u, 274048u, 181760u, 227968u}},
    {&OCTO19, 499999u, 150u, {40005120u, 320u, 119032320u, 80020480u, 99026560u}},
};

int main()
{
    // the smallest C of 2, 3, 5, 9, 17 with 2 * band + 1 <= 64 * C, and the K_GEN_* row of that C
    static const struct { u32 band; int cols; KernelId kid; } BANDS[] = {
        {0, 2, K_GEN_C2}, {63, 2, K_GEN_C2}, {64, 3, K_GEN_C3}, {95, 3, K_GEN_C3}, {96, 5, K_GEN_C5}, {150, 5, K_GEN_C5}, {159, 5, K_GEN_C5},
        {160, 9, K_GEN_C9}, {287, 9, K_GEN_C9}, {288, 17, K_GEN_C17}, {512, 17, K_GEN_C17}, {543, 17, K_GEN_C17},
    };
    for (const auto& b : BANDS) {
        CHECK(band_cols(b.band) == b.cols);
        CHECK(gen_kernel_id(band_cols(b.band)) == (int)b.kid);
        CHECK(FAMILY_COLS[cols_index(b.cols)] == b.cols);
    }
    CHECK(band_cols(544) == 17 && band_cols(1u << 20) == 17);   // (wider bands: the callers' own guards)

    for (const Case& c : CASES) {
        const KernelInfo& ki = *c.ki;
        const u64 dir = dir_words_for(ki, c.X, c.band);
        const SlotGeom g = slot_geom(ki, dir, c.band);
        const bool same = g.dir_words == c.want.dir_words && g.ypad == c.want.ypad && g.slot_words == c.want.slot_words &&
                          g.ckpt_off == c.want.ckpt_off && g.bnd_off == c.want.bnd_off;
        if (!same) {
            bad++;
            std::printf("%s X %llu band %u: dir %llu ypad %u slot %llu ckpt %llu bnd %llu\n", ki.name, (unsigned long long)c.X, c.band, (unsigned long long)g.dir_words,
                        g.ypad, (unsigned long long)g.slot_words, (unsigned long long)g.ckpt_off, (unsigned long long)g.bnd_off);
        }
        // what holds for every slot: the direction words hold the image and are whole 64-word lines; the side buffers hold a band row;
        // the stores lie in order behind the images and the side buffers, inside the slot
        const u64 images = ki.two_dir_images ? 2 : 1, sides = 4ull * g.ypad * (u64)ki.tasks_per_wave;
        CHECK(g.dir_words % 64 == 0 && g.dir_words >= dir && g.dir_words < dir + 64);
        CHECK(g.ypad % 64 == 0 && g.ypad >= 2 * c.band + 2);
        CHECK(images * g.dir_words + sides <= g.slot_words);
        if (ki.tasks_per_wave > 1 || ki.dirfree) {
            CHECK(g.ckpt_off == images * g.dir_words + sides);
            CHECK(g.ckpt_off < g.bnd_off && g.bnd_off < g.slot_words);
        } else {
            CHECK(g.ckpt_off == 0 && g.bnd_off == 0 && g.slot_words == images * g.dir_words + sides);
        }
    }
    // K_WIDE keeps the band matrix itself
    {
        static const KernelInfo WIDE = {K_WIDE, "wide", 0, 0, 1, 8, true, false, false, 1, 1, 512, nullptr};
        CHECK(dir_words_for(WIDE, 1000, 600) == 1000ull * 1201ull);
        const SlotGeom g = slot_geom(WIDE, 1000ull * 1201ull, 600);
        CHECK(g.dir_words == 1201024u && g.ypad == 1216u && g.slot_words == 1201024u + 4u * 1216u && g.ckpt_off == 0 && g.bnd_off == 0);
    }
    std::printf("slot_geom_test: %zu cases, bad %d\n", sizeof(CASES) / sizeof(CASES[0]), bad);
    return bad ? 1 : 0;
}
