// Test of the pattern format of the two-task band-512 kernel (gam_ngs_amd/csrc/gamdp_dev.h: PAT_OFF, PAT_MIN, PAT_MAX, pat_encode,
// pat_decode; the argument is in kernel_pair.inc), exhaustively on the CPU; built with g++ under ASan + UBSan and run by
// tests/test_pattern_order.py.  The kernel keeps a half-word as the integer PAT_OFF + (value - base), hands it to v_pk_maximum3_f16
// as if it were an f16, and forms the diag candidate of both tasks with ONE 32-bit integer add.  That rests on three facts:
//   1. over all patterns 0x0400 ... 0x7BFF and 0xFC00 ("no source", -inf) the order as _Float16 equals the order as uint16_t, with
//      0xFC00 below everything (what the device's instruction returns is checked on the GPU: tools/valu_rate7.hip);
//   2. for every pair of live patterns (PAT_MIN ... PAT_MAX) the 32-bit add of (sB << 16) | sA, s = 12 or 21, equals two independent
//      16-bit adds, and the sums are finite, normal f16 patterns again;
//   3. pat_encode / pat_decode round-trip every value - base whose pattern is live, and every pattern with the top bit set decodes
//      below every live one.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "gamdp_dev.h"

using namespace gamdp;

// the number an f16 bit pattern stands for (IEEE 754 binary16, exact in a float; not every g++ has _Float16)
static float as_half(uint16_t p)
{
    const int e = (p >> 10) & 31, m = p & 1023;
    float v;
    if (e == 31) v = m ? NAN : INFINITY;
    else if (e == 0) v = std::ldexp((float)m, -24);
    else v = std::ldexp((float)(1024 + m), e - 25);
    return (p & 0x8000u) ? -v : v;
}

int main()
{
    long bad = 0, n = 0;
    // 1. the order
    static uint16_t pat[0x7C00 - 0x0400 + 1];
    int np = 0;
    pat[np++] = 0xFC00u;
    for (uint32_t p = 0x0400u; p <= 0x7BFFu; ++p) pat[np++] = (uint16_t)p;
    for (int i = 0; i + 1 < np; ++i, ++n) {
        // consecutive in integer order (0xFC00 first): strictly increasing as numbers -- hence the same order over all pairs
        const float lo = (float)as_half(pat[i]), hi = (float)as_half(pat[i + 1]);
        if (!(lo < hi)) ++bad;
        if (i > 0 && !(pat[i] < pat[i + 1])) ++bad;
    }
    // ... and over pairs spread across the range, both ways round
    for (int i = 0; i < np; i += 61) {
        for (int j = 0; j < np; j += 67, ++n) {
            const bool num = (float)as_half(pat[i]) < (float)as_half(pat[j]);
            const bool integer = (pat[i] == 0xFC00u ? -1 : (int)pat[i]) < (pat[j] == 0xFC00u ? -1 : (int)pat[j]);
            if (num != integer) ++bad;
        }
    }
    // every live pattern is a normal number (maximum3 hands normal operands back bit for bit), and stays finite under + 21
    static_assert(PAT_MIN == 0x0400u && PAT_MAX + 21u == 0x7BFFu, "the asserted range");
    static_assert(PAT_OFF > PAT_MIN && PAT_OFF < PAT_MAX, "the offset is a live pattern");
    // 2. the packed add: low halves over the whole live range (the carry can only come from there), high halves spread + the extremes
    const uint32_t s[2] = {12u, 21u};
    for (uint32_t a = PAT_MIN; a <= PAT_MAX; ++a) {
        for (uint32_t b = PAT_MIN; b <= PAT_MAX; b = (b < PAT_MIN + 64 || b + 64 >= PAT_MAX) ? b + 1 : (b + 997 < PAT_MAX - 64 ? b + 997 : PAT_MAX - 64)) {
            for (int i = 0; i < 4; ++i, ++n) {
                const uint32_t sa = s[i & 1], sb = s[i >> 1];
                const uint32_t packed = ((b << 16) | a) + ((sb << 16) | sa);
                const uint16_t lo = (uint16_t)(a + sa), hi = (uint16_t)(b + sb);
                if (packed != (((uint32_t)hi << 16) | lo)) ++bad;
                if (lo < 0x0400u || lo > 0x7BFFu || hi < 0x0400u || hi > 0x7BFFu) ++bad;
            }
        }
    }
    // 3. encode / decode
    for (int rel = (int)PAT_MIN - (int)PAT_OFF; rel <= (int)PAT_MAX - (int)PAT_OFF; ++rel, ++n) {
        const u32 p = pat_encode(rel);
        if (p != PAT_OFF + (u32)rel || p < PAT_MIN || p > PAT_MAX) ++bad;
        if (pat_decode(p) != rel) ++bad;
    }
    const int lowest_live = pat_decode(PAT_MIN);
    for (uint32_t p = 0x8000u; p <= 0xFFFFu; ++p, ++n) {
        if (!(pat_decode(p) < lowest_live)) ++bad;
    }
    if (pat_decode(0xFC00u) != -1024 - (int)PAT_OFF) ++bad;
    std::printf("checked %ld, bad %ld\n", n, bad);
    return bad ? 1 : 0;
}
