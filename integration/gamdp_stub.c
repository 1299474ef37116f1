/* Stand-in for libgamdp.so on a host WITHOUT an MI355X / hipcc, for ONE purpose: building the patched gam-merge so that
 * its own CPU path can write the golden-vector dump (GAMDP_DUMP_PREFIX, integration/make_l1_dump.sh).  It exports the
 * entry points integration/GamdpBridge.cc binds (include/gamdp.h) and refuses every one of them with GAMDP_ENODEV, which
 * makes the bridge report "using the CPU alignment" -- gam-merge then runs exactly the reference's code.  Never shipped,
 * never used by the product or its tests: the real library is gam_ngs_amd/libgamdp.so. */
#include "gamdp.h"

int gamdp_multi_create(const int* devices, int n, gamdp_multi** out) { (void)devices; (void)n; if (out) *out = 0; return GAMDP_ENODEV; }
void gamdp_multi_destroy(gamdp_multi* m) { (void)m; }
const char* gamdp_multi_last_error(const gamdp_multi* m) { (void)m; return "gamdp stub library: no GPU implementation on this host"; }
int gamdp_multi_seqset_create(gamdp_multi* m, const uint8_t* const* seqs, const uint64_t* lens, uint32_t n, int is_ascii, gamdp_multi_seqset** out)
{ (void)m; (void)seqs; (void)lens; (void)n; (void)is_ascii; if (out) *out = 0; return GAMDP_ENODEV; }
void gamdp_multi_seqset_destroy(gamdp_multi_seqset* s) { (void)s; }
int gamdp_multi_align_merge_blocks(gamdp_multi* m, const gamdp_multi_seqset* master, const gamdp_multi_seqset* slave, const gamdp_mb_in* in,
                                   size_t n, uint32_t band, gamdp_mb_out* out, gamdp_result* audit, uint32_t audit_stride)
{ (void)m; (void)master; (void)slave; (void)in; (void)n; (void)band; (void)out; (void)audit; (void)audit_stride; return GAMDP_ENODEV; }
/* (a bridge that opts in to GAMDP_WALK_SKIP_DIAG on the contexts of its handle links against these two; there is no context here) */
int gamdp_ctx_set_walk_skip(gamdp_ctx* ctx, int mode) { (void)ctx; (void)mode; return GAMDP_ENODEV; }
int gamdp_ctx_walk_skip_stats(const gamdp_ctx* ctx, gamdp_walk_skip_stats* out) { (void)ctx; (void)out; return GAMDP_ENODEV; }
/* (... and to the same test in the two-task band-512 kernel) */
int gamdp_ctx_set_walk_skip_pair(gamdp_ctx* ctx, int mode) { (void)ctx; (void)mode; return GAMDP_ENODEV; }
int gamdp_ctx_walk_skip_pair_stats(const gamdp_ctx* ctx, gamdp_walk_skip_pair_stats* out) { (void)ctx; (void)out; return GAMDP_ENODEV; }
/* (... and in the int32 direction-free kernels) */
int gamdp_ctx_set_walk_skip_i32(gamdp_ctx* ctx, int mode) { (void)ctx; (void)mode; return GAMDP_ENODEV; }
int gamdp_ctx_walk_skip_i32_stats(const gamdp_ctx* ctx, gamdp_walk_skip_i32_stats* out) { (void)ctx; (void)out; return GAMDP_ENODEV; }
/* (a bridge that opts in to GAMDP_OPS_WALK_RUNS for the edit strings of its batches links against these two) */
int gamdp_ctx_set_ops_walk(gamdp_ctx* ctx, int mode)
{ return ((mode != GAMDP_OPS_WALK_STEPS && mode != GAMDP_OPS_WALK_RUNS) || !ctx) ? GAMDP_EINVAL : GAMDP_ENODEV; }
int gamdp_ctx_ops_walk_stats(const gamdp_ctx* ctx, gamdp_ops_walk_stats* out) { return (!ctx || !out) ? GAMDP_EINVAL : GAMDP_ENODEV; }
/* (a bridge that checks the edit strings of its batches links against these three; the fingerprint needs no device and is the real one) */
int gamdp_carry_ops_batch(gamdp_ctx* ctx, const gamdp_seqset* set_a, const gamdp_seqset* set_b, const gamdp_task* tasks, size_t n,
                          gamdp_result* out, uint32_t* ops_fp)
{ (void)ctx; (void)set_a; (void)set_b; (void)tasks; (void)n; (void)out; (void)ops_fp; return GAMDP_ENODEV; }
int gamdp_ctx_carry_ops_info(const gamdp_ctx* ctx, gamdp_score_launch_info* out, size_t cap, size_t* n)
{ (void)ctx; (void)out; (void)cap; if (n) *n = 0; return GAMDP_ENODEV; }
/* (a bridge that takes the fingerprints of its batches' edit strings from the device links against these five; the bound on an edit
 * string's length needs no device and is the real one: the pre-checks of banded_smith_waterman.cc:90-132 as gamdp_task_preflight
 * makes them, then X + min(X + 2 band, |a|, begin_a + X + band) rounded up to 16 -- tests/test_ops_fp_cabi.py compares the two) */
int gamdp_align_batch_fp(gamdp_ctx* ctx, const gamdp_seqset* set_a, const gamdp_seqset* set_b, const gamdp_task* tasks, size_t n,
                         gamdp_result* out, uint32_t* ops_fp)
{ (void)n; if (!ctx || !set_a || !set_b || !out || !ops_fp || (n && !tasks)) return GAMDP_EINVAL; return GAMDP_ENODEV; }
int gamdp_ctx_set_ops_chunk_bytes(gamdp_ctx* ctx, uint64_t bytes) { (void)bytes; return ctx ? GAMDP_ENODEV : GAMDP_EINVAL; }
int gamdp_ops_fingerprint_batch(gamdp_ctx* ctx, const uint8_t* ops, const uint64_t* off, const uint64_t* len, size_t n, uint32_t* fp)
{ (void)ops; if (!ctx || !fp || (n && (!off || !len))) return GAMDP_EINVAL; return GAMDP_ENODEV; }
int gamdp_ctx_ops_fp_info(const gamdp_ctx* ctx, gamdp_ops_fp_info* out) { return (!ctx || !out) ? GAMDP_EINVAL : GAMDP_ENODEV; }
uint64_t gamdp_task_ops_cap(uint64_t alen, uint64_t blen, uint32_t band32, uint64_t begin_a, uint64_t end_a, uint64_t begin_b,
                            uint64_t end_b, int force_start, int force_end)
{
    const uint64_t band = band32;
    const int64_t maxgap = 10;   /* FORCE_MAXGAP_LEN */
    int64_t lo, hi, up;
    uint64_t X, lim, by_band, by_view, bound;
    (void)force_end;             /* (it moves the end cell, not the bound) */
    if (end_b < begin_b) return 0;                                   /* :90, EMPTY */
    if (begin_a >= (1ull << 31) - 65536) return 0;                   /* INVALID */
    if (begin_b >= blen) return 0;                                   /* OUT_OF_RANGE or INVALID */
    if (end_b >= blen) end_b = blen - 1;                             /* :91 */
    X = end_b - begin_b + 1;                                         /* :93-95 */
    lim = alen + band - begin_a;
    if (lim < X) X = lim;
    if (X > 500000) X = 500000;
    if (X == 0) return 0;                                            /* INVALID */
    lo = (int64_t)begin_a - (int64_t)band > 0 ? (int64_t)begin_a - (int64_t)band : 0;
    hi = (int64_t)begin_a + (int64_t)band;
    if (force_start) {                                               /* row 0 reads a.at(pos) for 0 <= pos <= 10 in the band (:116) */
        up = hi < maxgap ? hi : maxgap;
        if (lo <= up && up >= (int64_t)alen) return 0;               /* OUT_OF_RANGE */
    }
    if (begin_a > alen + band) return 0;                             /* every cell beyond |a|: OUT_OF_RANGE or EMPTY */
    by_band = X + 2 * band;
    by_view = begin_a + X + band < alen ? begin_a + X + band : alen;
    bound = X + (by_band < by_view ? by_band : by_view);
    if (bound == 0) bound = 1;
    return (bound + 15) / 16 * 16;
}
uint32_t gamdp_ops_fingerprint(const uint8_t* ops, uint64_t n)
{
    uint32_t f = 0;
    uint64_t i;
    if (!ops) return 0;
    for (i = 0; i < n; i++) f = f * GAMDP_OPS_FP_MULT + ((uint32_t)ops[i] + 1u);
    return f;
}
/* (the live width of a call needs no device and is the real one: the pre-checks of gamdp_task_preflight, then the closed form
 * include/gamdp.h states -- tests/test_carry_wide_cabi.py compares the two) */
uint64_t gamdp_task_live_columns(uint64_t alen, uint64_t blen, uint32_t band32, uint64_t begin_a, uint64_t end_a, uint64_t begin_b,
                                 uint64_t end_b, int force_start, int force_end)
{
    /* a call the pre-checks let through has an edit-string bound (gamdp_task_ops_cap above makes the same pre-checks) */
    const int64_t band = band32;
    int64_t A0, last, i, right, left, w;
    uint64_t X, lim;
    if (gamdp_task_ops_cap(alen, blen, band32, begin_a, end_a, begin_b, end_b, force_start, force_end) == 0 || alen == 0) return 0;
    if (end_b >= blen) end_b = blen - 1;
    X = end_b - begin_b + 1;
    lim = alen + (uint64_t)band - begin_a;
    if (lim < X) X = lim;
    if (X > 500000) X = 500000;
    if (alen > (1ull << 62)) alen = 1ull << 62;
    A0 = (int64_t)begin_a - band;
    last = (int64_t)alen - 1 - A0;
    i = -A0 < last - 2 * band ? -A0 : last - 2 * band;
    if (i < 0) i = 0;
    if (i > (int64_t)X - 1) i = (int64_t)X - 1;
    right = 2 * band < last - i ? 2 * band : last - i;
    left = A0 + i < 0 ? A0 + i : 0;
    w = right + left + 1;
    return w > 0 ? (uint64_t)w : 0;
}
