/* gamdp.h -- C ABI of libgamdp: MI355X (gfx950) implementation of gam-merge's contig-pair
 * alignment hot path.  Plain C types only; no C++/torch types cross this boundary.
 *
 * What each entry point replaces in the reference (paths relative to the reference repo):
 *
 *   gamdp_align_batch          N independent calls of
 *                              BandedSmithWaterman(band).find_alignment(a,begin_a,end_a,b,begin_b,end_b,
 *                              force_start,force_end)        lib/include/alignment/banded_smith_waterman.hpp:66-71
 *                              (lib/src/alignment/banded_smith_waterman.cc:69-322) plus the
 *                              first_match_pos / last_match_pos scans of each result
 *                              (lib/src/alignment/my_alignment.cc:167-193, 228-262).
 *   gamdp_find_hits            ABlast(word).findHits(...)    lib/src/alignment/ablast.cc:41-76
 *   gamdp_find_hits_batch      N independent calls of ABlast(word).findHits(...) on the GPU, over uploaded sequence sets
 *                              (lib/src/alignment/ablast.cc:41-76, lib/include/alignment/ablast.hpp:53-99).
 *   gamdp_align_merge_blocks   the loop `for list: for mb: builder.alignMergeBlock(graph,*mb)`
 *                              lib/src/pctg/BuildPctgFunctions.cc:82-84, i.e. N calls of
 *                              PctgBuilder::alignMergeBlock  lib/src/pctg/PctgBuilder.cc:726-844
 *                              (findBestAlignment :1361-1614, alignBlocks :1617-1708, is_good :1711-1730).
 *   gamdp_seqset_*             the RefSequence vectors filled by loadSequences
 *                              (lib/include/assembly/io_contig.code.hpp:568-596) -- uploaded once per GPU.
 *   gamdp_encode / _revcomp    Nucleotide(char) (lib/include/assembly/nucleotide.code.hpp:47-75) and
 *                              reverse_complement (lib/include/assembly/contig.code.hpp:187-229).
 *
 * Conventions: every function returns 0 on success or a negative GAMDP_E* code; nothing throws;
 * the caller owns every buffer it passes; a gamdp_ctx binds one GPU + one HIP stream and must be
 * used by one host thread at a time (one ctx per thread / per GPU).  There is NO CPU fallback:
 * with no usable gfx950 device gamdp_ctx_create fails with GAMDP_ENODEV.
 */
#ifndef GAMDP_H
#define GAMDP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GAMDP_VERSION 1

/* error codes (negative return values) */
#define GAMDP_EINVAL  (-1)  /* bad argument                                        */
#define GAMDP_ENODEV  (-2)  /* no usable GPU / HIP runtime failure at context setup */
#define GAMDP_ENOMEM  (-3)  /* host or device allocation failed                    */
#define GAMDP_ENOTSUP (-4)  /* band wider than GAMDP_MAX_BAND                          */
#define GAMDP_EHIP    (-5)  /* a HIP call failed at run time (see gamdp_last_error) */

/* per-task status, mirrors the reference's observable outcomes */
#define GAMDP_ST_OK           0 /* a MyAlignment was produced                                          */
#define GAMDP_ST_EMPTY        1 /* reference returns MyAlignment() (banded_smith_waterman.cc:90, :215) */
#define GAMDP_ST_OUT_OF_RANGE 2 /* reference throws std::out_of_range from Contig::at; gam-merge then
                                   drops the whole graph (lib/src/pctg/ThreadedBuildPctg.cc:322-329)   */
#define GAMDP_ST_INVALID      3 /* arguments for which the reference has undefined behaviour           */
#define GAMDP_ST_DIAG_RANGE   9 /* libgamdp_diag.so only (never the product library): a packed-f16 block of this task held
                                   a value outside the exactly representable range -- the assertion behind the range argument
                                   of DESIGN.md section 4; the parity campaigns run on that build and expect none           */

/* edit-string alphabet (lib/include/alignment/my_alignment.hpp:57-62) */
#define GAMDP_OP_GAP_A 0
#define GAMDP_OP_GAP_B 1
#define GAMDP_OP_MATCH 2
#define GAMDP_OP_MISMATCH 3

#define GAMDP_DEFAULT_BAND 150   /* DEFAULT_BAND_SIZE, banded_smith_waterman.hpp:38 */
/* The reference takes any band (banded_smith_waterman.hpp:66).  So does this library, up to GAMDP_MAX_BAND = 2^20 (beyond it the
 * reference's own index arithmetic is untested and the oracle declines): bands up to GAMDP_MAX_TUNED_BAND run on the systolic
 * kernels (2*band+1 <= 64 lanes x 17 columns), wider ones on a correct-at-any-speed kernel that keeps the whole band matrix
 * (x_size * (2*band+1) int32) in the scratch arena -- a call whose matrix does not fit the arena fails with GAMDP_ENOMEM. */
#define GAMDP_MAX_BAND 1048576
#define GAMDP_MAX_TUNED_BAND 543

typedef struct gamdp_ctx gamdp_ctx;
typedef struct gamdp_seqset gamdp_seqset;
typedef struct gamdp_fasta gamdp_fasta;

/* One find_alignment call.  Sequences are referenced by index into a seqset; *_rc selects the
 * reverse complement of that sequence (the reference reverse-complements the slave contig in
 * place, PctgBuilder.cc:1443, 1467); *_off makes the sequence a suffix view seq[off..] (the
 * reference's chop_begin copy, PctgBuilder.cc:1577, 1596).  Coordinates are relative to the view. */
typedef struct gamdp_task {
    uint32_t a_id, b_id;
    uint64_t a_off, b_off;
    uint8_t a_rc, b_rc, force_start, force_end;
    uint32_t band;
    uint64_t begin_a, end_a, begin_b, end_b;
} gamdp_task;

/* What the callers of find_alignment consume (PctgBuilder.cc:761-762, 787, 801, 1516-1517, 1672).
 * homology is (double)(n_match*100)/(double)length, or 0 when length==0, exactly as
 * banded_smith_waterman.cc:319; it is filled in on the host. */
typedef struct gamdp_result {
    uint64_t begin_a, begin_b;   /* MyAlignment::begin_a / begin_b                          */
    int64_t score;               /* MyAlignment::score                                      */
    uint64_t n_match, length;    /* #MATCH ops, #ops                                        */
    uint64_t first_a, first_b;   /* first_match_pos                                         */
    uint64_t last_a, last_b;     /* last_match_pos                                          */
    uint64_t cells;              /* x_size*y_size of the reference's fill loops (GCUPS unit) */
    double homology;
    uint8_t first_found, last_found; /* bool results of first/last_match_pos               */
    uint8_t status;              /* GAMDP_ST_*                                              */
    uint8_t pad_[5];
} gamdp_result;

/* Optional edit strings: ops[task i] occupies ops_buf[ops_off[i] .. ops_off[i]+length) in forward
 * order, truncated to ops_cap[i].  The caller fills ops_off/ops_cap; pass NULL to skip. */
typedef struct gamdp_ops {
    uint8_t* ops_buf;
    const uint64_t* ops_off;
    const uint64_t* ops_cap;
} gamdp_ops;

/* Block / Frame fields the merge-block driver reads (Frame::getBegin/getEnd/getStrand,
 * Block::getReadsNumber; lib/src/assembly/Frame.cc:100-127, Block.cc:79-82). */
typedef struct gamdp_block {
    int32_t m_begin, m_end, s_begin, s_end;
    char m_strand, s_strand;
    int64_t n_reads;
} gamdp_block;

/* MergeBlock (lib/include/pctg/MergeDescriptor.hpp:40-69): inputs the driver reads ... */
typedef struct gamdp_mb_in {
    int32_t m_id, s_id;                       /* indices into the master / slave seqsets */
    uint8_t m_ltail, m_rtail, s_ltail, s_rtail;
    uint32_t n_blocks;
    const gamdp_block* blocks;                /* graph.getBlocks(mb.vertex), in list order */
} gamdp_mb_in;

/* ... and the fields it writes. coords_set==0 means the reference returned before writing
 * align_rev/m_start/... (PctgBuilder.cc:825-829) so the caller must leave them untouched. */
typedef struct gamdp_mb_out {
    uint8_t align_ok, align_rev;
    uint8_t status;       /* GAMDP_ST_OK, or OUT_OF_RANGE/INVALID: the reference would throw -> drop graph */
    uint8_t coords_set;
    int32_t m_start, m_end, s_start, s_end;
    uint32_t n_dp;        /* find_alignment calls made for this merge block */
    uint64_t cells;       /* sum of their cells                              */
} gamdp_mb_out;

/* ---- context ------------------------------------------------------------------------------ */
int gamdp_ctx_create(int device, gamdp_ctx** out);
void gamdp_ctx_destroy(gamdp_ctx* ctx);
/* bound the scratch arena (direction matrix) in bytes; 0 = default (75 % of free HBM) */
int gamdp_ctx_set_arena_bytes(gamdp_ctx* ctx, uint64_t bytes);
const char* gamdp_last_error(const gamdp_ctx* ctx);
/* the hipStream_t the kernels run on, as an opaque pointer */
void* gamdp_ctx_stream(gamdp_ctx* ctx);
/* HIP-event timing of the DP kernel launches since the last reset: total ms and launch count.  Launches of one call that run side
 * by side (a batch's small N-aware launch beside its big launch, each on a stream of its own) count with the time the GPU was busy
 * with them -- the union of their intervals --, not with the sum of their durations. */
int gamdp_ctx_kernel_time(gamdp_ctx* ctx, double* total_ms, uint64_t* launches, int reset);
/* What the last gamdp_align_batch call on this context launched, in launch order (the pieces of a batch that went through in
 * pieces included): the library's own account of its launch planner's choices (which kernel instantiation a group of calls
 * took, how many wavefront slots, how many rounds) and of what the wavefronts then did on the device (counted there).
 * No reference counterpart: BandedSmithWaterman::find_alignment (banded_smith_waterman.cc:69) is one code path. */
typedef struct gamdp_launch_info {
    char kernel[40];                 /* the instantiation, e.g. "k_align_o<19,15>" */
    uint32_t n_aware;                /* 1: the instantiation handles N (v_dot8 cells) */
    uint32_t tasks_per_wavefront;    /* 1, 2, 4 or 8 */
    uint32_t tasks;                  /* calls in the launch (the copies that fill up its last wavefront not counted) */
    uint32_t units;                  /* wavefront units handed out: tasks / pairs / quads / octets */
    uint32_t slots;                  /* resident wavefronts = scratch slots */
    uint32_t band_max;               /* widest band among the calls */
    uint32_t units_dirfree;          /* units that ran a direction-free range (counted on the device) */
    uint32_t units_packed_top;       /* ... whose blocks with pos <= 0 cells ran packed (device) */
    uint32_t units_packed_top_mixed; /* ... of those, through the per-task form: calls that differ in begin_a / force_start calls (device) */
    uint32_t strips;                 /* strip re-creations (materialise calls) of the launch's walks (device) */
    uint32_t piece;                  /* piece of a batch that went through in pieces (0 = the whole batch / its first piece) */
    uint32_t units_top_wanted;       /* units with a packed range whose calls hold blocks with pos <= 0 cells behind the ramp: what packed top blocks are for (device) */
    double rounds;                   /* units / slots */
    double kernel_ms;                /* HIP events around the launch, on the stream it ran on (this launch alone: side-by-side launches overlap) */
} gamdp_launch_info;
/* copies up to `cap` records to out (may be NULL when cap == 0); *n = how many launches the call made */
int gamdp_ctx_launch_info(const gamdp_ctx* ctx, gamdp_launch_info* out, size_t cap, size_t* n);

/* How the walks of the eight-task band-150 kernel ("k_align_o<19,15>") cross the rows whose directions the fill did not keep.
 *   GAMDP_WALK_STRIPS     the default: the directions of every group of 64 rows on the path are re-created (a strip call).
 *   GAMDP_WALK_SKIP_DIAG  opt-in: a walk that stands on a block without directions first compares H(x, y) - H(x - 64, y), two
 *       values the fill stored, with the score sum of the 64 base pairs between them.  The reference's traceback tests diag first
 *       (banded_smith_waterman.cc:265-285) and its fill makes every cell >= its diag candidate (:158-168), so equality proves 64
 *       diagonal steps: the walk takes them at once, eight groups per test, and asks for a strip only where the test fails.
 * Results do not depend on the mode.  Every other kernel (one-, two-, four-task, generic, the merge-block chains) ignores it.
 * gamdp_multi_* honours each context's own setting (gamdp_multi_ctx); GAMDP_WALK_SKIP=1 in the environment (read once per
 * process) makes SKIP_DIAG the mode of new contexts. */
#define GAMDP_WALK_STRIPS     0   /* default */
#define GAMDP_WALK_SKIP_DIAG  1
int gamdp_ctx_set_walk_skip(gamdp_ctx* ctx, int mode);   /* GAMDP_EINVAL for NULL / unknown mode (mode checked first) */
/* What the eight-task launches of the last gamdp_align_batch on this context counted on the device, summed over the call's
 * launches and pieces; all counters 0 when the call made no eight-task launch, everything 0 before the first call. */
typedef struct gamdp_walk_skip_stats {
    uint64_t tests;            /* times a walk ran the test (one test looks at up to 8 groups below the walk) */
    uint64_t groups_tested;    /* groups whose equality was evaluated (both stored rows exist, the span stays in x >= 1, pos >= 1) */
    uint64_t groups_skipped;   /* groups a walk jumped over */
    uint64_t rows_skipped;     /* rows of those (64 each; the span below a walk's end cell ends on the next stored row: 1..64) */
    uint64_t strips;           /* strip re-creations of those launches (the sum of their gamdp_launch_info.strips) */
    uint32_t mode;             /* GAMDP_WALK_* the call ran in */
    uint32_t pad_;
} gamdp_walk_skip_stats;       /* 48 bytes */
int gamdp_ctx_walk_skip_stats(const gamdp_ctx* ctx, gamdp_walk_skip_stats* out);   /* GAMDP_EINVAL for NULL ctx / out */

/* The same choice for the walks of the two-task band-512 kernel ("k_align_p<17,4>"), a property of its own: the modes are
 * GAMDP_WALK_STRIPS (the default) and GAMDP_WALK_SKIP_DIAG as above, and the test is the same one, read off that kernel's checkpoint
 * rows.  It covers both ways the kernel walks: its two tasks side by side (launches of few rounds) and one task after the other with
 * the whole wavefront (long launches), where up to 64 groups are tested at a time.  A task whose edit string is wanted keeps its
 * strips.  Results do not depend on the mode.  The two properties are independent: gamdp_ctx_set_walk_skip leaves the two-task
 * kernel alone, this one leaves the eight-task kernel (and every other kernel) alone.  gamdp_multi_* honours each context's own
 * setting; GAMDP_WALK_SKIP_PAIR=1 in the environment (read once per process) makes SKIP_DIAG the mode of new contexts. */
int gamdp_ctx_set_walk_skip_pair(gamdp_ctx* ctx, int mode);   /* GAMDP_EINVAL for NULL / unknown mode (mode checked first) */
/* What the two-task launches of the last gamdp_align_batch on this context counted on the device, summed over the call's launches
 * and pieces; everything 0 (`mode` too) when the call made no two-task launch, and before the first call. */
typedef struct gamdp_walk_skip_pair_stats {
    uint64_t tests;            /* as in gamdp_walk_skip_stats (one test looks at up to 8 groups side by side, up to 64 one by one) */
    uint64_t groups_tested;
    uint64_t groups_skipped;
    uint64_t rows_skipped;
    uint64_t strips;           /* strip re-creations of those launches (the sum of their gamdp_launch_info.strips) */
    uint32_t mode;             /* GAMDP_WALK_* the call ran in */
    uint32_t launches_side_by_side;   /* two-task launches that walked their two tasks side by side ... */
    uint32_t launches_one_by_one;     /* ... and one task after the other */
    uint32_t pad_;
} gamdp_walk_skip_pair_stats;  /* 56 bytes */
int gamdp_ctx_walk_skip_pair_stats(const gamdp_ctx* ctx, gamdp_walk_skip_pair_stats* out);   /* GAMDP_EINVAL for NULL ctx / out */

/* The same choice for the walks of the int32 direction-free kernels, a third property: "k_align<17,4,false>" and
 * "k_align<17,4,true>" (band 512, one task per wavefront), "k_align_q<19,15,false>" and "k_align_q<19,15,true>" (band 150, four
 * tasks per wavefront), "k_align<9,-1,true>" and "k_align<17,-1,true>" (every band from 160 to 543 other than 512).  The modes are
 * GAMDP_WALK_STRIPS (the default) and GAMDP_WALK_SKIP_DIAG as above; the test is the same one, read off those kernels' int32
 * checkpoint rows, with the reference's three-valued score where a sequence may hold N (N against N scores as a match, N against
 * a base 0; both are MATCH ops).  Up to 64 groups are tested at a time.  A task whose edit string is wanted keeps its strips (so
 * gamdp_align_batch_fp does); the chain kernels of gamdp_align_merge_blocks and "k_align_w" do not have the test.  Results do not
 * depend on the mode.  The three properties are independent: each leaves the kernels of the other two alone.  gamdp_multi_*
 * honours each context's own setting; GAMDP_WALK_SKIP_I32=1 in the environment (read once per process) makes SKIP_DIAG the mode
 * of new contexts. */
int gamdp_ctx_set_walk_skip_i32(gamdp_ctx* ctx, int mode);   /* GAMDP_EINVAL for NULL / unknown mode (mode checked first) */
/* What the launches of those six kernels in the last gamdp_align_batch on this context counted on the device, summed over the
 * call's launches and pieces; everything 0 (`mode` too) when the call made no such launch, and before the first call. */
typedef struct gamdp_walk_skip_i32_stats {
    uint64_t tests;            /* as in gamdp_walk_skip_stats (one test looks at up to 64 groups) */
    uint64_t groups_tested;
    uint64_t groups_skipped;
    uint64_t rows_skipped;
    uint64_t strips;           /* strip re-creations of those launches (the sum of their gamdp_launch_info.strips) */
    uint32_t mode;             /* GAMDP_WALK_* the call ran in */
    uint32_t launches;         /* the call's launches of the six kernels */
} gamdp_walk_skip_i32_stats;   /* 48 bytes */
int gamdp_ctx_walk_skip_i32_stats(const gamdp_ctx* ctx, gamdp_walk_skip_i32_stats* out);   /* GAMDP_EINVAL for NULL ctx / out */

/* Whether walks in GAMDP_WALK_SKIP_DIAG mode back off from the test after failures, a fourth property: it applies to whichever
 * of the three properties above is in SKIP_DIAG mode and does nothing where none is.  A failed test is a memory round trip in
 * front of the strip call it did not save, and the indel rate of a pair is about the same all along it.
 *   GAMDP_WALK_BACKOFF_OFF  the default: every point where a walk runs out of directions is tested.
 *   GAMDP_WALK_BACKOFF_ON   each walk counts the tests in a row that skipped nothing (`fails`).  After such a test its next
 *       gamdp_walk_skip_backoff_hold(fails) = min(2^fails - 1, a cap) such points pass without a test and without a load: the
 *       walk asks for its strip at once, as after a failed test.  A test that skips at least one group puts fails back to 0.
 * Results do not depend on the mode.  A task whose edit string is wanted never tests and never holds.  gamdp_multi_* honours
 * each context's own setting; GAMDP_WALK_SKIP_BACKOFF=1 in the environment (read once per process) makes ON the mode of new
 * contexts. */
#define GAMDP_WALK_BACKOFF_OFF 0   /* default */
#define GAMDP_WALK_BACKOFF_ON  1
int gamdp_ctx_set_walk_skip_backoff(gamdp_ctx* ctx, int mode);   /* GAMDP_EINVAL for NULL / unknown mode (mode checked first) */
/* The schedule itself (host only, no context): 0 for fails == 0, non-decreasing, 2^fails - 1 up to the cap the device code uses. */
uint32_t gamdp_walk_skip_backoff_hold(uint32_t fails);
/* The points the walks of the last gamdp_align_batch on this context passed without a test, per kernel family (the families of
 * the three properties above), summed over the call's launches and pieces: tests of gamdp_walk_skip*_stats + held = the points a
 * walk in BACKOFF_OFF mode would have tested on the same path.  Everything 0 before the first call. */
typedef struct gamdp_walk_skip_backoff_stats {
    uint64_t held;             /* eight-task launches ("k_align_o<19,15>") */
    uint64_t held_pair;        /* two-task launches ("k_align_p<17,4>"), both ways it walks */
    uint64_t held_i32;         /* launches of the six int32 direction-free kernels */
    uint32_t mode;             /* GAMDP_WALK_BACKOFF_* the call ran in */
    uint32_t pad_;
} gamdp_walk_skip_backoff_stats;   /* 32 bytes */
int gamdp_ctx_walk_skip_backoff_stats(const gamdp_ctx* ctx, gamdp_walk_skip_backoff_stats* out);   /* GAMDP_EINVAL for NULL ctx / out */

/* How the walks of the thirteen systolic kernels (every kernel of gamdp_launch_info but "k_align_w") write the edit string of a call
 * that wants one: gamdp_align_batch with a gamdp_ops, every call of gamdp_align_batch_fp.
 *   GAMDP_OPS_WALK_STEPS  the default: such a walk takes one step per iteration and writes one op.
 *   GAMDP_OPS_WALK_RUNS   opt-in: away from row 0 and pos == 0 such a walk consumes a whole run of diagonal steps per iteration, as
 *       the walk of a call without a string does, and the 64 lanes that compared the run's bases write its MATCH / MISMATCH ops, 16
 *       steps each.  Gap steps, row 0 and pos == 0 stay single steps.
 * Results and the bytes of every edit string (clipped ones too: nothing is written at or behind a string's capacity) do not depend on
 * the mode.  "k_align_w", the merge-block chains and calls that want no string ignore it; a walk that wants a string makes no
 * diagonal test in either mode.  gamdp_multi_* honours each context's own setting; GAMDP_OPS_WALK_RUNS=1 in the environment (read once
 * per process) makes RUNS the mode of new contexts. */
#define GAMDP_OPS_WALK_STEPS 0   /* default */
#define GAMDP_OPS_WALK_RUNS  1
int gamdp_ctx_set_ops_walk(gamdp_ctx* ctx, int mode);   /* GAMDP_EINVAL for NULL / unknown mode (mode checked first) */
/* What the walks of the last gamdp_align_batch / gamdp_align_batch_fp on this context that wrote their string in RUNS mode counted
 * on the device, summed over the call's launches, pieces and chunks.  Steps, not bytes: an op clipped by its string's capacity
 * counts.  ops_by_run + ops_by_step = the sum of gamdp_result.length over the counted calls with status GAMDP_ST_OK.  In STEPS
 * mode, and before the first call, the four counters are 0; "k_align_w" calls are never counted. */
typedef struct gamdp_ops_walk_stats {
    uint64_t tasks;            /* calls that wanted a string and walked in RUNS mode (whatever their status) */
    uint64_t ops_by_run;       /* ops of run iterations: the diagonal steps taken from cells with x >= 1 and pos >= 1 */
    uint64_t ops_by_step;      /* every other op of those walks (gaps, row 0, pos == 0) */
    uint64_t runs;             /* run iterations that took at least one step */
    uint32_t mode;             /* GAMDP_OPS_WALK_* the call ran in */
    uint32_t pad_;
} gamdp_ops_walk_stats;        /* 40 bytes */
int gamdp_ctx_ops_walk_stats(const gamdp_ctx* ctx, gamdp_ops_walk_stats* out);   /* GAMDP_EINVAL for NULL ctx / out */

/* ---- sequences ---------------------------------------------------------------------------- */
/* seqs[i] points to lens[i] bytes: ASCII bases when is_ascii!=0 (normalised like Nucleotide(char)),
 * else base codes A=0 T=1 C=2 G=3 N=4.  Packs to 2 bit + N mask and uploads to the ctx's GPU. */
int gamdp_seqset_create(gamdp_ctx* ctx, const uint8_t* const* seqs, const uint64_t* lens, uint32_t n,
                        int is_ascii, gamdp_seqset** out);
void gamdp_seqset_destroy(gamdp_seqset* set);
uint32_t gamdp_seqset_size(const gamdp_seqset* set);
uint64_t gamdp_seqset_length(const gamdp_seqset* set, uint32_t id);

/* ---- FASTA loader (input side of the path; lib/include/assembly/io_contig.code.hpp:511-596) ------------- */
/* Reads a (multi-)FASTA file with the reference's rules: name = header up to the first blank, every character
 * other than newline / blank is a base through Nucleotide(char) (unknown -> N).  No GPU needed. */
int gamdp_fasta_open(const char* path, gamdp_fasta** out);
void gamdp_fasta_close(gamdp_fasta* f);
uint32_t gamdp_fasta_count(const gamdp_fasta* f);
const char* gamdp_fasta_name(const gamdp_fasta* f, uint32_t i);
const uint8_t* gamdp_fasta_codes(const gamdp_fasta* f, uint32_t i, uint64_t* len);
/* sequence i of the set = record i of the file */
int gamdp_seqset_create_from_fasta(gamdp_ctx* ctx, const gamdp_fasta* f, gamdp_seqset** out);

/* ---- .blocks files (gam-create's output, gam-merge's input; lib/src/assembly/Block.cc:669-690, 737-747, 795-807,
 *      Frame.cc:197-222) -------------------------------------------------------------------------------------- */
/* One line = numReads, then for the master and for the slave frame: 0 ctgId strand begin end blockReadsLen readsLen
 * (tab separated on output, any blanks on input).  Lines that are empty or start with '#' are skipped, lines that do
 * not parse are dropped silently, blocks with numReads < min_block_size are dropped (loadBlocks, :669-690). */
typedef struct gamdp_block_rec {
    int64_t n_reads;
    uint64_t m_block_reads_len, m_reads_len, s_block_reads_len, s_reads_len;
    int32_t m_ctg, m_begin, m_end, s_ctg, s_begin, s_end;
    char m_strand, s_strand;
    uint8_t pad_[6];
} gamdp_block_rec;
typedef struct gamdp_blocks gamdp_blocks;
int gamdp_blocks_open(const char* path, int64_t min_block_size, gamdp_blocks** out);
void gamdp_blocks_close(gamdp_blocks* b);
uint64_t gamdp_blocks_count(const gamdp_blocks* b);
const gamdp_block_rec* gamdp_blocks_data(const gamdp_blocks* b);
/* writeBlocks (:737-747): the header line, then one block per line */
int gamdp_blocks_write(const char* path, const gamdp_block_rec* recs, uint64_t n);

/* ---- L0: batch of independent banded alignments ------------------------------------------- */
/* a sequences come from set_a, b sequences from set_b (may be the same set). */
int gamdp_align_batch(gamdp_ctx* ctx, const gamdp_seqset* set_a, const gamdp_seqset* set_b,
                      const gamdp_task* tasks, size_t n, gamdp_result* out, const gamdp_ops* ops_or_null);

/* What gamdp_align_batch decides for one call before anything is launched, on plain numbers (view lengths alen / blen):
 * the checks of banded_smith_waterman.cc:90-132 in the reference's order.  Returns GAMDP_ST_OK when the call needs the
 * DP (it would be launched), otherwise the final status (EMPTY / OUT_OF_RANGE / INVALID) the batch call reports without
 * launching.  *cells (may be NULL) = x_size * y_size, the GCUPS unit and the weight the multi-GPU partitioner balances. */
int gamdp_task_preflight(uint64_t alen, uint64_t blen, uint32_t band, uint64_t begin_a, uint64_t end_a, uint64_t begin_b,
                         uint64_t end_b, int force_start, int force_end, uint64_t* cells);

/* Score and end cell of BandedSmithWaterman(band).find_alignment(...) without the traceback: the fill
 * (banded_smith_waterman.cc:80-171) and the end-cell search (:173-215).  score = MyAlignment::score()
 * (max_score, :189/:207); (end_a, end_b) = the end cell's position in the a view and in b
 * (pos = begin_a + max_i + max_j - band, begin_b + max_i); last_pos (my_alignment.cc:197-226) of the alignment
 * the reference would return is (end_a + 1, end_b + 1). */
typedef struct gamdp_score_result {
    int64_t score;
    uint64_t end_a, end_b;
    uint64_t cells;          /* as gamdp_result.cells */
    uint8_t status;          /* GAMDP_ST_*, equal to what gamdp_align_batch reports for the same task */
    uint8_t pad_[7];
} gamdp_score_result;        /* 40 bytes */
/* Tasks as for gamdp_align_batch (reverse-complement and suffix views, a band per task); status, score and cells of every task equal
 * those of its gamdp_result, the cases gamdp_task_preflight settles included, and GAMDP_ST_EMPTY (no end cell, :215) /
 * GAMDP_ST_OUT_OF_RANGE (the end cell's pos >= |a|: the traceback's a.at(pos) throws) decided at the end cell.  For a status other
 * than GAMDP_ST_OK score, end_a and end_b are 0.
 * A second implementation, not a mode of the alignment kernels: every cell is computed in int32, one call per wavefront, by a kernel
 * that shares no code with them.  It keeps no direction and no row of the matrix -- the end cell is searched while the cells are
 * computed -- so the scratch arena (gamdp_ctx_set_arena_bytes) is NOT used: a batch too large for the arena can be scored, and a
 * gamdp_align_batch run can be checked on the device it ran on (tools/score_crosscheck.py).  Exact arithmetic and no scratch are what
 * it offers; it makes no promise of speed.
 * GAMDP_EINVAL for NULL ctx / sets / out, NULL tasks with n > 0, ids out of range and reverse complements of a packed-only set (as
 * gamdp_align_batch); n == 0 succeeds.  Bands above GAMDP_MAX_TUNED_BAND are not taken: a batch that holds one returns
 * GAMDP_ENOTSUP as a whole (gamdp_last_error names the task; the context stays usable).  tasks must not change before the call
 * returns.  The launches count toward gamdp_ctx_kernel_time; gamdp_ctx_launch_info keeps describing the last gamdp_align_batch. */
int gamdp_score_batch(gamdp_ctx* ctx, const gamdp_seqset* set_a, const gamdp_seqset* set_b,
                      const gamdp_task* tasks, size_t n, gamdp_score_result* out);
/* What the last gamdp_score_batch call on this context launched, in launch order: one launch per instantiation its bands take. */
typedef struct gamdp_score_launch_info {
    char kernel[24];         /* the instantiation, e.g. "k_score<5>" */
    uint32_t cols;           /* band columns per lane, as the wavefronts of the launch reported it with their results (0: they differ) */
    uint32_t tasks;          /* calls in the launch */
    uint32_t slots;          /* resident wavefronts */
    uint32_t band_max;       /* widest band among the calls */
    double kernel_ms;        /* HIP events around the launch */
} gamdp_score_launch_info;   /* 48 bytes */
/* copies up to `cap` records to out (may be NULL when cap == 0); *n = how many launches the call made */
int gamdp_ctx_score_info(const gamdp_ctx* ctx, gamdp_score_launch_info* out, size_t cap, size_t* n);

/* The whole result of BandedSmithWaterman(band).find_alignment(...) from a fill alone.  The reference's traceback
 * (banded_smith_waterman.cc:227-311) is a pointer chase whose step from a cell depends only on that cell's value and its three
 * neighbours' values (:229-308), which the fill holds when it computes the cell; so every cell carries the summary of the traceback
 * that would start in it -- where it ends (:321), its ops, its MATCH ops (:239, :274), its first and last MATCH
 * (first_match_pos, my_alignment.cc:167-193; last_match_pos, :228-262) -- made from the summary of the cell the step leads to, and
 * the summary of the end cell (:173-215) is the result.
 * Tasks as for gamdp_align_batch.  Every field of every gamdp_result equals what gamdp_align_batch writes for the same task, the cases
 * gamdp_task_preflight settles included, and GAMDP_ST_EMPTY (:215) / GAMDP_ST_OUT_OF_RANGE (the traceback's a.at(pos) throws) decided
 * at the end cell; homology is computed on the host from n_match and length (:319).  There is no edit string.
 * What it is for: a check of gamdp_align_batch's traceback half -- strips, re-created directions, walks, side captures -- on the
 * device the batch ran on, call by call at any scale (tools/score_crosscheck.py --carry), as gamdp_score_batch is of its fill.  A
 * third implementation: int32, one call per wavefront, by a kernel that shares its sequence windows and scoring rows with
 * gamdp_score_batch's and no code with the alignment kernels.  It keeps no direction and no row of the matrix, and the scratch arena
 * (gamdp_ctx_set_arena_bytes) is NOT used.  It makes no promise of speed.
 * Refusals as gamdp_score_batch: GAMDP_EINVAL for NULL ctx / sets / out, NULL tasks with n > 0, ids out of range and reverse
 * complements of a packed-only set; n == 0 succeeds; a batch that holds a band above GAMDP_MAX_TUNED_BAND returns GAMDP_ENOTSUP as a
 * whole (gamdp_last_error names the task; the context stays usable).  tasks must not change before the call returns.  The launches
 * count toward gamdp_ctx_kernel_time; gamdp_ctx_launch_info and gamdp_ctx_score_info keep describing their own calls. */
int gamdp_carry_batch(gamdp_ctx* ctx, const gamdp_seqset* set_a, const gamdp_seqset* set_b,
                      const gamdp_task* tasks, size_t n, gamdp_result* out);
/* What the last gamdp_carry_batch call on this context launched, in launch order: one launch ("k_carry<5>") per instantiation its
 * bands take; the fields as for gamdp_ctx_score_info. */
int gamdp_ctx_carry_info(const gamdp_ctx* ctx, gamdp_score_launch_info* out, size_t cap, size_t* n);

/* A fingerprint of an edit string over the public alphabet (GAMDP_OP_*), in forward order as gamdp_ops delivers it:
 *     F(empty) = 0,    F(s . e) = F(s) * GAMDP_OPS_FP_MULT + (e + 1)   (mod 2^32).
 * A total function of the bytes, on the host, without a context: any byte value e contributes e + 1, and n == 0 or ops == NULL
 * gives 0.
 * What it guarantees (the multiplier M is odd, and two ops differ by 0 < |d| <= 3):
 *   - two strings of equal length that differ in exactly one op differ in F: the difference is d * M^k, which has at most one
 *     factor of 2 (M^k is odd) and so is not 0 mod 2^32;
 *   - two strings that differ by swapping two adjacent unequal ops differ in F: the difference is d * (M - 1) * M^k, and
 *     M - 1 = 2^4 * 0x9E3779B with 0x9E3779B odd, so it has at most five factors of 2 and is not 0 mod 2^32.
 * Any other pair of different strings collides with probability about 2^-32 per comparison. */
#define GAMDP_OPS_FP_MULT 0x9E3779B1u
uint32_t gamdp_ops_fingerprint(const uint8_t* ops, uint64_t n);

/* gamdp_carry_batch with the fingerprint of the edit string: out[i] is exactly what gamdp_carry_batch writes, and ops_fp[i] is
 * gamdp_ops_fingerprint of the edit string the reference would return for task i -- the bytes gamdp_align_batch delivers through
 * gamdp_ops -- and 0 for every status other than GAMDP_ST_OK, the cases gamdp_task_preflight settles included.  There is still no
 * edit string: the forward edit string of a cell is that of the cell the traceback's step leads to plus one op, so the fingerprint
 * is a sixth field of the summary a cell carries (k_carry_f<C>: no directions, no walk, no scratch arena).
 * What it is for: two edit strings can agree in begin, length, n_match, first and last match and still differ (a GAP_A / GAP_B
 * pair taken in the other order); comparing ops_fp[i] with the fingerprint of the bytes gamdp_align_batch returned checks every
 * op of every string on the device the batch ran on, call by call (tools/score_crosscheck.py --ops).
 * Refusals as gamdp_carry_batch, with NULL ops_fp among the NULL arguments (GAMDP_EINVAL); n == 0 succeeds; a batch that holds a band
 * above GAMDP_MAX_TUNED_BAND returns GAMDP_ENOTSUP as a whole (gamdp_last_error names the task; the context stays usable).  The
 * launches count toward gamdp_ctx_kernel_time; gamdp_ctx_launch_info, gamdp_ctx_score_info and gamdp_ctx_carry_info keep describing
 * their own calls.  It makes no promise of speed. */
int gamdp_carry_ops_batch(gamdp_ctx* ctx, const gamdp_seqset* set_a, const gamdp_seqset* set_b,
                          const gamdp_task* tasks, size_t n, gamdp_result* out, uint32_t* ops_fp);
/* What the last gamdp_carry_ops_batch call on this context launched, in launch order: one launch ("k_carry_f<5>") per instantiation
 * its bands take; the fields as for gamdp_ctx_score_info. */
int gamdp_ctx_carry_ops_info(const gamdp_ctx* ctx, gamdp_score_launch_info* out, size_t cap, size_t* n);

/* The live width of one find_alignment call, on plain numbers (the arguments of gamdp_task_preflight; host only, no context): 0
 * for a call the pre-checks settle, otherwise the largest number of cells with 0 <= begin_a + i + j - band < alen in any one row
 * i < x_size, 0 <= j <= 2 band.  In closed form, with A0 = begin_a - band and last = alen - 1 - A0: row i holds
 *     n(i) = min(2 band, last - i) + min(0, A0 + i) + 1
 * such cells (none when that is negative), which rises while i < min(-A0, last - 2 band), is level up to the larger of the two and
 * falls behind it; so the result is max(0, n(i*)) with i* = min(-A0, last - 2 band) clamped to [0, x_size - 1].  It never exceeds
 * min(2 band + 1, alen).
 * What it is for: a cell outside a holds 0 and no traceback enters it, so a fill needs the live cells only, and a sweep by
 * anti-diagonals (cell (i, j) at step 2 i + j, sources one and two steps back) holds at most one cell per row and at most this many
 * rows in a step: three steps of this many entries are the whole state of a carry fill (gamdp_carry_batch) at any band, whatever
 * the rows and however far the band reaches beyond a -- against x_size * (2 band + 1) * 4 bytes of band matrix in gamdp_align_batch.
 * tests/_carrywmodel.py is that schedule in Python, its ring sized by this function and every read checked. */
uint64_t gamdp_task_live_columns(uint64_t alen, uint64_t blen, uint32_t band, uint64_t begin_a, uint64_t end_a, uint64_t begin_b,
                                 uint64_t end_b, int force_start, int force_end);

/* An upper bound on gamdp_result.length of one find_alignment call, on plain numbers (the arguments of gamdp_task_preflight; host
 * only, no context): 0 for a call the pre-checks settle, otherwise a multiple of 16 (the bound rounded up; at least 16).
 * The argument, against the traceback loop of banded_smith_waterman.cc:227-311.  Let X = x_size (:93-95, what the pre-checks size)
 * and y_size = 2 band + 1.  The loop starts at x = max_i <= X - 1, y = max_j <= 2 band, pos = begin_a + x + y - band, runs while
 * x >= 0, y >= 0 and pos >= 0, and every pass emits one op and takes one of three steps, in the pos == 0 branch (:229-262) as in
 * the general one (:263-308):
 *   diag   (MATCH / MISMATCH, :237-250, :272-285)   x--          : x and pos fall by one;
 *   GAP_A  (:256-261, :286-291, :297-302)           x--, y++     : x falls by one, pos stays;
 *   GAP_B  (:251-255, :292-296, :303-307)           y--          : pos falls by one, x stays.
 * GAP_A is taken only where y < y_size - 1 (:251 tests y == y_size - 1 first; :286 and :297 require it), so y never exceeds 2 band.
 * Row 0 is no exception: a diag or GAP_A step from x == 0 leaves x == -1 and ends the loop, a GAP_B step there lowers y and pos as
 * anywhere; nor is pos == 0, where a diag or GAP_B step leaves pos == -1 and ends the loop and GAP_A lowers x.  Hence
 *   #diag + #GAP_A <= max_i + 1 <= X                 (x falls from max_i to -1 at most),
 *   #GAP_B         <= max_j + #GAP_A <= 2 band + X   (y rises only by GAP_A and ends the loop below 0),
 *   #diag + #GAP_B <= pos(end cell) + 1 <= min(|a|, begin_a + X + band)   (a result with status OK read a.at(pos) at its end cell),
 * and length = #diag + #GAP_A + #GAP_B <= X + min(X + 2 band, |a|, begin_a + X + band) <= 2 X + 2 band.  X <= 500 000 and
 * band <= GAMDP_MAX_BAND keep the bound below 2^22 + 2^21. */
uint64_t gamdp_task_ops_cap(uint64_t alen, uint64_t blen, uint32_t band, uint64_t begin_a, uint64_t end_a, uint64_t begin_b,
                            uint64_t end_b, int force_start, int force_end);

/* gamdp_align_batch with an edit string requested for every task, and the fingerprint of each in place of the strings: out[i] is
 * exactly what gamdp_align_batch writes for such a call, ops_fp[i] is gamdp_ops_fingerprint of the bytes it would deliver through
 * gamdp_ops, and 0 for every status other than GAMDP_ST_OK, the cases gamdp_task_preflight settles included.  The strings never
 * leave the device: the library lays them out itself (task i in a room of gamdp_task_ops_cap bytes at a 16-byte aligned offset),
 * runs the ordinary alignment launches, leaves the strings where the walks wrote them -- in traceback order, which is the order the
 * fingerprint's polynomial wants -- and folds them with k_ops_fp (segments of 4 096 bytes, one wavefront each) on the context's
 * stream; n x 4 bytes come back.  A batch goes in chunks of consecutive tasks whose rooms sum to at most the context's ops budget
 * (gamdp_ctx_set_ops_chunk_bytes: 1 GiB by default; a task whose own room exceeds it goes alone).
 * Which walk this checks: a task that wants an edit string takes the one-task walk of its kernel (every step one at a time, the
 * multi-task kernels included), so the fingerprints check that walk and everything it reads -- strips, re-created directions, side
 * captures -- against gamdp_carry_ops_batch, op by op, at any batch size (tools/score_crosscheck.py --ops --device-fp); the result
 * fields of the multi-task walks are what gamdp_carry_batch checks.  It is also the fingerprint for bands above
 * GAMDP_MAX_TUNED_BAND: there is no band refusal, anything gamdp_align_batch takes is taken.
 * GAMDP_EINVAL for NULL ctx / sets / out / ops_fp and NULL tasks with n > 0, before anything is touched; n == 0 succeeds; ids out of
 * range and reverse complements of a packed-only set are refused as gamdp_align_batch refuses them.  Should a task come back with
 * length above its room (the bound of gamdp_task_ops_cap violated), the call fails with GAMDP_EHIP and gamdp_last_error names the
 * task: never a fingerprint of a truncated string.  gamdp_ctx_launch_info describes the alignment launches of the last chunk;
 * every launch counts toward gamdp_ctx_kernel_time. */
int gamdp_align_batch_fp(gamdp_ctx* ctx, const gamdp_seqset* set_a, const gamdp_seqset* set_b, const gamdp_task* tasks, size_t n,
                         gamdp_result* out, uint32_t* ops_fp);
/* The ops budget of gamdp_align_batch_fp and gamdp_ops_fingerprint_batch: the bytes of edit strings one chunk may hold on the device;
 * 0 = the default (1 GiB).  A property of the context like gamdp_ctx_set_arena_bytes.  GAMDP_EINVAL for a NULL ctx. */
int gamdp_ctx_set_ops_chunk_bytes(gamdp_ctx* ctx, uint64_t bytes);

/* fp[i] = gamdp_ops_fingerprint(ops + off[i], len[i]) for n strings in forward order in a host buffer, at any offsets, of any
 * bytes: staged into the aligned layout on upload, in chunks of the same budget, and folded by k_ops_fp's forward instantiation.
 * The kernel on its own.  GAMDP_EINVAL for NULL ctx / fp, NULL off / len with n > 0, NULL ops with a string that is not empty, and a
 * string of 2^32 - 4 096 bytes or more; n == 0 succeeds. */
int gamdp_ops_fingerprint_batch(gamdp_ctx* ctx, const uint8_t* ops, const uint64_t* off, const uint64_t* len, size_t n, uint32_t* fp);

/* What the last gamdp_align_batch_fp or gamdp_ops_fingerprint_batch call on this context did with k_ops_fp, summed over its chunks. */
typedef struct gamdp_ops_fp_info {
    char kernel[24];          /* "k_ops_fp<false>" (traceback order: gamdp_align_batch_fp) or "k_ops_fp<true>" (forward order) */
    uint32_t segment_bytes;   /* bytes of a string one wavefront folds */
    uint32_t lane_bytes;      /* ... and one lane of it */
    uint64_t tasks;           /* strings handed to the kernel (empty strings and calls the pre-checks settle are not) */
    uint64_t segments;        /* wavefront units */
    uint64_t bytes;           /* bytes of strings folded */
    uint32_t chunks;          /* chunks the batch went in */
    uint32_t pad_;
    double kernel_ms;         /* HIP events around the k_ops_fp launches */
} gamdp_ops_fp_info;          /* 72 bytes */
int gamdp_ctx_ops_fp_info(const gamdp_ctx* ctx, gamdp_ops_fp_info* out);   /* GAMDP_EINVAL for NULL ctx / out */

/* bit 0: this library is the diagnostics build (-DGAMDP_DIAG; honours the GAMDP_DIAG_* switches that change kernel
 * paths or invalidate results).  The product build returns 0 and ignores those switches. */
unsigned gamdp_build_info(void);

/* ---- L1: batch of merge blocks ------------------------------------------------------------ */
/* band is DEFAULT_BAND_SIZE (150) in the reference.  audit (optional) receives, per merge block i,
 * up to audit_stride results of its DP calls in call order at audit[i*audit_stride ...]. */
int gamdp_align_merge_blocks(gamdp_ctx* ctx, const gamdp_seqset* master, const gamdp_seqset* slave,
                             const gamdp_mb_in* in, size_t n, uint32_t band, gamdp_mb_out* out,
                             gamdp_result* audit, uint32_t audit_stride);

/* What the last gamdp_align_merge_blocks call on this context did (timing of the driver itself). */
typedef struct gamdp_l1_stats {
    uint64_t merge_blocks, dp_calls, cells;
    uint32_t rounds;          /* most rounds any cohort needed (a round = one batch of pending find_alignment calls) */
    uint32_t cohorts;         /* host threads / streams the merge blocks were spread over on this device          */
    uint32_t launches;        /* kernel launches                                                                   */
    uint32_t pad_;
    double wall_ms;           /* inside the call                                                                   */
    double gpu_busy_ms;       /* union of the kernels' execution intervals (HIP events): time with >= 1 kernel running */
    double kernel_sum_ms;     /* sum of the kernels' durations (can exceed gpu_busy_ms: cohorts overlap)          */
    double host_pending_ms;   /* building pending calls incl. findHits, summed over cohort threads                 */
    double host_feed_ms;      /* feeding results back, summed over cohort threads                                  */
} gamdp_l1_stats;
int gamdp_ctx_l1_stats(const gamdp_ctx* ctx, gamdp_l1_stats* out);

/* Where gamdp_align_merge_blocks computes the seeds of its tail alignments: after the main chain each merge block makes up to two
 * more find_alignment calls (PctgBuilder.cc:1535-1569 left, :1573-1611 right), each seeded by ABlast(20).findHits
 * (lib/src/alignment/ablast.cc:41-76; the driver reads hitsList.empty(), .back() at PctgBuilder.cc:1544-1551 and .front() at
 * :1584-1591).  HOST: one query at a time on the host's 1 byte/base codes.  DEVICE: the queries of a round as one batch of the
 * gamdp_find_hits_batch kernels (summaries only: n_hits, first, last) on the cohort's stream, beside the chain launch; a query
 * whose scratch does not fit the cohort's share of the arena is answered on the host.  Results, n_dp, cells and the audit trail
 * do not depend on the mode.  A property of the context (gamdp_multi_align_merge_blocks honours what each gamdp_multi_ctx(m, i)
 * was set to); GAMDP_L1_DEVICE_HITS=1 in the environment (read once per process) makes DEVICE the mode of new contexts. */
#define GAMDP_L1_HITS_HOST   0   /* default */
#define GAMDP_L1_HITS_DEVICE 1
int gamdp_ctx_set_l1_hits(gamdp_ctx* ctx, int mode);      /* GAMDP_EINVAL for NULL / unknown mode */
/* The findHits calls (ablast.cc:41-76) of the last gamdp_align_merge_blocks on this context. */
typedef struct gamdp_l1_hits_stats {
    uint64_t tail_queries;    /* findHits calls the last gamdp_align_merge_blocks made = device + trivial + host_fallback + host */
    uint64_t device_queries;  /* answered by the hits kernels */
    uint64_t trivial_queries; /* device mode, no work after the clamps of ablast.cc:47-53 (no launch) */
    uint64_t host_fallback;   /* device mode, did not fit the arena share */
    uint64_t host_queries;    /* host mode */
    uint32_t hits_launches;   /* kernel launches of the hits batches (part of gamdp_l1_stats.launches) */
    uint32_t mode;            /* GAMDP_L1_HITS_* the call ran in */
    double hits_kernel_ms;    /* sum of those kernels' durations (part of gamdp_l1_stats.kernel_sum_ms) */
    double host_hits_ms;      /* inside the host findHits, summed over cohort threads */
} gamdp_l1_hits_stats;
int gamdp_ctx_l1_hits_stats(const gamdp_ctx* ctx, gamdp_l1_hits_stats* out);
/* The tail alignments the last gamdp_align_merge_blocks on this context issued, ordered by merge block, left before right: the
 * seed each was given.  gamdp_result holds what find_alignment returned, not the window it was called with; this is the one
 * number of that window that findHits decides (begin_a: hitsList.back() / sb - sa, PctgBuilder.cc:1544-1561, hitsList.front() /
 * 0, :1584-1604), so that a test can pin the seed itself.  *n = how many there are; the first cap are written (as
 * gamdp_ctx_launch_info). */
#define GAMDP_L1_SEED_HOST     0   /* host mode                           */
#define GAMDP_L1_SEED_DEVICE   1   /* the hits kernels                    */
#define GAMDP_L1_SEED_TRIVIAL  2   /* device mode, no work after the clamps */
#define GAMDP_L1_SEED_FALLBACK 3   /* device mode, host fallback          */
typedef struct gamdp_l1_tail_call {
    uint64_t begin_a;         /* of the find_alignment call                          */
    uint32_t merge_block;     /* index in the call's `in` array                      */
    uint8_t right;            /* 0: left tail (force_end), 1: right tail (force_start) */
    uint8_t source;           /* GAMDP_L1_SEED_*                                     */
    uint8_t pad_[2];
} gamdp_l1_tail_call;
int gamdp_ctx_l1_tail_calls(const gamdp_ctx* ctx, gamdp_l1_tail_call* out, size_t cap, size_t* n);

/* Which kernel runs the main chains of gamdp_align_merge_blocks on the device (alignBlocks, PctgBuilder.cc:1617-1708, and the
 * orientation retry of findBestAlignment, :1420-1509): one launch takes every merge block without an empty slave frame through its
 * whole chain, and the host replays its own state machine over the records the chains leave (a difference is GAMDP_EHIP, never a
 * wrong answer).
 * WALK: a workgroup of three wavefronts per merge block (one fills, two walk), the long chains with a twin workgroup for the other
 *   orientation, three scratch slots per merge block, sized for its longest slave frame, out of half of the arena
 *   (gamdp_ctx_set_arena_bytes): what does not fit at once goes in pieces, without twins, or -- a frame too long for the arena --
 *   through the round loop (one launch and one host round trip per link of every chain).  Which bands have such a kernel is the
 *   context's gamdp_ctx_set_l1_walk_bands property:
 *     GAMDP_L1_WALK_BAND_150 (the default): band 150 only, k_chain2 (the 5-column band-150 cell, N-aware by the window of each call);
 *       every other band takes the round loop.
 *     GAMDP_L1_WALK_ANY_BAND: band 150 takes k_chain2 unchanged; every other band up to GAMDP_MAX_TUNED_BAND takes k_chain2g<C>, the
 *       same workgroup around the generic cell with C = 2, 3, 5, 9, 17 columns per lane by band (what gamdp_align_batch runs at
 *       that band; C >= 9 fills without directions and re-creates them along the path).  Every call of such a chain runs the
 *       N-aware cell.  gamdp_l1_chain_stats then reports mode = WALK, kernel = "k_chain2g<C>", cols = C, and scratch_bytes, twins
 *       and launches as for k_chain2.  Wider bands keep the round loop.
 * CARRY: k_chain_c<C>, one wavefront per merge block on gamdp_carry_batch's cell: the last match a chain's next call starts from
 *   is in the end cell's summary when the fill ends, so there is no walk, no scratch slot (the arena does not matter), no twin, and
 *   any band up to GAMDP_MAX_TUNED_BAND runs its chains on the device (C = 2, 3, 5, 9, 17 columns per lane by band, as
 *   gamdp_carry_batch).  Wider bands keep the round loop.
 * In either mode merge blocks with an empty slave frame, the tail alignments and everything under GAMDP_L1_ROUNDS=1 take the round
 * loop.  Results, n_dp, cells and the audit trail do not depend on the mode; gamdp_l1_stats and gamdp_l1_hits_stats keep their
 * layout and meaning.  A property of the context (gamdp_multi_align_merge_blocks honours what each gamdp_multi_ctx(m, i) was set
 * to); GAMDP_L1_CHAIN_CARRY=1 in the environment (read once per process) makes CARRY the mode of new contexts,
 * GAMDP_L1_WALK_ANY_BAND=1 makes GAMDP_L1_WALK_ANY_BAND their walk-bands property.  CARRY mode ignores that property. */
#define GAMDP_L1_CHAIN_WALK  0   /* default: k_chain2 / k_chain2g<C> (scratch slots from the arena; bands: gamdp_ctx_set_l1_walk_bands) */
#define GAMDP_L1_CHAIN_CARRY 1   /* k_chain_c<C>: any band <= GAMDP_MAX_TUNED_BAND, no scratch */
int gamdp_ctx_set_l1_chain(gamdp_ctx* ctx, int mode);     /* GAMDP_EINVAL for NULL / unknown mode (mode checked first) */
#define GAMDP_L1_WALK_BAND_150 0   /* default: WALK has a chain kernel at band 150 only */
#define GAMDP_L1_WALK_ANY_BAND 1   /* WALK: k_chain2 at 150, k_chain2g<C> at every other band <= GAMDP_MAX_TUNED_BAND */
int gamdp_ctx_set_l1_walk_bands(gamdp_ctx* ctx, int which);   /* GAMDP_EINVAL for NULL / unknown value (value checked first) */
/* The chain launch of the last gamdp_align_merge_blocks on this context, in either mode. */
typedef struct gamdp_l1_chain_stats {
    uint64_t chains;          /* merge blocks whose main chain a chain launch ran and whose records the replay used */
    uint64_t chain_calls;     /* records replayed: the find_alignment calls of those chains */
    uint64_t round_loop_mbs;  /* merge blocks whose main phase took the round loop instead */
    uint64_t scratch_bytes;   /* scratch slots of the chain launch; 0 in CARRY mode and when there was no launch */
    uint32_t mode;            /* GAMDP_L1_CHAIN_* the call ran in */
    uint32_t launches;        /* kernel launches of the chains (WALK: one per piece); part of gamdp_l1_stats.launches as ONE */
    uint32_t twins;           /* twin workgroups (WALK only) */
    uint32_t cols;            /* band columns per lane of the instantiation (k_chain2: 5); 0 when there was no launch */
    char kernel[24];          /* e.g. "k_chain_c<5>", "k_chain2<true>" or "k_chain2g<9>"; "" when there was no launch */
    double chain_ms;          /* HIP events around the launches */
} gamdp_l1_chain_stats;       /* 80 bytes */
int gamdp_ctx_l1_chain_stats(const gamdp_ctx* ctx, gamdp_l1_chain_stats* out);   /* GAMDP_EINVAL for NULL ctx / out */

/* ---- several GPUs of one node ------------------------------------------------------------- */
/* Replaces gam-merge's worker pool (lib/src/pctg/ThreadedBuildPctg.cc:143-197: N pthreads, mutex-guarded cursor
 * :50-74) for this path: one host thread + context + resident copy of the sequences per device; the task / merge-block
 * list is partitioned statically (longest-processing-time first by predicted cell updates), every device fills the
 * result slots of its own items, and nothing is exchanged between devices (no collective).  Results are identical to
 * the single-context calls whatever the number of devices.  A device may be listed more than once (one context each). */
typedef struct gamdp_multi gamdp_multi;
typedef struct gamdp_multi_seqset gamdp_multi_seqset;
int gamdp_multi_create(const int* devices, int n, gamdp_multi** out);
void gamdp_multi_destroy(gamdp_multi* m);
int gamdp_multi_size(const gamdp_multi* m);
gamdp_ctx* gamdp_multi_ctx(gamdp_multi* m, int i);            /* borrowed: context of device slot i */
const char* gamdp_multi_last_error(const gamdp_multi* m);
/* the same sequences resident on every device (RefSequence is shared read-only by the reference's workers) */
int gamdp_multi_seqset_create(gamdp_multi* m, const uint8_t* const* seqs, const uint64_t* lens, uint32_t n, int is_ascii,
                              gamdp_multi_seqset** out);
int gamdp_multi_seqset_create_from_fasta(gamdp_multi* m, const gamdp_fasta* f, gamdp_multi_seqset** out);
void gamdp_multi_seqset_destroy(gamdp_multi_seqset* s);
gamdp_seqset* gamdp_multi_seqset_on(gamdp_multi_seqset* s, int i);   /* borrowed: the copy on device slot i */
/* gamdp_align_batch / gamdp_align_merge_blocks over all devices of m; out / audit are indexed like the input */
int gamdp_multi_align_batch(gamdp_multi* m, const gamdp_multi_seqset* set_a, const gamdp_multi_seqset* set_b,
                            const gamdp_task* tasks, size_t n, gamdp_result* out);
int gamdp_multi_align_merge_blocks(gamdp_multi* m, const gamdp_multi_seqset* master, const gamdp_multi_seqset* slave,
                                   const gamdp_mb_in* in, size_t n, uint32_t band, gamdp_mb_out* out, gamdp_result* audit,
                                   uint32_t audit_stride);
/* The partitioner on its own (host only): items in order of decreasing weight, ties by index, go to the least-loaded
 * part, ties to the lower part.  Deterministic: the ranks of a one-process-per-GPU run (bench.py under
 * torch.distributed.run) each derive the same assignment from it without communicating. */
int gamdp_partition_lpt(const uint64_t* weights, size_t n, int parts, uint32_t* part_of);

/* ---- host-side helpers on the path -------------------------------------------------------- */
/* ABlast::findHits on code arrays; returns the number of hits (first cap written) or <0. */
int64_t gamdp_find_hits(const uint8_t* a, uint64_t alen, uint64_t a_start, uint64_t a_end,
                        const uint8_t* b, uint64_t blen, uint64_t b_start, uint64_t b_end,
                        uint64_t word, uint32_t* hits, uint64_t cap);

/* ABlast(word).findHits(a_view, a_start, a_end, b_view, b_start, b_end) (lib/src/alignment/ablast.cc:41-76,
 * lib/include/alignment/ablast.hpp:53-99) for a batch of queries on the GPU, over the packed sequences of the sets (a packed-only
 * synthetic set included).  Views as in gamdp_task: *_rc = reverse complement, then *_off = suffix; coordinates are relative to
 * the view and clamped exactly as ablast.cc:47-53 (word == 0: no hits).  The hits of a query are the positions a_start + i of the
 * diagonals i that hold the most votes, ascending, as uint32_t (the reference's list<uint32_t>). */
typedef struct gamdp_hits_task {
    uint32_t a_id, b_id;
    uint64_t a_off, b_off;
    uint8_t a_rc, b_rc, pad_[2];
    uint32_t word;                  /* ABlast word size (the reference's default: 20) */
    uint64_t a_start, a_end, b_start, b_end;
} gamdp_hits_task;

typedef struct gamdp_hits_result {
    uint64_t n_hits;                /* hitsList.size()                                                        */
    uint64_t votes;                 /* max_score of ablast.cc:44-73 (0 when there is no hit)                  */
    uint32_t first, last;           /* hitsList.front() / .back() (what PctgBuilder.cc:1544, 1584 consume); 0 without hits */
    uint8_t status;                 /* GAMDP_ST_OK, or GAMDP_ST_INVALID: *_off beyond the end of the sequence */
    uint8_t pad_[7];
} gamdp_hits_result;

/* The hits of query i go to hits_buf[hits_off[i] .. + min(n_hits, hits_cap[i])); hits_buf == NULL: the summaries only.
 * GAMDP_EINVAL for NULL ctx / sets / out and for ids out of range or reverse complements of a packed-only set;
 * GAMDP_ENOMEM when one query alone does not fit the scratch arena (gamdp_ctx_set_arena_bytes; gamdp_last_error names it) --
 * a batch whose queries fit one by one goes in pieces.  The launches count toward gamdp_ctx_kernel_time; gamdp_ctx_launch_info
 * keeps describing the last gamdp_align_batch. */
int gamdp_find_hits_batch(gamdp_ctx* ctx, const gamdp_seqset* set_a, const gamdp_seqset* set_b, const gamdp_hits_task* tasks,
                          size_t n, gamdp_hits_result* out, uint32_t* hits_buf, const uint64_t* hits_off,
                          const uint64_t* hits_cap);
void gamdp_encode(const char* chars, uint64_t n, uint8_t* codes);
void gamdp_decode(const uint8_t* codes, uint64_t n, char* chars);
void gamdp_revcomp(uint8_t* codes, uint64_t n);

/* ---- post-alignment stage: merge lists -> paired contigs -> .gam.fasta / .pctgs ----- */
/* Host only (no GPU, no ctx).  Replaces, for one assembly graph, BuildPctgFunctions.cc:86-92 after the align loop:
 * splitMergeBlocksByAlign / ByDirection / sortMergeBlocksByDirection / splitMergeBlocksByInclusions
 * (PctgBuilder.cc:667-723, 543-665, 507-541, 291-505) and buildPctgs (PctgBuilder.cc:172-288); and, for the whole
 * run, the id assignment, the single-contig pctgs and the two writers of src/Merge.cc:380-385, 437-465. */

/* a host-side assembly from memory (what gamdp_fasta_open builds from a file): names[i] may be NULL */
int gamdp_fasta_create(const char* const* names, const uint8_t* const* seqs, const uint64_t* lens, uint32_t n,
                       int is_ascii, gamdp_fasta** out);

/* MergeBlock as the post-alignment stage sees it (MergeDescriptor.hpp:40-69 without vertex/valid). */
typedef struct gamdp_mblock {
    int32_t m_id, m_start, m_end;
    int32_t s_id, s_start, s_end;
    uint8_t align_rev, align_ok;
    uint8_t m_ltail, m_rtail, s_ltail, s_rtail;
    uint8_t ext_slave_next, ext_slave_prev;   /* carried and updated like the reference; nothing reads them */
    uint8_t m_rev, s_rev;                     /* written by the direction stage */
    uint8_t pad_[2];
} gamdp_mblock;

/* CtgInPctgInfo (lib/include/pctg/CtgInPctgInfo.hpp:44-69): one row of a paired contig's merge list */
typedef struct gamdp_pctg_row {
    int64_t start, end;        /* first / last base taken from the contig, on the strand it is used on */
    int32_t ctg_id;
    uint8_t reversed, is_master;
    uint8_t pad_[2];
} gamdp_pctg_row;

#define GAMDP_STAGE_ALIGN      1u   /* splitMergeBlocksByAlign      */
#define GAMDP_STAGE_DIRECTION  2u   /* splitMergeBlocksByDirection  */
#define GAMDP_STAGE_SORT       4u   /* sortMergeBlocksByDirection   */
#define GAMDP_STAGE_INCLUSIONS 8u   /* splitMergeBlocksByInclusions */
#define GAMDP_STAGE_ALL        15u

/* The list surgery alone (stages applied in the reference's order, selected by the mask).  Lists are passed flat:
 * blocks holds list 0, then list 1, ...; list_sizes their lengths.  Returns GAMDP_ENOMEM (with *n_out_lists set)
 * when the output does not fit. */
int gamdp_merge_lists_prepare(const gamdp_fasta* master, const gamdp_fasta* slave, const gamdp_mblock* blocks,
                              const uint32_t* list_sizes, uint32_t n_lists, unsigned stages, gamdp_mblock* out_blocks,
                              uint64_t cap_blocks, uint32_t* out_sizes, uint32_t cap_lists, uint32_t* n_out_lists);

/* appendBlocksRegionToPctg asks the BAMs which assembly to trust when the two copies of a block region differ in
 * length by more than 3 % (computeZScore, PctgBuilder.cc:147-168).  The host supplies that decision:
 * return 0 = take the master's copy, 1 = the slave's, < 0 = error (the graph is dropped).  Coordinates are the ones
 * the reference passes (strand coordinates of the merge block). */
typedef int (*gamdp_region_vote_fn)(void* user, int32_t m_id, int32_t m_start, int32_t m_end, int32_t s_id,
                                    int32_t s_start, int32_t s_end);
/* the evidence count of PctgBuilder.cc:155-168 on two z-score vectors: 0 = master, 1 = slave */
int gamdp_zscore_vote(const double* master_z, const double* slave_z, size_t n);

typedef struct gamdp_pctgs gamdp_pctgs;   /* std::list<PairedContig> of one gam-merge run */
int gamdp_pctgs_create(const gamdp_fasta* master, const gamdp_fasta* slave, gamdp_pctgs** out);
void gamdp_pctgs_destroy(gamdp_pctgs* p);
const char* gamdp_pctgs_last_error(const gamdp_pctgs* p);
/* One graph's merge lists (after gamdp_align_merge_blocks filled align_ok/align_rev/m_start..s_end): list surgery +
 * buildPctgs; the resulting paired contigs are appended in list order.  On error nothing of this graph is kept
 * (the reference drops a graph whose worker throws, ThreadedBuildPctg.cc:322-329). */
int gamdp_pctgs_add_graph(gamdp_pctgs* p, const gamdp_mblock* blocks, const uint32_t* list_sizes, uint32_t n_lists,
                          gamdp_region_vote_fn vote, void* user);
/* ids 0.. in insertion order, then one paired contig per master contig no paired contig uses (ascending id, empty
 * contigs skipped): src/Merge.cc:380-385, 437-452, BuildPctgFunctions.cc:111-129 */
int gamdp_pctgs_finish(gamdp_pctgs* p);
uint32_t gamdp_pctgs_count(const gamdp_pctgs* p);
uint32_t gamdp_pctgs_merged_count(const gamdp_pctgs* p);   /* how many came from merge lists (old_pctg_id) */
const uint8_t* gamdp_pctgs_codes(const gamdp_pctgs* p, uint32_t i, uint64_t* len);
/* merge list of paired contig i: returns its length, writes the first cap rows */
uint32_t gamdp_pctgs_rows(const gamdp_pctgs* p, uint32_t i, gamdp_pctg_row* out, uint32_t cap);
/* which contigs any paired contig touches (getMasterCtgIdSet / getSlaveIds; Merge.cc:418-424 needs the slave side
 * for .notmerged.fasta); either pointer may be NULL */
int gamdp_pctgs_contig_use(const gamdp_pctgs* p, uint8_t* master_used, uint8_t* slave_used);
/* ".gam.fasta": >PairedContig_<id>, 60 bases per line (io_contig.code.hpp:246-262 + the endl of Merge.cc:458) */
int gamdp_pctgs_write_fasta(const gamdp_pctgs* p, const char* path);
/* ".pctgs" (PairedContig.cc:305-349) */
int gamdp_pctgs_write_descriptors(const gamdp_pctgs* p, const char* path);

/* ---- gam-merge's side outputs: slave contigs no block lies on, slave contigs no paired contig uses -------------
 * (src/Merge.cc:273-277, 294-297, 335-373, 412-431; host only).  All flag arrays are one byte per contig. */
/* getNoBlocksContigs (Block.cc:810-862): master_nbc[i] / slave_nbc[i] = 1 iff no block lies on contig i.  A block with a
 * contig id outside [0, n_master) / [0, n_slave) is where the reference prints an error and exits: GAMDP_EINVAL. */
int gamdp_no_blocks_contigs(const gamdp_block_rec* blocks, uint64_t n_blocks, uint32_t n_master, uint32_t n_slave,
                            uint8_t* master_nbc, uint8_t* slave_nbc);
/* getNoBlocksAfterFilterContigs (Block.cc:865-925): contigs that had blocks before the coverage filter
 * (master_nbc / slave_nbc = the arrays of the call above on the unfiltered list) and have none in `filtered`. */
int gamdp_no_blocks_after_filter(const gamdp_block_rec* filtered, uint64_t n_blocks, uint32_t n_master, uint32_t n_slave,
                                 const uint8_t* master_nbc, const uint8_t* slave_nbc, uint8_t* master_af, uint8_t* slave_af);
/* Merge.cc:416-429: not_merged[i] = 1 iff slave contig i is in no paired contig and in neither no-blocks set */
int gamdp_pctgs_not_merged(const gamdp_pctgs* p, const uint8_t* slave_nbc_bf, const uint8_t* slave_nbc_af, uint8_t* not_merged);
/* the contigs with select[i] != 0, each as `os << contig << std::endl` (io_contig.code.hpp:246-262: ">" name, 60 bases
 * per line): ".noblocks.BF.fasta", ".noblocks.AF.fasta", ".notmerged.fasta" (Merge.cc:336-373, 414-431) */
int gamdp_fasta_write_selected(const gamdp_fasta* f, const uint8_t* select, const char* path);

/* Synthetic pair k of the benchmark workload (BASELINE.json config 5): master = len uniform ACGT
 * codes, slave = master with 3 % substitutions, 1 % insertions, 1 % deletions (splitmix64 keyed by
 * k).  slave must hold len + len/8 + 64 codes; returns the slave length. */
uint64_t gamdp_synth_pair(uint64_t k, uint64_t len, uint8_t* master, uint8_t* slave);
/* Benchmark helper: a sequence set holding synthetic pairs [first_pair, first_pair+n_pairs) (sequence 2k =
 * master, 2k+1 = slave of pair first_pair+k), generated on host threads straight into the packed planes.
 * Such a set keeps no host copy of the bases: reverse-complement views and merge blocks are refused on it. */
int gamdp_seqset_create_synth(gamdp_ctx* ctx, uint64_t first_pair, uint32_t n_pairs, uint64_t len,
                              gamdp_seqset** out);
/* the same for pairs first_pair + k * stride_pairs, k < n_pairs: the share of one GPU when the fixed pair list of the
 * benchmark is dealt round-robin over several (what gamdp_partition_lpt yields for equal weights) */
int gamdp_seqset_create_synth_strided(gamdp_ctx* ctx, uint64_t first_pair, uint64_t stride_pairs, uint32_t n_pairs,
                                      uint64_t len, gamdp_seqset** out);

#ifdef __cplusplus
}
#endif
#endif /* GAMDP_H */
