"""Host-side mirror of the reference's operator interface for the alignment path, on top of the C ABI.

Names and argument meaning follow the reference so the parity tests read like its call sites:

  BandedSmithWaterman(band).find_alignment(a, begin_a, end_a, b, begin_b, end_b, force_start, force_end)
      lib/include/alignment/banded_smith_waterman.hpp:66-71
  MyAlignment + first_match_pos / last_match_pos      lib/include/alignment/my_alignment.hpp:65-131
  ABlast(word).findHits(a, a_start, a_end, b, b_start, b_end)   lib/include/alignment/ablast.hpp:116-117
  PctgBuilder.alignMergeBlock(graph, mb)              lib/include/pctg/PctgBuilder.hpp:162
  MergeBlock                                          lib/include/pctg/MergeDescriptor.hpp:40-69

Everything that computes goes through libgamdp.so on the GPU; nothing here falls back to the CPU.
"""
import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

from . import lib as L

GAP_A, GAP_B, MATCH, MISMATCH = 0, 1, 2, 3
OPS_CHARS = "ABMX"
DEFAULT_BAND_SIZE = 150


def _check(ctx, rc, what):
    if rc != 0:
        msg = L.load_library().gamdp_last_error(ctx.handle) if ctx is not None and ctx.handle else b""
        raise L.GamdpError("%s failed with code %d: %s" % (what, rc, (msg or b"").decode()))


class Context:
    """One GPU + one HIP stream (gamdp_ctx)."""

    def __init__(self, device: int = 0):
        self.lib = L.load_library()
        h = C.c_void_p()
        rc = self.lib.gamdp_ctx_create(device, C.byref(h))
        if rc != 0:
            raise L.GamdpError("gamdp_ctx_create(device=%d) failed with code %d (no gfx950 GPU?); "
                               "libgamdp has no CPU fallback" % (device, rc))
        self.handle = h
        self.device = device

    def set_arena_bytes(self, nbytes: int):
        _check(self, self.lib.gamdp_ctx_set_arena_bytes(self.handle, nbytes), "gamdp_ctx_set_arena_bytes")

    def last_error(self):
        return (self.lib.gamdp_last_error(self.handle) or b"").decode()

    def set_l1_hits(self, mode: int):
        """Where alignMergeBlocks computes the findHits seeds of its tail alignments: L.L1_HITS_HOST (the default) or
        L.L1_HITS_DEVICE (gamdp_ctx_set_l1_hits).  The results do not depend on it."""
        _check(self, self.lib.gamdp_ctx_set_l1_hits(self.handle, mode), "gamdp_ctx_set_l1_hits")

    def l1_hits_stats(self):
        """The findHits calls of the last alignMergeBlocks on this context, as a dict (gamdp_ctx_l1_hits_stats)."""
        st = L.L1HitsStats()
        _check(self, self.lib.gamdp_ctx_l1_hits_stats(self.handle, C.byref(st)), "gamdp_ctx_l1_hits_stats")
        return st.as_dict()

    def set_l1_chain(self, mode: int):
        """Which kernel runs the main chains of alignMergeBlocks on the device: L.L1_CHAIN_WALK (the default: k_chain2, band 150,
        scratch slots from the arena) or L.L1_CHAIN_CARRY (k_chain_c: any band up to 543, no scratch; gamdp_ctx_set_l1_chain).
        The results do not depend on it."""
        _check(self, self.lib.gamdp_ctx_set_l1_chain(self.handle, mode), "gamdp_ctx_set_l1_chain")

    def set_l1_walk_bands(self, which: int):
        """Which bands the default chain mode (L.L1_CHAIN_WALK) has a chain kernel for: L.L1_WALK_BAND_150 (the default: k_chain2 at
        band 150, the round loop elsewhere) or L.L1_WALK_ANY_BAND (k_chain2 at 150, k_chain2g<C> at every other band up to 543;
        gamdp_ctx_set_l1_walk_bands).  Results do not depend on it; L.L1_CHAIN_CARRY ignores it."""
        _check(self, self.lib.gamdp_ctx_set_l1_walk_bands(self.handle, which), "gamdp_ctx_set_l1_walk_bands")

    def l1_chain_stats(self):
        """The chain launch of the last alignMergeBlocks on this context, as a dict (gamdp_ctx_l1_chain_stats)."""
        st = L.L1ChainStats()
        _check(self, self.lib.gamdp_ctx_l1_chain_stats(self.handle, C.byref(st)), "gamdp_ctx_l1_chain_stats")
        return st.as_dict()

    def _set_walk_mode(self, name, mode):
        _check(self, getattr(self.lib, name)(self.handle, mode), name)

    def _walk_stats(self, name, struct):
        st = struct()
        _check(self, getattr(self.lib, name)(self.handle, C.byref(st)), name)
        return st.as_dict()

    def set_walk_skip(self, mode: int):
        """How the walks of the eight-task band-150 kernel cross rows without directions: L.WALK_STRIPS (the default: a strip call per
        stretch of the path) or L.WALK_SKIP_DIAG (groups of 64 rows that provably hold diagonal steps only are jumped over;
        gamdp_ctx_set_walk_skip).  The results do not depend on it."""
        self._set_walk_mode("gamdp_ctx_set_walk_skip", mode)

    def walk_skip_stats(self):
        """What the eight-task launches of the last gamdp_align_batch on this context counted, as a dict (gamdp_ctx_walk_skip_stats)."""
        return self._walk_stats("gamdp_ctx_walk_skip_stats", L.WalkSkipStats)

    def set_walk_skip_pair(self, mode: int):
        """The same choice for the walks of the two-task band-512 kernel, a property of its own: L.WALK_STRIPS (the default) or
        L.WALK_SKIP_DIAG (gamdp_ctx_set_walk_skip_pair).  The results do not depend on it."""
        self._set_walk_mode("gamdp_ctx_set_walk_skip_pair", mode)

    def walk_skip_pair_stats(self):
        """What the two-task launches of the last gamdp_align_batch on this context counted, as a dict (gamdp_ctx_walk_skip_pair_stats)."""
        return self._walk_stats("gamdp_ctx_walk_skip_pair_stats", L.WalkSkipPairStats)

    def set_walk_skip_i32(self, mode: int):
        """The same choice for the walks of the int32 direction-free kernels (k_align<17,4>, k_align_q<19,15>, k_align<9,-1,true>,
        k_align<17,-1,true>), a third property: L.WALK_STRIPS (the default) or L.WALK_SKIP_DIAG (gamdp_ctx_set_walk_skip_i32).
        The results do not depend on it."""
        self._set_walk_mode("gamdp_ctx_set_walk_skip_i32", mode)

    def walk_skip_i32_stats(self):
        """What the launches of those kernels in the last gamdp_align_batch on this context counted, as a dict (gamdp_ctx_walk_skip_i32_stats)."""
        return self._walk_stats("gamdp_ctx_walk_skip_i32_stats", L.WalkSkipI32Stats)

    def set_walk_skip_backoff(self, mode: int):
        """Whether walks in L.WALK_SKIP_DIAG mode of any of the three properties above back off from the test after failures, a
        fourth property: L.WALK_BACKOFF_OFF (the default: every candidate point is tested) or L.WALK_BACKOFF_ON (after `fails` tests
        in a row that skipped nothing, the next gamdp_walk_skip_backoff_hold(fails) points pass without a test;
        gamdp_ctx_set_walk_skip_backoff).  The results do not depend on it."""
        self._set_walk_mode("gamdp_ctx_set_walk_skip_backoff", mode)

    def walk_skip_backoff_stats(self):
        """The candidate points the walks of the last gamdp_align_batch on this context passed without a test, per kernel family, as a
        dict (gamdp_ctx_walk_skip_backoff_stats)."""
        return self._walk_stats("gamdp_ctx_walk_skip_backoff_stats", L.WalkSkipBackoffStats)

    def set_ops_walk(self, mode: int):
        """How the walks of calls that want an edit string write it: L.OPS_WALK_STEPS (the default: one op per iteration) or
        L.OPS_WALK_RUNS (a whole run of diagonal steps per iteration, its ops written by the lanes that compared its bases;
        gamdp_ctx_set_ops_walk).  Results and bytes do not depend on it; k_align_w ignores it."""
        self._set_walk_mode("gamdp_ctx_set_ops_walk", mode)

    def ops_walk_stats(self):
        """What the walks of the last gamdp_align_batch / gamdp_align_batch_fp on this context that wrote their string a run at a time
        counted, as a dict (gamdp_ctx_ops_walk_stats)."""
        return self._walk_stats("gamdp_ctx_ops_walk_stats", L.OpsWalkStats)

    def l1_tail_calls(self):
        """The tail alignments of the last alignMergeBlocks on this context and the seed each was given, as
        (merge_block, right, begin_a, source) tuples ordered by merge block, left before right (gamdp_ctx_l1_tail_calls)."""
        n = C.c_size_t()
        _check(self, self.lib.gamdp_ctx_l1_tail_calls(self.handle, None, 0, C.byref(n)), "gamdp_ctx_l1_tail_calls")
        arr = (L.L1TailCall * max(1, n.value))()
        _check(self, self.lib.gamdp_ctx_l1_tail_calls(self.handle, arr, n.value, C.byref(n)), "gamdp_ctx_l1_tail_calls")
        return [(arr[i].merge_block, bool(arr[i].right), arr[i].begin_a, arr[i].source) for i in range(n.value)]

    def kernel_time(self, reset=False):
        ms, n = C.c_double(), C.c_uint64()
        self.lib.gamdp_ctx_kernel_time(self.handle, C.byref(ms), C.byref(n), int(reset))
        return ms.value, n.value

    def _launches(self, getter_name, struct):
        """One of the context's launch logs, as dicts: its length first, then that many records."""
        getter = getattr(self.lib, getter_name)
        n = C.c_size_t()
        getter(self.handle, None, 0, C.byref(n))
        arr = (struct * max(1, n.value))()
        getter(self.handle, arr, n.value, C.byref(n))
        return [arr[i].as_dict() for i in range(n.value)]

    def launch_info(self):
        """The launches of the last gamdp_align_batch call on this context, as dicts (gamdp_ctx_launch_info)."""
        return self._launches("gamdp_ctx_launch_info", L.LaunchInfo)

    def score_info(self):
        """The launches of the last gamdp_score_batch call on this context, as dicts (gamdp_ctx_score_info)."""
        return self._launches("gamdp_ctx_score_info", L.ScoreLaunchInfo)

    def carry_info(self):
        """The launches of the last gamdp_carry_batch call on this context, as dicts (gamdp_ctx_carry_info)."""
        return self._launches("gamdp_ctx_carry_info", L.ScoreLaunchInfo)

    def carry_ops_info(self):
        """The launches of the last gamdp_carry_ops_batch call on this context, as dicts (gamdp_ctx_carry_ops_info)."""
        return self._launches("gamdp_ctx_carry_ops_info", L.ScoreLaunchInfo)

    def set_ops_chunk_bytes(self, nbytes: int):
        """The bytes of edit strings one chunk of find_alignments_with_ops_fingerprints / ops_fingerprint_many may hold on the device
        (gamdp_ctx_set_ops_chunk_bytes); 0 = the default, 1 GiB.  The results do not depend on it."""
        _check(self, self.lib.gamdp_ctx_set_ops_chunk_bytes(self.handle, nbytes), "gamdp_ctx_set_ops_chunk_bytes")

    def ops_fp_info(self):
        """What the last find_alignments_with_ops_fingerprints / ops_fingerprint_many on this context did with k_ops_fp, as a dict
        (gamdp_ctx_ops_fp_info)."""
        st = L.OpsFpInfo()
        _check(self, self.lib.gamdp_ctx_ops_fp_info(self.handle, C.byref(st)), "gamdp_ctx_ops_fp_info")
        return st.as_dict()

    def close(self):
        if getattr(self, "handle", None):
            self.lib.gamdp_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SequenceSet:
    """RefSequence equivalent: contigs packed (2 bit + N mask) and resident in HBM (gamdp_seqset)."""

    def __init__(self, ctx: Context, seqs: Sequence[bytes], ascii: bool = True):
        self.ctx = ctx
        n = len(seqs)
        self._keep = [bytes(s) for s in seqs]
        arr = (C.c_char_p * max(1, n))(*self._keep)
        lens = (C.c_uint64 * max(1, n))(*[len(s) for s in self._keep])
        h = C.c_void_p()
        rc = ctx.lib.gamdp_seqset_create(ctx.handle, arr, lens, n, int(ascii), C.byref(h))
        _check(ctx, rc, "gamdp_seqset_create")
        self.handle = h
        self.lengths = [len(s) for s in self._keep]

    @classmethod
    def from_fasta(cls, ctx: "Context", path: str):
        """loadSequences equivalent: every record of a FASTA file, in file order (names in .names)."""
        names, codes = load_fasta(path)
        self = cls(ctx, codes, ascii=False)
        self.names = names
        return self

    @classmethod
    def synthetic(cls, ctx: "Context", first_pair: int, n_pairs: int, length: int, stride: int = 1):
        """Pairs first_pair + k*stride, k < n_pairs, of the benchmark generator, built and packed inside the
        library (sequence 2k = master, 2k+1 = slave); no host copy of the bases is kept."""
        self = cls.__new__(cls)
        self.ctx = ctx
        self._keep = []
        h = C.c_void_p()
        _check(ctx, ctx.lib.gamdp_seqset_create_synth_strided(ctx.handle, first_pair, stride, n_pairs, length, C.byref(h)),
               "gamdp_seqset_create_synth_strided")
        self.handle = h
        self.lengths = [ctx.lib.gamdp_seqset_length(h, i) for i in range(2 * n_pairs)]
        return self

    def __len__(self):
        return len(self.lengths)

    def contig(self, idx, rc=False, off=0):
        return Contig(self, idx, rc, off)

    def close(self):
        if getattr(self, "handle", None) and self.ctx.handle:
            self.ctx.lib.gamdp_seqset_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiContext:
    """Several GPUs of one node behind one handle (gamdp_multi): the worker pool of ThreadedBuildPctg.cc:143-197.
    `devices` may name a device more than once (one context each)."""

    def __init__(self, devices: Sequence[int]):
        self.lib = L.load_library()
        arr = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        rc = self.lib.gamdp_multi_create(arr, len(devices), C.byref(h))
        if rc != 0:
            raise L.GamdpError("gamdp_multi_create(%r) failed with code %d; libgamdp has no CPU fallback" % (list(devices), rc))
        self.handle = h
        self.devices = list(devices)

    def last_error(self):
        return (self.lib.gamdp_multi_last_error(self.handle) or b"").decode()

    def set_l1_hits(self, mode: int):
        """Context.set_l1_hits on every context of the handle."""
        for i in range(len(self.devices)):
            if self.lib.gamdp_ctx_set_l1_hits(self.lib.gamdp_multi_ctx(self.handle, i), mode) != 0:
                raise L.GamdpError("gamdp_ctx_set_l1_hits(%r) failed on context %d" % (mode, i))

    def set_l1_chain(self, mode: int):
        """Context.set_l1_chain on every context of the handle."""
        for i in range(len(self.devices)):
            if self.lib.gamdp_ctx_set_l1_chain(self.lib.gamdp_multi_ctx(self.handle, i), mode) != 0:
                raise L.GamdpError("gamdp_ctx_set_l1_chain(%r) failed on context %d" % (mode, i))

    def set_l1_walk_bands(self, which: int):
        """Context.set_l1_walk_bands on every context of the handle."""
        for i in range(len(self.devices)):
            if self.lib.gamdp_ctx_set_l1_walk_bands(self.lib.gamdp_multi_ctx(self.handle, i), which) != 0:
                raise L.GamdpError("gamdp_ctx_set_l1_walk_bands(%r) failed on context %d" % (which, i))

    def _set_walk_mode(self, name, mode, which):
        for i in (range(len(self.devices)) if which is None else (which,)):
            if getattr(self.lib, name)(self.lib.gamdp_multi_ctx(self.handle, i), mode) != 0:
                raise L.GamdpError("%s(%r) failed on context %d" % (name, mode, i))

    def _walk_stats(self, name, struct):
        out = []
        for i in range(len(self.devices)):
            st = struct()
            if getattr(self.lib, name)(self.lib.gamdp_multi_ctx(self.handle, i), C.byref(st)) != 0:
                raise L.GamdpError("%s failed on context %d" % (name, i))
            out.append(st.as_dict())
        return out

    def set_walk_skip(self, mode: int, which=None):
        """Context.set_walk_skip on every context of the handle, or on context `which` alone."""
        self._set_walk_mode("gamdp_ctx_set_walk_skip", mode, which)

    def walk_skip_stats(self):
        """Context.walk_skip_stats of every context of the handle (a list of dicts)."""
        return self._walk_stats("gamdp_ctx_walk_skip_stats", L.WalkSkipStats)

    def set_walk_skip_pair(self, mode: int, which=None):
        """Context.set_walk_skip_pair on every context of the handle, or on context `which` alone."""
        self._set_walk_mode("gamdp_ctx_set_walk_skip_pair", mode, which)

    def walk_skip_pair_stats(self):
        """Context.walk_skip_pair_stats of every context of the handle (a list of dicts)."""
        return self._walk_stats("gamdp_ctx_walk_skip_pair_stats", L.WalkSkipPairStats)

    def set_walk_skip_i32(self, mode: int, which=None):
        """Context.set_walk_skip_i32 on every context of the handle, or on context `which` alone."""
        self._set_walk_mode("gamdp_ctx_set_walk_skip_i32", mode, which)

    def walk_skip_i32_stats(self):
        """Context.walk_skip_i32_stats of every context of the handle (a list of dicts)."""
        return self._walk_stats("gamdp_ctx_walk_skip_i32_stats", L.WalkSkipI32Stats)

    def set_walk_skip_backoff(self, mode: int, which=None):
        """Context.set_walk_skip_backoff on every context of the handle, or on context `which` alone."""
        self._set_walk_mode("gamdp_ctx_set_walk_skip_backoff", mode, which)

    def walk_skip_backoff_stats(self):
        """Context.walk_skip_backoff_stats of every context of the handle (a list of dicts)."""
        return self._walk_stats("gamdp_ctx_walk_skip_backoff_stats", L.WalkSkipBackoffStats)

    def set_ops_walk(self, mode: int, which=None):
        """Context.set_ops_walk on every context of the handle, or on context `which` alone."""
        self._set_walk_mode("gamdp_ctx_set_ops_walk", mode, which)

    def ops_walk_stats(self):
        """Context.ops_walk_stats of every context of the handle (a list of dicts)."""
        return self._walk_stats("gamdp_ctx_ops_walk_stats", L.OpsWalkStats)

    def l1_chain_stats(self):
        """Context.l1_chain_stats of every context of the handle (a list of dicts)."""
        out = []
        for i in range(len(self.devices)):
            st = L.L1ChainStats()
            if self.lib.gamdp_ctx_l1_chain_stats(self.lib.gamdp_multi_ctx(self.handle, i), C.byref(st)) != 0:
                raise L.GamdpError("gamdp_ctx_l1_chain_stats failed on context %d" % i)
            out.append(st.as_dict())
        return out

    def l1_hits_stats(self):
        """Context.l1_hits_stats of every context of the handle (a list of dicts)."""
        out = []
        for i in range(len(self.devices)):
            st = L.L1HitsStats()
            if self.lib.gamdp_ctx_l1_hits_stats(self.lib.gamdp_multi_ctx(self.handle, i), C.byref(st)) != 0:
                raise L.GamdpError("gamdp_ctx_l1_hits_stats failed on context %d" % i)
            out.append(st.as_dict())
        return out

    def close(self):
        if getattr(self, "handle", None):
            self.lib.gamdp_multi_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiSequenceSet:
    """The same contigs resident on every device of a MultiContext (gamdp_multi_seqset)."""

    def __init__(self, mctx: MultiContext, seqs: Sequence[bytes], ascii: bool = True):
        self.ctx = mctx
        n = len(seqs)
        self._keep = [bytes(s) for s in seqs]
        arr = (C.c_char_p * max(1, n))(*self._keep)
        lens = (C.c_uint64 * max(1, n))(*[len(s) for s in self._keep])
        h = C.c_void_p()
        rc = mctx.lib.gamdp_multi_seqset_create(mctx.handle, arr, lens, n, int(ascii), C.byref(h))
        if rc != 0:
            raise L.GamdpError("gamdp_multi_seqset_create failed with code %d: %s" % (rc, mctx.last_error()))
        self.handle = h
        self.lengths = [len(s) for s in self._keep]

    def __len__(self):
        return len(self.lengths)

    def contig(self, idx, rc=False, off=0):
        return Contig(self, idx, rc, off)

    def close(self):
        if getattr(self, "handle", None) and self.ctx.handle:
            self.ctx.lib.gamdp_multi_seqset_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def partition_lpt(weights: Sequence[int], parts: int) -> List[int]:
    """gamdp_partition_lpt: part of every item (deterministic longest-processing-time-first)."""
    n = len(weights)
    w = (C.c_uint64 * max(1, n))(*weights)
    out = (C.c_uint32 * max(1, n))()
    if L.load_library().gamdp_partition_lpt(w, n, parts, out) != 0:
        raise L.GamdpError("gamdp_partition_lpt failed")
    return list(out[:n])


def task_preflight(alen, blen, band, begin_a, end_a, begin_b, end_b, fs=False, fe=False):
    """(status, cells) the batch call settles on before launching anything (gamdp_task_preflight); status ST_OK means
    the call needs the DP."""
    m64 = (1 << 64) - 1
    cells = C.c_uint64()
    st = L.load_library().gamdp_task_preflight(alen, blen, band, begin_a & m64, end_a & m64, begin_b & m64, end_b & m64,
                                               int(fs), int(fe), C.byref(cells))
    return st, cells.value


def task_ops_cap(alen, blen, band, begin_a, end_a, begin_b, end_b, fs=False, fe=False):
    """An upper bound on the length of the call's edit string, a multiple of 16, or 0 where task_preflight settles the call
    (gamdp_task_ops_cap)."""
    m64 = (1 << 64) - 1
    return int(L.load_library().gamdp_task_ops_cap(alen, blen, band, begin_a & m64, end_a & m64, begin_b & m64, end_b & m64,
                                                    int(fs), int(fe)))


def task_live_columns(alen, blen, band, begin_a, end_a, begin_b, end_b, fs=False, fe=False):
    """The largest number of cells inside a (0 <= begin_a - band + i + j < alen) in one row of the call's band matrix, or 0 where
    task_preflight settles the call (gamdp_task_live_columns): the entries per step a fill over the live cells alone needs."""
    m64 = (1 << 64) - 1
    return int(L.load_library().gamdp_task_live_columns(alen, blen, band, begin_a & m64, end_a & m64, begin_b & m64, end_b & m64,
                                                         int(fs), int(fe)))


@dataclass(frozen=True)
class Contig:
    """A view of one sequence of a SequenceSet: optionally reverse-complemented (the reference's
    in-place reverse_complement) and/or a suffix (its chop_begin copy)."""
    seqset: SequenceSet
    idx: int
    rc: bool = False
    off: int = 0

    def size(self):
        return self.seqset.lengths[self.idx] - self.off


@dataclass
class MyAlignment:
    _begin_a: int = 0
    _begin_b: int = 0
    _score: int = 0
    _homology: float = 0.0
    _length: int = 0
    n_match: int = 0
    first_match: tuple = (0, 0)
    first_found: bool = False
    last_match: tuple = (0, 0)
    last_found: bool = False
    status: int = L.ST_EMPTY
    cells: int = 0
    ops: Optional[str] = None  # edit string over "ABMX" (GAP_A, GAP_B, MATCH, MISMATCH) when requested

    def begin_a(self): return self._begin_a
    def begin_b(self): return self._begin_b
    def score(self): return self._score
    def homology(self): return self._homology
    def length(self): return self._length

    def sequence(self):
        if self.ops is None:
            raise L.GamdpError("edit string was not requested (want_ops=False)")
        return [OPS_CHARS.index(ch) for ch in self.ops]

    def key(self):
        return (self.status, self._begin_a, self._begin_b, self._score, self.n_match, self._length,
                self.first_match[0], self.first_match[1], int(self.first_found), self.last_match[0],
                self.last_match[1], int(self.last_found), self._homology)

    @staticmethod
    def from_result(r: "L.Result", ops=None):
        return MyAlignment(r.begin_a, r.begin_b, r.score, r.homology, r.length, r.n_match, (r.first_a, r.first_b),
                           bool(r.first_found), (r.last_a, r.last_b), bool(r.last_found), r.status, r.cells, ops)


def first_match_pos(aln: MyAlignment):
    """(found, (a, b)) -- my_alignment.cc:167-193"""
    return aln.first_found, aln.first_match


def last_match_pos(aln: MyAlignment):
    """(found, (a, b)) -- my_alignment.cc:228-262"""
    return aln.last_found, aln.last_match


def _no_ops(r):
    """the MyAlignment of a gamdp_result that comes without an edit string"""
    return MyAlignment.from_result(r, None)


class BandedSmithWaterman:
    """BandedSmithWaterman(band): find_alignment for one call, find_alignments for a batch."""

    def __init__(self, ctx: Context, band: int = DEFAULT_BAND_SIZE):
        self.ctx = ctx
        self.band = band

    def find_alignment(self, a: Contig, begin_a, end_a, b: Contig, begin_b, end_b, force_start=False, force_end=False,
                       want_ops=False) -> MyAlignment:
        return self.find_alignments([(a, begin_a, end_a, b, begin_b, end_b, force_start, force_end)], want_ops)[0]

    def _tasks(self, calls, bands):
        """The gamdp_task array of a batch of calls and the two sequence sets they refer to."""
        n = len(calls)
        sa, sb = calls[0][0].seqset, calls[0][3].seqset
        tasks = (L.Task * n)()
        m64 = (1 << 64) - 1
        for i, cl in enumerate(calls):
            a, begin_a, end_a, b, begin_b, end_b = cl[:6]
            fs = bool(cl[6]) if len(cl) > 6 else False
            fe = bool(cl[7]) if len(cl) > 7 else False
            if a.seqset is not sa or b.seqset is not sb:
                raise L.GamdpError("all a / all b contigs of one batch must share a SequenceSet")
            t = tasks[i]
            t.a_id, t.b_id, t.a_off, t.b_off = a.idx, b.idx, a.off, b.off
            t.a_rc, t.b_rc, t.force_start, t.force_end = int(a.rc), int(b.rc), int(fs), int(fe)
            t.band = self.band if bands is None else bands[i]
            t.begin_a, t.end_a, t.begin_b, t.end_b = begin_a & m64, end_a & m64, begin_b & m64, end_b & m64
        return tasks, sa, sb

    def _fill_only(self, calls, bands, symbol, struct, with_fp, convert, method):
        """What find_scores, find_results and the two *_with_ops_fingerprints share: one call of `symbol` over the batch into an array
        of `struct` (and, with_fp, a fingerprint per call beside it) -> [convert(result)], or that and the fingerprints.  method: the
        public method's name, for its error message."""
        n = len(calls)
        if n == 0:
            return ([], []) if with_fp else []
        if isinstance(self.ctx, MultiContext):
            raise L.GamdpError("%s is a single-context call" % method)
        tasks, sa, sb = self._tasks(calls, bands)
        out = (struct * n)()
        extra = [(C.c_uint32 * n)()] if with_fp else []
        _check(self.ctx, getattr(self.ctx.lib, symbol)(self.ctx.handle, sa.handle, sb.handle, tasks, n, out, *extra), symbol)
        res = [convert(r) for r in out]
        return (res, list(extra[0])) if with_fp else res

    def find_scores(self, calls, bands=None):
        """Score and end cell of every call without the traceback (gamdp_score_batch: a second, int32-only kernel that uses no
        scratch arena): a list of (score, end_a, end_b, status, cells) for the calls find_alignments takes.  score, status and
        cells equal those of find_alignments; (end_a, end_b) is the cell the alignment ends in."""
        return self._fill_only(calls, bands, "gamdp_score_batch", L.ScoreResult, with_fp=False, method="find_scores",
                               convert=lambda r: (r.score, r.end_a, r.end_b, r.status, r.cells))

    def find_results(self, calls, bands=None) -> List[MyAlignment]:
        """Every call's whole result from a fill alone (gamdp_carry_batch: a third, int32-only kernel in which every cell carries the
        summary of the traceback that would start in it; no scratch arena, no walk): a list of MyAlignment without edit strings
        (ops None), field by field what find_alignments returns for the same calls."""
        return self._fill_only(calls, bands, "gamdp_carry_batch", L.Result, with_fp=False, convert=_no_ops, method="find_results")

    def find_results_with_ops_fingerprints(self, calls, bands=None):
        """find_results with the fingerprint of every call's edit string (gamdp_carry_ops_batch: the carry kernel with the
        fingerprint as a sixth field of a cell's summary): (results, fingerprints).  fingerprints[i] equals
        ops_fingerprint(find_alignments(calls, want_ops=True)[i].ops) for a call whose status is OK and is 0 otherwise."""
        return self._fill_only(calls, bands, "gamdp_carry_ops_batch", L.Result, with_fp=True, convert=_no_ops,
                               method="find_results_with_ops_fingerprints")

    def find_alignments_with_ops_fingerprints(self, calls, bands=None):
        """find_alignments(calls, want_ops=True) with the fingerprint of every edit string in place of the strings
        (gamdp_align_batch_fp: the strings stay on the device, k_ops_fp folds them there): (results, fingerprints), the results
        without edit strings (ops None).  fingerprints[i] equals ops_fingerprint(find_alignments(calls, want_ops=True)[i].ops) for a
        call whose status is OK and is 0 otherwise.  Any band find_alignments takes."""
        return self._fill_only(calls, bands, "gamdp_align_batch_fp", L.Result, with_fp=True, convert=_no_ops,
                               method="find_alignments_with_ops_fingerprints")

    def find_alignments(self, calls, want_ops=False, bands=None) -> List[MyAlignment]:
        """calls: list of (a, begin_a, end_a, b, begin_b, end_b[, force_start[, force_end]]); all a's
        must come from one SequenceSet and all b's from one SequenceSet."""
        n = len(calls)
        if n == 0:
            return []
        tasks, sa, sb = self._tasks(calls, bands)
        out = (L.Result * n)()
        ops_struct = None
        # want_ops: one flag for the batch, or one per call (a capacity of 0 = no edit string for that call)
        per_call = list(want_ops) if isinstance(want_ops, (list, tuple)) else [bool(want_ops)] * n
        want_ops = any(per_call)
        if want_ops:
            caps = []
            for i, cl in enumerate(calls):
                band = tasks[i].band
                caps.append(cl[0].size() + cl[3].size() + 2 * band + 64 if per_call[i] else 0)
            offs = [0] * n
            tot = 0
            for i in range(n):
                offs[i] = tot
                tot += caps[i]
            buf = C.create_string_buffer(max(1, tot))
            offs_c = (C.c_uint64 * n)(*offs)
            caps_c = (C.c_uint64 * n)(*caps)
            ops_struct = L.Ops(C.cast(buf, C.c_void_p), offs_c, caps_c)
        if isinstance(self.ctx, MultiContext):
            if want_ops:
                raise L.GamdpError("edit strings are a single-context (test) feature")
            rc = self.ctx.lib.gamdp_multi_align_batch(self.ctx.handle, sa.handle, sb.handle, tasks, n, out)
            if rc != 0:
                raise L.GamdpError("gamdp_multi_align_batch failed with code %d: %s" % (rc, self.ctx.last_error()))
        else:
            rc = self.ctx.lib.gamdp_align_batch(self.ctx.handle, sa.handle, sb.handle, tasks, n, out,
                                                C.byref(ops_struct) if ops_struct else None)
            _check(self.ctx, rc, "gamdp_align_batch")
        res = []
        for i in range(n):
            ops = None
            if want_ops and per_call[i]:
                ops = ""
                if out[i].status == L.ST_OK:
                    raw = buf.raw[offs[i]:offs[i] + out[i].length]
                    ops = "".join(OPS_CHARS[c] for c in raw)
            res.append(MyAlignment.from_result(out[i], ops))
        return res


class ABlast:
    """ABlast(word_size).findHits: on code arrays (host function of libgamdp), or find_hits_many for a batch of calls
    over the views of uploaded sequence sets (gamdp_find_hits_batch, on the GPU)."""

    def __init__(self, word_size: int = 20):
        self.word_size = word_size
        self.lib = L.load_library()

    def findHits(self, a: bytes, a_start, a_end, b: bytes, b_start, b_end):
        cap = len(a) + 1
        buf = (C.c_uint32 * cap)()
        m64 = (1 << 64) - 1
        n = self.lib.gamdp_find_hits(a, len(a), a_start & m64, a_end & m64, b, len(b), b_start & m64, b_end & m64,
                                     self.word_size, buf, cap)
        if n < 0:
            raise L.GamdpError("gamdp_find_hits failed")
        return list(buf[:n])

    def find_hits_many(self, ctx: Context, calls, want_hits=True, caps=None, words=None):
        """calls: list of (a: Contig, a_start, a_end, b: Contig, b_start, b_end); all a's from one SequenceSet, all b's from
        one SequenceSet.  Returns one hit list per call (what findHits returns for those views), or, with want_hits=False,
        (n_hits, first, last, votes) tuples.  caps (one per call) bounds how many hits of each call are returned (the
        default: all of them); words (one per call) replaces this ABlast's word size call by call."""
        n = len(calls)
        if n == 0:
            return []
        sa, sb = calls[0][0].seqset, calls[0][3].seqset
        tasks = (L.HitsTask * n)()
        m64 = (1 << 64) - 1
        for i, (a, a_start, a_end, b, b_start, b_end) in enumerate(calls):
            if a.seqset is not sa or b.seqset is not sb:
                raise L.GamdpError("all a / all b contigs of one batch must share a SequenceSet")
            t = tasks[i]
            t.a_id, t.b_id, t.a_off, t.b_off, t.a_rc, t.b_rc = a.idx, b.idx, a.off, b.off, int(a.rc), int(b.rc)
            t.word = self.word_size if words is None else words[i]
            t.a_start, t.a_end, t.b_start, t.b_end = a_start & m64, a_end & m64, b_start & m64, b_end & m64

        def call(tasks, n, caps):
            out = (L.HitsResult * n)()
            buf = offs = capc = None
            offs_l = []
            if caps is not None:
                tot = 0
                for c in caps:
                    offs_l.append(tot)
                    tot += c
                buf = (C.c_uint32 * max(1, tot))()
                offs = (C.c_uint64 * n)(*offs_l)
                capc = (C.c_uint64 * n)(*caps)
            _check(ctx, ctx.lib.gamdp_find_hits_batch(ctx.handle, sa.handle, sb.handle, tasks, n, out, buf, offs, capc),
                   "gamdp_find_hits_batch")
            hits = None if caps is None else [list(buf[offs_l[i]:offs_l[i] + min(out[i].n_hits, caps[i])]) for i in range(n)]
            return out, hits

        if not want_hits:
            return [(r.n_hits, r.first, r.last, r.votes) for r in call(tasks, n, None)[0]]
        if caps is not None:
            return call(tasks, n, list(caps))[1]
        # all hits: room for a few per call, then the calls with longer lists once more with room for all of theirs
        first = 64
        out, hits = call(tasks, n, [first] * n)
        again = [i for i in range(n) if out[i].n_hits > first]
        if again:
            sub = (L.HitsTask * len(again))(*[tasks[i] for i in again])
            _, more = call(sub, len(again), [out[i].n_hits for i in again])
            for i, h in zip(again, more):
                hits[i] = h
        return hits


def load_fasta(path: str):
    """(names, code arrays) of a FASTA file through the library's loader (reference rules, no GPU needed)."""
    lib = L.load_library()
    h = C.c_void_p()
    rc = lib.gamdp_fasta_open(path.encode(), C.byref(h))
    if rc != 0:
        raise L.GamdpError("gamdp_fasta_open(%s) failed with code %d" % (path, rc))
    try:
        names, codes = [], []
        for i in range(lib.gamdp_fasta_count(h)):
            names.append(lib.gamdp_fasta_name(h, i).decode())
            n = C.c_uint64()
            p = lib.gamdp_fasta_codes(h, i, C.byref(n))
            codes.append(bytes(bytearray(p[:n.value])) if n.value else b"")
        return names, codes
    finally:
        lib.gamdp_fasta_close(h)


def ops_fingerprint(ops) -> int:
    """gamdp_ops_fingerprint of an edit string: a str over OPS_CHARS ("ABMX", as MyAlignment.ops), or bytes / a sequence of op codes
    (GAMDP_OP_*: GAP_A 0, GAP_B 1, MATCH 2, MISMATCH 3; any byte value is taken)."""
    if isinstance(ops, str):
        ops = bytes(OPS_CHARS.index(ch) for ch in ops)
    else:
        ops = bytes(ops)
    return int(L.load_library().gamdp_ops_fingerprint(ops, len(ops)))


def ops_fingerprint_many(ctx: Context, strings) -> List[int]:
    """gamdp_ops_fingerprint of every string (str over OPS_CHARS, bytes, or sequences of byte values, as ops_fingerprint takes them),
    computed on the GPU by k_ops_fp's forward instantiation (gamdp_ops_fingerprint_batch): the strings go up back to back."""
    raw = [bytes(OPS_CHARS.index(ch) for ch in s) if isinstance(s, str) else bytes(s) for s in strings]
    n = len(raw)
    if n == 0:
        return []
    offs, tot = [], 0
    for s in raw:
        offs.append(tot)
        tot += len(s)
    buf = b"".join(raw)
    fp = (C.c_uint32 * n)()
    _check(ctx, ctx.lib.gamdp_ops_fingerprint_batch(ctx.handle, buf, (C.c_uint64 * n)(*offs), (C.c_uint64 * n)(*[len(s) for s in raw]), n, fp),
           "gamdp_ops_fingerprint_batch")
    return list(fp)


def encode(s) -> bytes:
    if isinstance(s, str):
        s = s.encode()
    out = C.create_string_buffer(len(s) + 1)
    L.load_library().gamdp_encode(s, len(s), out)
    return out.raw[:len(s)]


def decode(codes: bytes) -> str:
    out = C.create_string_buffer(len(codes) + 1)
    L.load_library().gamdp_decode(codes, len(codes), out)
    return out.raw[:len(codes)].decode()


def reverse_complement(codes: bytes) -> bytes:
    buf = C.create_string_buffer(codes, max(1, len(codes)))
    L.load_library().gamdp_revcomp(buf, len(codes))
    return buf.raw[:len(codes)]


def synth_pair(k: int, length: int):
    """(master codes, slave codes) of synthetic pair k (gamdp_synth_pair)."""
    m = C.create_string_buffer(length)
    s = C.create_string_buffer(length + length // 8 + 64)
    sl = L.load_library().gamdp_synth_pair(k, length, m, s)
    return m.raw[:length], s.raw[:sl]


@dataclass
class Block:
    """The Block/Frame fields the driver reads."""
    m_begin: int
    m_end: int
    s_begin: int
    s_end: int
    m_strand: str = "+"
    s_strand: str = "+"
    n_reads: int = 1


@dataclass
class MergeBlock:
    """MergeDescriptor.hpp:40-69: inputs (ids, tails, block list) and the fields alignMergeBlock writes."""
    m_id: int
    s_id: int
    blocks: List[Block] = field(default_factory=list)
    m_ltail: bool = False
    m_rtail: bool = False
    s_ltail: bool = False
    s_rtail: bool = False
    # outputs
    align_ok: bool = False
    align_rev: bool = False
    m_start: int = 0
    m_end: int = 0
    s_start: int = 0
    s_end: int = 0
    status: int = L.ST_OK
    coords_set: bool = False
    n_dp: int = 0
    cells: int = 0
    audit: Optional[list] = None


class PctgBuilder:
    """alignMergeBlock for a whole list of merge blocks (the loop of BuildPctgFunctions.cc:82-84)."""

    def __init__(self, ctx: Context, masterRef: SequenceSet, slaveRef: SequenceSet, band: int = DEFAULT_BAND_SIZE):
        self.ctx, self.masterRef, self.slaveRef, self.band = ctx, masterRef, slaveRef, band

    def alignMergeBlock(self, mb: MergeBlock, audit=0):
        self.alignMergeBlocks([mb], audit)
        return mb

    def alignMergeBlocks(self, mbs: List[MergeBlock], audit=0):
        n = len(mbs)
        if n == 0:
            return mbs
        ins = (L.MbIn * n)()
        keep = []
        for i, mb in enumerate(mbs):
            nb = len(mb.blocks)
            arr = (L.BlockC * max(1, nb))()
            for k, b in enumerate(mb.blocks):
                arr[k].m_begin, arr[k].m_end, arr[k].s_begin, arr[k].s_end = b.m_begin, b.m_end, b.s_begin, b.s_end
                arr[k].m_strand, arr[k].s_strand, arr[k].n_reads = b.m_strand.encode(), b.s_strand.encode(), b.n_reads
            keep.append(arr)
            x = ins[i]
            x.m_id, x.s_id = mb.m_id, mb.s_id
            x.m_ltail, x.m_rtail, x.s_ltail, x.s_rtail = int(mb.m_ltail), int(mb.m_rtail), int(mb.s_ltail), int(mb.s_rtail)
            x.n_blocks = nb
            x.blocks = C.cast(arr, C.POINTER(L.BlockC))
        outs = (L.MbOut * n)()
        aud = (L.Result * (n * audit))() if audit else None
        if isinstance(self.ctx, MultiContext):
            rc = self.ctx.lib.gamdp_multi_align_merge_blocks(self.ctx.handle, self.masterRef.handle, self.slaveRef.handle,
                                                             ins, n, self.band, outs, aud, audit)
            if rc != 0:
                raise L.GamdpError("gamdp_multi_align_merge_blocks failed with code %d: %s" % (rc, self.ctx.last_error()))
        else:
            rc = self.ctx.lib.gamdp_align_merge_blocks(self.ctx.handle, self.masterRef.handle, self.slaveRef.handle, ins, n,
                                                       self.band, outs, aud, audit)
            _check(self.ctx, rc, "gamdp_align_merge_blocks")
        for i, mb in enumerate(mbs):
            o = outs[i]
            mb.align_ok, mb.status, mb.coords_set = bool(o.align_ok), o.status, bool(o.coords_set)
            mb.n_dp, mb.cells = o.n_dp, o.cells
            if o.coords_set:  # the reference leaves these untouched otherwise (PctgBuilder.cc:825-829)
                mb.align_rev = bool(o.align_rev)
                mb.m_start, mb.m_end, mb.s_start, mb.s_end = o.m_start, o.m_end, o.s_start, o.s_end
            if audit:
                mb.audit = [MyAlignment.from_result(aud[i * audit + k]) for k in range(min(audit, o.n_dp))]
        return mbs


def load_blocks(path: str, min_block_size: int = 1):
    """Block::loadBlocks (lib/src/assembly/Block.cc:669-690): the blocks of a .blocks file as dicts."""
    lib = L.load_library()
    h = C.c_void_p()
    if lib.gamdp_blocks_open(str(path).encode(), min_block_size, C.byref(h)):
        raise L.GamdpError("cannot read " + str(path))
    try:
        n = lib.gamdp_blocks_count(h)
        p = lib.gamdp_blocks_data(h)
        return [p[i].as_dict() for i in range(n)]
    finally:
        lib.gamdp_blocks_close(h)


def write_blocks(path: str, blocks):
    """Block::writeBlocks (Block.cc:737-747)."""
    lib = L.load_library()
    arr = (L.BlockRec * max(1, len(blocks)))()
    for r, b in zip(arr, blocks):
        for k in L.BlockRec.KEYS:
            v = b[k]
            setattr(r, k, v.encode("latin1") if isinstance(v, str) else v)
    if lib.gamdp_blocks_write(str(path).encode(), arr, len(blocks)):
        raise L.GamdpError("cannot write " + str(path))


def _block_array(blocks):
    arr = (L.BlockRec * max(1, len(blocks)))()
    for r, b in zip(arr, blocks):
        for k in L.BlockRec.KEYS:
            v = b[k]
            setattr(r, k, v.encode("latin1") if isinstance(v, str) else v)
    return arr


def no_blocks_contigs(blocks, n_master: int, n_slave: int):
    """getNoBlocksContigs (Block.cc:810-862): (master flags, slave flags), 1 = no block lies on the contig."""
    lib = L.load_library()
    m, s = (C.c_uint8 * max(1, n_master))(), (C.c_uint8 * max(1, n_slave))()
    rc = lib.gamdp_no_blocks_contigs(_block_array(blocks), len(blocks), n_master, n_slave, m, s)
    if rc:
        raise L.GamdpError("a block names a contig outside the assemblies (the reference exits here)")
    return list(m[:n_master]), list(s[:n_slave])


def no_blocks_after_filter(filtered, n_master: int, n_slave: int, master_nbc, slave_nbc):
    """getNoBlocksAfterFilterContigs (Block.cc:865-925): contigs that lost all their blocks in the coverage filter."""
    lib = L.load_library()
    m, s = (C.c_uint8 * max(1, n_master))(), (C.c_uint8 * max(1, n_slave))()
    mb, sb = (C.c_uint8 * max(1, n_master))(*master_nbc), (C.c_uint8 * max(1, n_slave))(*slave_nbc)
    rc = lib.gamdp_no_blocks_after_filter(_block_array(filtered), len(filtered), n_master, n_slave, mb, sb, m, s)
    if rc:
        raise L.GamdpError("a block names a contig outside the assemblies (the reference exits here)")
    return list(m[:n_master]), list(s[:n_slave])


def write_selected_fasta(assembly, select, path):
    """The contigs with select[i] != 0 as gam-merge writes .noblocks.BF/.AF.fasta and .notmerged.fasta
    (src/Merge.cc:336-373, 414-431): `stream << contig << std::endl`."""
    lib = L.load_library()
    sel = (C.c_uint8 * max(1, len(select)))(*[int(bool(x)) for x in select])
    if lib.gamdp_fasta_write_selected(assembly.handle, sel, str(path).encode()):
        raise L.GamdpError("cannot write " + str(path))

