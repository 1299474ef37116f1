"""CPU checks of the merge-block driver's findHits mode (gamdp_ctx_set_l1_hits / gamdp_ctx_l1_hits_stats of include/gamdp.h):
the library exports both, the ctypes struct matches the header's layout as a C compiler sees it, and the argument checks
need no GPU."""
import ctypes
import os
import subprocess

from gam_ngs_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "gamdp.h"
#define F(T, m) printf("%s.%s %zu\n", #T, #m, offsetof(T, m))
int main(void)
{
    printf("gamdp_l1_hits_stats %zu\n", sizeof(gamdp_l1_hits_stats));
    F(gamdp_l1_hits_stats, tail_queries); F(gamdp_l1_hits_stats, device_queries); F(gamdp_l1_hits_stats, trivial_queries);
    F(gamdp_l1_hits_stats, host_fallback); F(gamdp_l1_hits_stats, host_queries); F(gamdp_l1_hits_stats, hits_launches);
    F(gamdp_l1_hits_stats, mode); F(gamdp_l1_hits_stats, hits_kernel_ms); F(gamdp_l1_hits_stats, host_hits_ms);
    printf("modes %d %d\n", GAMDP_L1_HITS_HOST, GAMDP_L1_HITS_DEVICE);
    printf("gamdp_l1_tail_call %zu\n", sizeof(gamdp_l1_tail_call));
    F(gamdp_l1_tail_call, begin_a); F(gamdp_l1_tail_call, merge_block); F(gamdp_l1_tail_call, right); F(gamdp_l1_tail_call, source);
    return 0;
}
"""


def test_both_functions_are_exported():
    l = lib.load_library()
    for name in ("gamdp_ctx_set_l1_hits", "gamdp_ctx_l1_hits_stats", "gamdp_ctx_l1_tail_calls"):
        assert name in lib.SYMBOLS
        assert hasattr(l, name)


def test_stats_struct_matches_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = [line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines()]
    seen = {l[0]: l[1:] for l in lines}
    cls = lib.L1HitsStats
    assert int(seen["gamdp_l1_hits_stats"][0]) == ctypes.sizeof(cls) == 64
    for field, _ in cls._fields_:
        assert int(seen["gamdp_l1_hits_stats.%s" % field][0]) == getattr(cls, field).offset, field
    assert int(seen["gamdp_l1_tail_call"][0]) == ctypes.sizeof(lib.L1TailCall) == 16
    for field in ("begin_a", "merge_block", "right", "source"):
        assert int(seen["gamdp_l1_tail_call.%s" % field][0]) == getattr(lib.L1TailCall, field).offset, field
    assert [int(x) for x in seen["modes"]] == [lib.L1_HITS_HOST, lib.L1_HITS_DEVICE] == [0, 1]


def test_null_and_unknown_mode_are_einval():
    l = lib.load_library()
    st = lib.L1HitsStats()
    assert l.gamdp_ctx_set_l1_hits(None, lib.L1_HITS_HOST) == lib.EINVAL
    assert l.gamdp_ctx_set_l1_hits(None, lib.L1_HITS_DEVICE) == lib.EINVAL
    assert l.gamdp_ctx_l1_hits_stats(None, ctypes.byref(st)) == lib.EINVAL
    # the mode is checked before the context is touched: any non-NULL handle will do for an unknown mode
    fake = ctypes.create_string_buffer(8)
    for mode in (-1, 2, 7):
        assert l.gamdp_ctx_set_l1_hits(ctypes.cast(fake, ctypes.c_void_p), mode) == lib.EINVAL
    assert l.gamdp_ctx_l1_hits_stats(ctypes.cast(fake, ctypes.c_void_p), None) == lib.EINVAL
    assert l.gamdp_ctx_l1_tail_calls(None, None, 0, None) == lib.EINVAL
    assert l.gamdp_ctx_l1_tail_calls(ctypes.cast(fake, ctypes.c_void_p), None, 1, None) == lib.EINVAL


def test_the_seed_case_depends_on_its_seed():
    """tests/_l1hits.py seed_case(), which the GPU tests use to show that a dropped seed is noticed: on the CPU oracle the
    left tail call seeded by findHits and the one seeded as if there were no hits give different results"""
    import _l1hits as H
    import _oracle as O
    import gam_ngs_amd as gam
    sc = H.seed_case()
    m, s = O.encode(sc["master"]), O.encode(sc["slave"])
    (blk,) = sc["blocks"]
    sa, sb = blk[0], blk[2]
    hits = gam.ABlast(20).findHits(m, 0, sa - 1, s, 0, sb - 1)
    assert hits and abs(hits[-1] - (sa - sb)) > 150
    seeded, _ = O.oracle_align(m, s, 150, hits[-1], sa - 1, 0, sb - 1, False, True, want_ops=False)
    unseeded, _ = O.oracle_align(m, s, 150, sa - sb, sa - 1, 0, sb - 1, False, True, want_ops=False)
    assert seeded.key() != unseeded.key()
