"""CPU checks of the merge-block driver's chain mode (gamdp_ctx_set_l1_chain / gamdp_ctx_l1_chain_stats of include/gamdp.h): the
library exports both, the ctypes struct matches the header's layout as a C compiler sees it, and the argument checks need no GPU."""
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
    printf("gamdp_l1_chain_stats %zu\n", sizeof(gamdp_l1_chain_stats));
    F(gamdp_l1_chain_stats, chains); F(gamdp_l1_chain_stats, chain_calls); F(gamdp_l1_chain_stats, round_loop_mbs);
    F(gamdp_l1_chain_stats, scratch_bytes); F(gamdp_l1_chain_stats, mode); F(gamdp_l1_chain_stats, launches);
    F(gamdp_l1_chain_stats, twins); F(gamdp_l1_chain_stats, cols); F(gamdp_l1_chain_stats, kernel); F(gamdp_l1_chain_stats, chain_ms);
    printf("kernel_chars %zu\n", sizeof(((gamdp_l1_chain_stats*)0)->kernel));
    printf("modes %d %d\n", GAMDP_L1_CHAIN_WALK, GAMDP_L1_CHAIN_CARRY);
    return 0;
}
"""


def test_both_functions_are_exported():
    l = lib.load_library()
    for name in ("gamdp_ctx_set_l1_chain", "gamdp_ctx_l1_chain_stats"):
        assert name in lib.SYMBOLS
        assert hasattr(l, name)


def test_stats_struct_matches_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = [line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines()]
    seen = {l[0]: l[1:] for l in lines}
    cls = lib.L1ChainStats
    assert int(seen["gamdp_l1_chain_stats"][0]) == ctypes.sizeof(cls) == 80
    for field, _ in cls._fields_:
        assert int(seen["gamdp_l1_chain_stats.%s" % field][0]) == getattr(cls, field).offset, field
    assert int(seen["kernel_chars"][0]) == cls.kernel.size == 24
    assert [int(x) for x in seen["modes"]] == [lib.L1_CHAIN_WALK, lib.L1_CHAIN_CARRY] == [0, 1]


def test_null_and_unknown_mode_are_einval():
    l = lib.load_library()
    st = lib.L1ChainStats()
    assert l.gamdp_ctx_set_l1_chain(None, lib.L1_CHAIN_WALK) == lib.EINVAL
    assert l.gamdp_ctx_set_l1_chain(None, lib.L1_CHAIN_CARRY) == lib.EINVAL
    assert l.gamdp_ctx_l1_chain_stats(None, ctypes.byref(st)) == lib.EINVAL
    # the mode is checked before the context is touched: any non-NULL handle will do for an unknown mode
    fake = ctypes.create_string_buffer(8)
    for mode in (-1, 2, 7):
        assert l.gamdp_ctx_set_l1_chain(ctypes.cast(fake, ctypes.c_void_p), mode) == lib.EINVAL
    assert l.gamdp_ctx_l1_chain_stats(ctypes.cast(fake, ctypes.c_void_p), None) == lib.EINVAL
