"""CPU checks of gamdp_ctx_set_l1_walk_bands (include/gamdp.h): which bands the merge-block driver's default chain mode has a chain
kernel for.  The library exports it, the two constants are what a C compiler sees in the header, and the argument checks need no
GPU."""
import ctypes
import os
import subprocess

from gam_ngs_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROBE = r"""
#include <stdio.h>
#include "gamdp.h"
int main(void)
{
    int (*f)(gamdp_ctx*, int) = 0;
    (void)sizeof(f = gamdp_ctx_set_l1_walk_bands);   /* the prototype the header declares (not evaluated: nothing to link) */
    printf("walk_bands %d %d\n", GAMDP_L1_WALK_BAND_150, GAMDP_L1_WALK_ANY_BAND);
    return 0;
}
"""


def test_the_function_is_exported():
    l = lib.load_library()
    assert "gamdp_ctx_set_l1_walk_bands" in lib.SYMBOLS
    assert hasattr(l, "gamdp_ctx_set_l1_walk_bands")


def test_constants_match_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    seen = subprocess.check_output([str(exe)]).decode().split()
    assert seen[0] == "walk_bands"
    assert [int(x) for x in seen[1:]] == [lib.L1_WALK_BAND_150, lib.L1_WALK_ANY_BAND] == [0, 1]


def test_null_and_unknown_value_are_einval():
    l = lib.load_library()
    assert l.gamdp_ctx_set_l1_walk_bands(None, lib.L1_WALK_BAND_150) == lib.EINVAL
    assert l.gamdp_ctx_set_l1_walk_bands(None, lib.L1_WALK_ANY_BAND) == lib.EINVAL
    # the value is checked before the context is touched: any non-NULL handle will do for an unknown value
    fake = ctypes.create_string_buffer(8)
    for which in (-1, 2, 7):
        assert l.gamdp_ctx_set_l1_walk_bands(ctypes.cast(fake, ctypes.c_void_p), which) == lib.EINVAL
