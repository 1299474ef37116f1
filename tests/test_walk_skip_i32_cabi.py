"""CPU checks of the int32 direction-free kernels' walk-skip property (gamdp_ctx_set_walk_skip_i32 / gamdp_ctx_walk_skip_i32_stats of
include/gamdp.h): the library exports both, the ctypes struct matches the header's layout as a C compiler sees it, the two older
structs keep theirs, the argument checks need no GPU, and the stand-in library of integration/ exports them too."""
import ctypes
import os
import subprocess

from gam_ngs_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gamdp_ctx_set_walk_skip_i32", "gamdp_ctx_walk_skip_i32_stats")

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "gamdp.h"
#define F(m) printf("f.%s %zu\n", #m, offsetof(gamdp_walk_skip_i32_stats, m))
int main(void)
{
    printf("size %zu\n", sizeof(gamdp_walk_skip_i32_stats));
    F(tests); F(groups_tested); F(groups_skipped); F(rows_skipped); F(strips); F(mode); F(launches);
    printf("modes %d %d\n", GAMDP_WALK_STRIPS, GAMDP_WALK_SKIP_DIAG);
    printf("eight %zu\n", sizeof(gamdp_walk_skip_stats));
    printf("pair %zu\n", sizeof(gamdp_walk_skip_pair_stats));
    return 0;
}
"""


def test_both_functions_are_exported():
    l = lib.load_library()
    for name in NAMES:
        assert name in lib.SYMBOLS
        assert hasattr(l, name)


def test_stats_struct_matches_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    seen = {l.split()[0]: l.split()[1:] for l in subprocess.check_output([str(exe)]).decode().splitlines()}
    cls = lib.WalkSkipI32Stats
    assert int(seen["size"][0]) == ctypes.sizeof(cls) == 48
    assert [f for f, _ in cls._fields_] == ["tests", "groups_tested", "groups_skipped", "rows_skipped", "strips", "mode", "launches"]
    for field, _ in cls._fields_:
        assert int(seen["f.%s" % field][0]) == getattr(cls, field).offset, field
    assert [int(x) for x in seen["modes"]] == [lib.WALK_STRIPS, lib.WALK_SKIP_DIAG] == [0, 1]
    assert int(seen["eight"][0]) == ctypes.sizeof(lib.WalkSkipStats) == 48          # the two older structs keep their layouts
    assert int(seen["pair"][0]) == ctypes.sizeof(lib.WalkSkipPairStats) == 56


def test_null_and_unknown_mode_are_einval():
    l = lib.load_library()
    st = lib.WalkSkipI32Stats()
    assert l.gamdp_ctx_set_walk_skip_i32(None, lib.WALK_STRIPS) == lib.EINVAL
    assert l.gamdp_ctx_set_walk_skip_i32(None, lib.WALK_SKIP_DIAG) == lib.EINVAL
    assert l.gamdp_ctx_walk_skip_i32_stats(None, ctypes.byref(st)) == lib.EINVAL
    # the mode is checked before the context is touched: any non-NULL handle will do for an unknown mode
    fake = ctypes.create_string_buffer(8)
    for mode in (-1, 2, 7):
        assert l.gamdp_ctx_set_walk_skip_i32(ctypes.cast(fake, ctypes.c_void_p), mode) == lib.EINVAL
    assert l.gamdp_ctx_walk_skip_i32_stats(ctypes.cast(fake, ctypes.c_void_p), None) == lib.EINVAL


def test_the_stand_in_library_exports_them(tmp_path):
    so = tmp_path / "stub.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-o", str(so),
                           os.path.join(ROOT, "integration", "gamdp_stub.c")])
    stub = ctypes.CDLL(str(so))
    st = lib.WalkSkipI32Stats()
    assert stub.gamdp_ctx_set_walk_skip_i32(None, lib.WALK_SKIP_DIAG) != 0
    assert stub.gamdp_ctx_walk_skip_i32_stats(None, ctypes.byref(st)) != 0
