"""CPU checks of the three walk-skip properties (gamdp_ctx_set_walk_skip, _pair, _i32 and their gamdp_ctx_walk_skip*_stats of
include/gamdp.h), one case per property: the library exports both functions, the ctypes struct matches the header's layout as a C
compiler sees it (and the other structs keep theirs), the argument checks need no GPU, and the stand-in library of integration/
exports them too."""
import ctypes
import os
import subprocess

import pytest

from gam_ngs_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = ["tests", "groups_tested", "groups_skipped", "rows_skipped", "strips", "mode"]
# property -> (setter, getter, C struct, ctypes struct, its size, its fields in order)
STRUCTS = {
    "eight": ("gamdp_ctx_set_walk_skip", "gamdp_ctx_walk_skip_stats", "gamdp_walk_skip_stats", lib.WalkSkipStats, 48, COMMON + ["pad_"]),
    "pair": ("gamdp_ctx_set_walk_skip_pair", "gamdp_ctx_walk_skip_pair_stats", "gamdp_walk_skip_pair_stats", lib.WalkSkipPairStats, 56,
             COMMON + ["launches_side_by_side", "launches_one_by_one", "pad_"]),
    "i32": ("gamdp_ctx_set_walk_skip_i32", "gamdp_ctx_walk_skip_i32_stats", "gamdp_walk_skip_i32_stats", lib.WalkSkipI32Stats, 48,
            COMMON + ["launches"]),
}
PROPS = pytest.mark.parametrize("prop", sorted(STRUCTS))

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "gamdp.h"
#define F(T, m) printf("%%s.%%s %%zu\n", #T, #m, offsetof(T, m))
int main(void)
{
%s
    printf("modes %%d %%d\n", GAMDP_WALK_STRIPS, GAMDP_WALK_SKIP_DIAG);
    printf("launch_info %%zu\n", sizeof(gamdp_launch_info));
    return 0;
}
"""


def probe_source():
    lines = []
    for _, _, cname, _, _, fields in STRUCTS.values():
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        lines += ["    F(%s, %s);" % (cname, f) for f in fields]
    return PROBE % "\n".join(lines)


@PROPS
def test_both_functions_are_exported(prop):
    l = lib.load_library()
    for name in STRUCTS[prop][:2]:
        assert name in lib.SYMBOLS
        assert hasattr(l, name)


@PROPS
def test_stats_struct_matches_header(prop, tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(probe_source())
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    seen = {l.split()[0]: l.split()[1:] for l in subprocess.check_output([str(exe)]).decode().splitlines()}
    _, _, cname, cls, size, fields = STRUCTS[prop]
    assert int(seen[cname][0]) == ctypes.sizeof(cls) == size
    assert [f for f, _ in cls._fields_] == fields
    for field, _ in cls._fields_:
        assert int(seen["%s.%s" % (cname, field)][0]) == getattr(cls, field).offset, field
    assert [int(x) for x in seen["modes"]] == [lib.WALK_STRIPS, lib.WALK_SKIP_DIAG] == [0, 1]
    assert int(seen["launch_info"][0]) == ctypes.sizeof(lib.LaunchInfo) == 104      # gamdp_launch_info keeps its layout
    assert int(seen["gamdp_walk_skip_stats"][0]) == ctypes.sizeof(lib.WalkSkipStats) == 48          # ... and so do the other structs
    assert int(seen["gamdp_walk_skip_pair_stats"][0]) == ctypes.sizeof(lib.WalkSkipPairStats) == 56


@PROPS
def test_null_and_unknown_mode_are_einval(prop):
    l = lib.load_library()
    setter, getter = (getattr(l, name) for name in STRUCTS[prop][:2])
    st = STRUCTS[prop][3]()
    assert setter(None, lib.WALK_STRIPS) == lib.EINVAL
    assert setter(None, lib.WALK_SKIP_DIAG) == lib.EINVAL
    assert getter(None, ctypes.byref(st)) == lib.EINVAL
    # the mode is checked before the context is touched: any non-NULL handle will do for an unknown mode
    fake = ctypes.create_string_buffer(8)
    for mode in (-1, 2, 7):
        assert setter(ctypes.cast(fake, ctypes.c_void_p), mode) == lib.EINVAL
    assert getter(ctypes.cast(fake, ctypes.c_void_p), None) == lib.EINVAL


@PROPS
def test_the_stand_in_library_exports_them(prop, tmp_path):
    so = tmp_path / "stub.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-o", str(so),
                           os.path.join(ROOT, "integration", "gamdp_stub.c")])
    stub = ctypes.CDLL(str(so))
    setter, getter = (getattr(stub, name) for name in STRUCTS[prop][:2])
    st = STRUCTS[prop][3]()
    assert setter(None, lib.WALK_SKIP_DIAG) != 0
    assert getter(None, ctypes.byref(st)) != 0
