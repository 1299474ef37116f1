"""gamdp_ctx_set_ops_walk / gamdp_ctx_ops_walk_stats of include/gamdp.h without a walk: the library, the stand-in library of
integration/ and lib.SYMBOLS have both symbols, the ctypes struct matches the header's layout as a C compiler sees it, the argument
checks need no GPU -- and, with one, GAMDP_OPS_WALK_RUNS in the environment sets the mode of new contexts (a child process each: the
library reads it once)."""
import ctypes
import os
import subprocess
import sys

import pytest

from gam_ngs_amd import api, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gamdp_ctx_set_ops_walk", "gamdp_ctx_ops_walk_stats")
FIELDS = ["tasks", "ops_by_run", "ops_by_step", "runs", "mode", "pad_"]

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "gamdp.h"
#define F(m) printf("%s %zu\n", #m, offsetof(gamdp_ops_walk_stats, m))
int main(void)
{
    printf("size %zu\n", sizeof(gamdp_ops_walk_stats));
    F(tasks); F(ops_by_run); F(ops_by_step); F(runs); F(mode); F(pad_);
    printf("modes %d %d\n", GAMDP_OPS_WALK_STEPS, GAMDP_OPS_WALK_RUNS);
    printf("launch_info %zu\n", sizeof(gamdp_launch_info));
    return 0;
}
"""


def test_the_symbols_are_everywhere():
    l = lib.load_library()
    for name in NAMES:
        assert name in lib.SYMBOLS and hasattr(l, name)
    for cls in (api.Context, api.MultiContext):
        assert hasattr(cls, "set_ops_walk") and hasattr(cls, "ops_walk_stats")
    assert (lib.OPS_WALK_STEPS, lib.OPS_WALK_RUNS) == (0, 1)


def test_stats_struct_matches_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    seen = {l.split()[0]: [int(v) for v in l.split()[1:]] for l in subprocess.check_output([str(exe)]).decode().splitlines()}
    assert seen["size"][0] == ctypes.sizeof(lib.OpsWalkStats) == 40
    assert [f for f, _ in lib.OpsWalkStats._fields_] == FIELDS
    for f in FIELDS:
        assert seen[f][0] == getattr(lib.OpsWalkStats, f).offset, f
    assert seen["modes"] == [lib.OPS_WALK_STEPS, lib.OPS_WALK_RUNS]
    assert seen["launch_info"][0] == ctypes.sizeof(lib.LaunchInfo) == 104   # gamdp_launch_info keeps its layout


def check_arguments(l, bad_handle_rc):
    st = lib.OpsWalkStats()
    fake = ctypes.cast(ctypes.create_string_buffer(8), ctypes.c_void_p)
    for mode in (lib.OPS_WALK_STEPS, lib.OPS_WALK_RUNS):
        assert l.gamdp_ctx_set_ops_walk(None, mode) == lib.EINVAL
    for mode in (-1, 2, 7):   # the mode is checked before the context is touched: any non-NULL handle will do
        assert l.gamdp_ctx_set_ops_walk(fake, mode) == lib.EINVAL
    assert l.gamdp_ctx_ops_walk_stats(None, ctypes.byref(st)) == lib.EINVAL
    assert l.gamdp_ctx_ops_walk_stats(fake, None) == lib.EINVAL
    return fake, st


def test_null_and_unknown_mode_are_einval():
    check_arguments(lib.load_library(), None)


def test_the_stand_in_library(tmp_path):
    so = tmp_path / "stub.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-o", str(so),
                           os.path.join(ROOT, "integration", "gamdp_stub.c")])
    stub = ctypes.CDLL(str(so))
    for name in NAMES:
        getattr(stub, name).argtypes = getattr(lib.load_library(), name).argtypes
        getattr(stub, name).restype = ctypes.c_int
    fake, st = check_arguments(stub, None)
    assert stub.gamdp_ctx_set_ops_walk(fake, lib.OPS_WALK_RUNS) == lib.ENODEV     # valid arguments: there is no device behind it
    assert stub.gamdp_ctx_ops_walk_stats(fake, ctypes.byref(st)) == lib.ENODEV


CHILD = ("import sys; sys.path.insert(0, %r)\n"
         "import gam_ngs_amd as gam\n"
         "c = gam.Context(0)\n"
         "import ctypes\nfrom gam_ngs_amd import lib as L\n"
         "out = (L.Result * 1)()\n"
         "s = gam.SequenceSet(c, [b'ACGTACGTAC', b'ACGTACGTAC'], ascii=True)\n"
         "t = (L.Task * 1)()\n"
         "t[0].a_id, t[0].b_id, t[0].band, t[0].end_a, t[0].end_b = 0, 1, 5, 9, 9\n"
         "assert c.lib.gamdp_align_batch(c.handle, s.handle, s.handle, t, 1, out, None) == 0\n"
         "print('ENV_MODE', c.ops_walk_stats()['mode'])\n") % ROOT   # (the mode the call ran in: before the first call it reads 0)


@pytest.mark.gpu
@pytest.mark.parametrize("value, mode", (("1", 1), ("0", 0), (None, 0), ("2", 0)))
def test_the_environment_sets_the_mode_of_new_contexts(value, mode):
    env = {k: v for k, v in os.environ.items() if k != "GAMDP_OPS_WALK_RUNS"}
    if value is not None:
        env["GAMDP_OPS_WALK_RUNS"] = value
    r = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ENV_MODE %d" % mode in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
