"""CPU checks of gamdp_find_hits_batch (the batched ABlast::findHits of include/gamdp.h): the library exports it, the
ctypes structs match the header's layout as a C compiler sees it, and the argument checks need no GPU."""
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
    printf("gamdp_hits_task %zu\n", sizeof(gamdp_hits_task));
    F(gamdp_hits_task, a_id); F(gamdp_hits_task, b_id); F(gamdp_hits_task, a_off); F(gamdp_hits_task, b_off);
    F(gamdp_hits_task, a_rc); F(gamdp_hits_task, b_rc); F(gamdp_hits_task, word); F(gamdp_hits_task, a_start);
    F(gamdp_hits_task, a_end); F(gamdp_hits_task, b_start); F(gamdp_hits_task, b_end);
    printf("gamdp_hits_result %zu\n", sizeof(gamdp_hits_result));
    F(gamdp_hits_result, n_hits); F(gamdp_hits_result, votes); F(gamdp_hits_result, first); F(gamdp_hits_result, last);
    F(gamdp_hits_result, status);
    return 0;
}
"""


def test_find_hits_batch_is_exported():
    assert "gamdp_find_hits_batch" in lib.SYMBOLS
    assert hasattr(lib.load_library(), "gamdp_find_hits_batch")


def test_hits_structs_match_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    seen = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    for cname, cls in (("gamdp_hits_task", lib.HitsTask), ("gamdp_hits_result", lib.HitsResult)):
        assert int(seen[cname]) == ctypes.sizeof(cls), cname
        for field, _ in cls._fields_:
            if field != "pad_":
                assert int(seen["%s.%s" % (cname, field)]) == getattr(cls, field).offset, (cname, field)
    assert ctypes.sizeof(lib.HitsTask) == 64 and ctypes.sizeof(lib.HitsResult) == 32


def test_null_arguments_are_einval():
    l = lib.load_library()
    out = (lib.HitsResult * 1)()
    tasks = (lib.HitsTask * 1)()
    assert l.gamdp_find_hits_batch(None, None, None, None, 0, None, None, None, None) == lib.EINVAL
    assert l.gamdp_find_hits_batch(None, None, None, tasks, 1, out, None, None, None) == lib.EINVAL
