"""CPU checks of gamdp_score_batch (score and end cell without the traceback, include/gamdp.h): the library exports it, the ctypes
structs match the header's layout as a C compiler sees it, and the argument checks need no GPU."""
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
    printf("gamdp_score_result %zu\n", sizeof(gamdp_score_result));
    F(gamdp_score_result, score); F(gamdp_score_result, end_a); F(gamdp_score_result, end_b); F(gamdp_score_result, cells);
    F(gamdp_score_result, status);
    printf("gamdp_score_launch_info %zu\n", sizeof(gamdp_score_launch_info));
    F(gamdp_score_launch_info, kernel); F(gamdp_score_launch_info, cols); F(gamdp_score_launch_info, tasks);
    F(gamdp_score_launch_info, slots); F(gamdp_score_launch_info, band_max); F(gamdp_score_launch_info, kernel_ms);
    return 0;
}
"""


def test_score_batch_is_exported():
    l = lib.load_library()
    for name in ("gamdp_score_batch", "gamdp_ctx_score_info"):
        assert name in lib.SYMBOLS
        assert hasattr(l, name)


def test_score_structs_match_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    seen = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    for cname, cls in (("gamdp_score_result", lib.ScoreResult), ("gamdp_score_launch_info", lib.ScoreLaunchInfo)):
        assert int(seen[cname]) == ctypes.sizeof(cls), cname
        for field, _ in cls._fields_:
            if field != "pad_":
                assert int(seen["%s.%s" % (cname, field)]) == getattr(cls, field).offset, (cname, field)
    assert ctypes.sizeof(lib.ScoreResult) == 40 and ctypes.sizeof(lib.ScoreLaunchInfo) == 48


def test_null_arguments_are_einval():
    l = lib.load_library()
    out = (lib.ScoreResult * 1)()
    tasks = (lib.Task * 1)()
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))   # never dereferenced: the NULL checks come first
    assert l.gamdp_score_batch(None, None, None, None, 0, None) == lib.EINVAL
    assert l.gamdp_score_batch(None, fake, fake, tasks, 1, out) == lib.EINVAL       # ctx
    assert l.gamdp_score_batch(fake, None, fake, tasks, 1, out) == lib.EINVAL       # set_a
    assert l.gamdp_score_batch(fake, fake, None, tasks, 1, out) == lib.EINVAL       # set_b
    assert l.gamdp_score_batch(fake, fake, fake, tasks, 1, None) == lib.EINVAL      # out
    assert l.gamdp_score_batch(fake, fake, fake, tasks, 0, None) == lib.EINVAL      # out, whatever n
    assert l.gamdp_score_batch(fake, fake, fake, None, 1, out) == lib.EINVAL        # tasks with n > 0
    assert l.gamdp_ctx_score_info(None, None, 0, None) == lib.EINVAL


def test_end_cell_rule_on_the_golden_l0_cases():
    """The GPU tests derive the expected end cell from an expected alignment: end_a = begin_a + #MATCH + #MISMATCH + #GAP_B - 1, end_b =
    begin_b + #MATCH + #MISMATCH + #GAP_A - 1.  Checked here on the reference's golden vectors, in their own terms: every alignment has
    an edit string, and walking it by that rule from (begin_a, begin_b) meets the recorded first and last match and ends inside both
    windows -- on a base of a (the traceback reads a.at(pos) there), within the rows of the b window."""
    import _golden
    n = 0
    for name, cs, e in _golden.l0_cases():
        if e["status"] != 0 or "ops" not in e:
            continue
        ops = e["ops"]
        assert ops and len(ops) == e["length"], name
        ia, ib, matches = e["begin_a"], e["begin_b"], []
        for op in ops:
            if op == "M":
                matches.append((ia, ib))
            ia += op in "MXB"
            ib += op in "MXA"
        m = ops.count("M") + ops.count("X")
        end_a, end_b = e["begin_a"] + m + ops.count("B") - 1, e["begin_b"] + m + ops.count("A") - 1
        assert (ia - 1, ib - 1) == (end_a, end_b), name
        assert len(matches) == e["n_match"], name
        if matches:
            assert e["first_found"] and e["last_found"], name
            assert matches[0] == (e["first_a"], e["first_b"]) and matches[-1] == (e["last_a"], e["last_b"]), name
        assert 0 <= end_a < len(cs["a"]) and (cs["fe"] or end_a <= cs["end_a"]), name
        assert cs["begin_b"] <= end_b <= min(cs["end_b"], len(cs["b"]) - 1), name
        n += 1
    assert n > 500
