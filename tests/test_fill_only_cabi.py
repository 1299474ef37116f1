"""CPU checks of the fill-only calls (gamdp_score_batch, gamdp_carry_batch, gamdp_carry_ops_batch and their gamdp_ctx_*_info of
include/gamdp.h) and of the edit-string fingerprint (gamdp_ops_fingerprint): the library and the stand-in library of integration/
export them, the ctypes structs match the header's layout as a C compiler sees it, the argument checks need no GPU, the end-cell rule
the GPU tests derive their expectation by holds on the reference's golden vectors, and the fingerprint equals its three-line
definition on the reference's own edit strings, with the two guarantees the header states checked exhaustively for every string of up
to 6 ops."""
import ctypes
import itertools
import os
import subprocess

import pytest

import _fillonly as F
import _golden as G
from gam_ngs_amd import api, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MULT = 0x9E3779B1
KINDS = F.KINDS   # the table of the three calls the GPU tests go by (tests/_fillonly.py; importing it needs no GPU)
EACH_CALL = pytest.mark.parametrize("kind", sorted(KINDS))


def getter_of(kind):
    return "gamdp_ctx_" + KINDS[kind].info   # Context.score_info reads gamdp_ctx_score_info, and so on


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


@EACH_CALL
def test_the_call_is_exported_and_listed(kind):
    l = lib.load_library()
    k = KINDS[kind]
    for name in (k.symbol, getter_of(kind)) + (("gamdp_ops_fingerprint",) if k.with_fp else ()):
        assert name in lib.SYMBOLS
        assert hasattr(l, name)
    assert getattr(l, k.symbol).argtypes[5] == ctypes.POINTER(k.struct)              # (a gamdp_result per call, as gamdp_align_batch, or a gamdp_score_result)
    assert len(getattr(l, k.symbol).argtypes) == 6 + k.with_fp
    assert getattr(l, getter_of(kind)).argtypes[1] == ctypes.POINTER(lib.ScoreLaunchInfo)   # the three logs share a layout
    if k.with_fp:
        header = open(os.path.join(ROOT, "include", "gamdp.h")).read()
        assert "#define GAMDP_OPS_FP_MULT 0x9E3779B1u" in header


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


@EACH_CALL
def test_the_python_api_has_the_call(kind):
    assert callable(getattr(api.BandedSmithWaterman, KINDS[kind].method)) and callable(getattr(api.Context, KINDS[kind].info))


@EACH_CALL
def test_null_arguments_are_einval_before_anything_is_touched(kind):
    l = lib.load_library()
    k = KINDS[kind]
    fn, getter = getattr(l, k.symbol), getattr(l, getter_of(kind))
    fake = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)   # (never read: every call below is refused on its NULLs)
    tasks, out = (lib.Task * 1)(), (k.struct * 1)()
    fp = ((ctypes.c_uint32 * 1)(),) if k.with_fp else ()
    for args in ((None, None, None, None, 0, None), (None, fake, fake, tasks, 1, out), (fake, None, fake, tasks, 1, out), (fake, fake, None, tasks, 1, out),
                 (fake, fake, fake, tasks, 1, None), (fake, fake, fake, tasks, 0, None),   # out, whatever n
                 (fake, fake, fake, None, 1, out)):                                        # tasks with n > 0
        assert fn(*(args + (fp if args[0] else (None,) * k.with_fp))) == lib.EINVAL, args
    if k.with_fp:   # ops_fp, whatever n
        for args in ((fake, fake, fake, tasks, 1, out, None), (fake, fake, fake, tasks, 0, out, None), (fake, fake, fake, None, 0, out, None)):
            assert fn(*args) == lib.EINVAL, args
    n = ctypes.c_size_t()
    assert getter(None, None, 0, None) == lib.EINVAL
    assert getter(None, None, 0, ctypes.byref(n)) == lib.EINVAL
    assert getter(fake, None, 1, ctypes.byref(n)) == lib.EINVAL


def test_end_cell_rule_on_the_golden_l0_cases():
    """The GPU tests derive the expected end cell from an expected alignment: end_a = begin_a + #MATCH + #MISMATCH + #GAP_B - 1, end_b =
    begin_b + #MATCH + #MISMATCH + #GAP_A - 1.  Checked here on the reference's golden vectors, in their own terms: every alignment has
    an edit string, and walking it by that rule from (begin_a, begin_b) meets the recorded first and last match and ends inside both
    windows -- on a base of a (the traceback reads a.at(pos) there), within the rows of the b window."""
    n = 0
    for name, cs, e in G.l0_cases():
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


def fp_py(codes):
    """F(empty) = 0, F(s . e) = F(s) * M + (e + 1) mod 2^32: the definition, in Python"""
    f = 0
    for e in codes:
        f = (f * MULT + e + 1) & 0xFFFFFFFF
    return f


def test_the_stand_in_library_exports_them(tmp_path):
    so = tmp_path / "stub.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-o", str(so),
                           os.path.join(ROOT, "integration", "gamdp_stub.c")])
    stub = ctypes.CDLL(str(so))
    n = ctypes.c_size_t(7)
    assert stub.gamdp_carry_ops_batch(None, None, None, None, 0, None, None) != 0
    assert stub.gamdp_ctx_carry_ops_info(None, None, 0, ctypes.byref(n)) != 0 and n.value == 0
    stub.gamdp_ops_fingerprint.argtypes = [ctypes.c_char_p, ctypes.c_uint64]
    stub.gamdp_ops_fingerprint.restype = ctypes.c_uint32
    for codes in (b"", bytes([2, 2, 3, 0, 1, 2]), bytes(range(256))):
        assert stub.gamdp_ops_fingerprint(codes, len(codes)) == fp_py(codes)   # (it needs no device: the stand-in's is the real one)


def golden_ops():
    out = []
    for _, _, e in G.l0_cases():
        assert "ops" in e
        out.append(bytes("ABMX".index(ch) for ch in e["ops"]))
    return out


def test_the_fingerprint_equals_its_definition():
    l = lib.load_library()
    strings = golden_ops()
    assert len(strings) == 673 and max(len(s) for s in strings) == 310
    for s in strings:
        assert l.gamdp_ops_fingerprint(s, len(s)) == fp_py(s) == api.ops_fingerprint(s)
        assert api.ops_fingerprint("".join("ABMX"[c] for c in s)) == fp_py(s)   # MyAlignment.ops as it comes
    assert len({fp_py(s) for s in strings}) == len(set(strings))   # distinct strings, distinct fingerprints
    # the empty string, however it is given; n bytes of a longer buffer
    assert l.gamdp_ops_fingerprint(None, 0) == l.gamdp_ops_fingerprint(None, 5) == l.gamdp_ops_fingerprint(b"", 0) == 0
    assert l.gamdp_ops_fingerprint(b"\x02\x02\x02", 0) == 0 and api.ops_fingerprint("") == api.ops_fingerprint(b"") == api.ops_fingerprint([]) == 0
    assert l.gamdp_ops_fingerprint(bytes([2, 3, 0, 1]), 2) == fp_py([2, 3])
    # a total function: every byte value e contributes e + 1 (a 0 byte is an op, not an end)
    for codes in (bytes([0]), bytes([0, 0, 0]), bytes([4]), bytes([255]), bytes([2, 255, 0, 7, 3]), bytes(range(256)), bytes([255] * 1000)):
        assert l.gamdp_ops_fingerprint(codes, len(codes)) == fp_py(codes) == api.ops_fingerprint(codes), codes[:8]
    assert fp_py([0]) == 1 and fp_py([3]) == 4 and fp_py([255]) == 256 and fp_py([0, 0]) == (MULT + 1) & 0xFFFFFFFF
    assert api.ops_fingerprint([2, 0, 1]) == fp_py([2, 0, 1])


def test_the_two_guarantees_hold_for_every_string_of_up_to_six_ops():
    """Equal length and exactly one op different: different fingerprints.  Two adjacent unequal ops swapped: different fingerprints.
    Checked with the library's function for all 4 + 16 + ... + 4096 strings."""
    l = lib.load_library()
    pairs = 0
    for n in range(1, 7):
        f = {s: l.gamdp_ops_fingerprint(bytes(s), n) for s in itertools.product(range(4), repeat=n)}
        assert len(f) == 4 ** n
        for s, fs in f.items():
            assert fs == fp_py(s)
            for k in range(n):
                for e in range(4):
                    if e != s[k]:
                        assert f[s[:k] + (e,) + s[k + 1:]] != fs, (s, k, e)
                        pairs += 1
                if k + 1 < n and s[k] != s[k + 1]:
                    assert f[s[:k] + (s[k + 1], s[k]) + s[k + 2:]] != fs, (s, k)
                    pairs += 1
    assert pairs > 100000
