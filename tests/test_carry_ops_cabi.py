"""CPU checks of the edit-string fingerprint (gamdp_ops_fingerprint, gamdp_carry_ops_batch, gamdp_ctx_carry_ops_info of
include/gamdp.h): the library and the stand-in library of integration/ export the three, the argument checks that need no GPU, the
fingerprint against its three-line definition on the reference's own edit strings, and the two guarantees the header states,
exhaustively for every string of up to 6 ops."""
import ctypes
import itertools
import os
import subprocess

import _golden as G
from gam_ngs_amd import api, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gamdp_ops_fingerprint", "gamdp_carry_ops_batch", "gamdp_ctx_carry_ops_info")
MULT = 0x9E3779B1


def fp_py(codes):
    """F(empty) = 0, F(s . e) = F(s) * M + (e + 1) mod 2^32: the definition, in Python"""
    f = 0
    for e in codes:
        f = (f * MULT + e + 1) & 0xFFFFFFFF
    return f


def test_the_three_functions_are_exported_and_listed():
    l = lib.load_library()
    for name in NAMES:
        assert name in lib.SYMBOLS
        assert hasattr(l, name)
    header = open(os.path.join(ROOT, "include", "gamdp.h")).read()
    assert "#define GAMDP_OPS_FP_MULT 0x9E3779B1u" in header
    assert hasattr(api.Context, "carry_ops_info") and hasattr(api.BandedSmithWaterman, "find_results_with_ops_fingerprints")


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


def test_null_arguments_are_einval_before_anything_is_touched():
    l = lib.load_library()
    fake = ctypes.cast(ctypes.create_string_buffer(8), ctypes.c_void_p)   # (never read: every call below is refused on its NULLs)
    tasks, out, fp = (lib.Task * 1)(), (lib.Result * 1)(), (ctypes.c_uint32 * 1)()
    for args in ((None, fake, fake, tasks, 1, out, fp), (fake, None, fake, tasks, 1, out, fp), (fake, fake, None, tasks, 1, out, fp),
                 (fake, fake, fake, None, 1, out, fp), (fake, fake, fake, tasks, 1, None, fp), (fake, fake, fake, tasks, 1, out, None),
                 (fake, fake, fake, tasks, 0, out, None), (fake, fake, fake, None, 0, out, None), (None, None, None, None, 0, None, None)):
        assert l.gamdp_carry_ops_batch(*args) == lib.EINVAL, args
    n = ctypes.c_size_t()
    assert l.gamdp_ctx_carry_ops_info(None, None, 0, ctypes.byref(n)) == lib.EINVAL
    assert l.gamdp_ctx_carry_ops_info(fake, None, 1, ctypes.byref(n)) == lib.EINVAL


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
