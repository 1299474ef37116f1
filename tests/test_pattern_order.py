"""tests/native/pattern_order_test.cpp -- the pattern format of the two-task band-512 kernel (PAT_OFF, pat_encode, pat_decode of
gam_ngs_amd/csrc/gamdp_dev.h) checked exhaustively on the CPU: f16 order == integer order over 0x0400 ... 0x7BFF and 0xFC00, the packed
32-bit add of two scores == two 16-bit adds over the live range, encode / decode round-trip -- built with g++ under ASan + UBSan, as
tests/test_views_cpu.py builds npre_test.cpp."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pattern_order_add_and_round_trip_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "pattern_order_test")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
           os.path.join(ROOT, "gam_ngs_amd", "csrc"), os.path.join(ROOT, "tests", "native", "pattern_order_test.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and ("cannot find" in b.stderr or "unrecognized" in b.stderr):
        pytest.skip("sanitizer runtime not installed: " + b.stderr[-200:])
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "bad 0" in r.stdout
