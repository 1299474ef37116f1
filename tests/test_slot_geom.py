"""The rules gamdp_dev.h states once for the host and the kernels -- the band's column count (band_cols, gen_kernel_id) and the layout
of a scratch slot (dir_words_for, slot_geom: the launch planner's slots and the merge-block driver's chain slots) -- against literals,
under AddressSanitizer + UBSan (tests/native/slot_geom_test.cpp).  CPU only (g++)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slot_geom_and_band_rule_against_literals(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "slot_geom_test")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I", os.path.join(ROOT, "gam_ngs_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "slot_geom_test.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and ("cannot find" in b.stderr or "unrecognized" in b.stderr):
        pytest.skip("sanitizer runtime not installed: " + b.stderr[-200:])
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "bad 0" in r.stdout
