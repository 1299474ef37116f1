"""The view cases of tests/_views.py checked on the CPU, and the host functions the kernels' handling of views rests on.

  * the generator: view(stored) == copy byte for byte (with the library's own reverse complement), every axis value present, every
    (kernel cell, view-kind pair) with at least 90 % of its cases aligning in the oracle;
  * npre_window_has_n / call_touches_n (gamdp_dev.h, host and chain kernels: which calls need the N-aware cells, by the window a
    call touches on a view) against brute force, compiled with g++ under ASan + UBSan (tests/native/npre_test.cpp) -- the header needs
    no guard for that: without hipcc GAMDP_HD is empty and the rest is declarations;
  * the Python mirror of that function (the GPU tests' predicate) against brute force as well;
  * the pre-checks on the degenerate views (gamdp_task_preflight on the copy's length) against the oracle."""
import os
import random
import shutil
import subprocess

import pytest

import _oracle as O
import _views as V
from gam_ngs_amd import api, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle(case, want_ops=False):
    return O.oracle_align(case["a"], case["b"], case["band"], case["begin_a"], case["end_a"], case["begin_b"], case["end_b"], case["fs"],
                          case["fe"], want_ops=want_ops)


def test_views_of_the_stored_sequences_are_the_copies():
    cases = V.matrix_cases() + V.nbait_cases()
    dg = V.digest(cases)
    for c in cases:
        V.check_case(c, api.reverse_complement)
    assert V.digest(V.matrix_cases() + V.nbait_cases()) == dg, "the generator is not deterministic"
    # N-free cells hold no N anywhere; the N bait holds N in front of the view only
    for c in cases:
        n_mode = V.CELLS[c["cell"]][2]
        if c["group"] == "main" and n_mode is False:
            assert 4 not in c["stored_a"] and 4 not in c["stored_b"], (dg, c["tag"])
        if c["group"] == "main" and n_mode is True:
            assert V.window_truth_n(c) is True, (dg, c["tag"])
        if c["group"] == "nbait":
            assert 4 not in c["a"] and 4 not in c["b"] and (4 in c["stored_a"] or 4 in c["stored_b"]), (dg, c["tag"])


def test_every_axis_value_is_present():
    cases = V.matrix_cases()
    dg = V.digest(cases)
    tags = [c["tag"] for c in cases]
    assert {t["cell"] for t in tags} == set(V.CELLS) and {V.CELLS[k][0] for k in V.CELLS} == V.kernel_names_in_source(), dg
    for cell, (name, bands, n_mode, env) in V.CELLS.items():
        for band in bands:
            mine = [t for t in tags if t["cell"] == cell and t["band"] == band]
            assert {t["kinds"] for t in mine} == set(V.KIND_PAIRS), (dg, cell, band)
    assert {t["band"] for t in tags} == {150, 512, 1, 63, 64, 95, 96, 159, 160, 287, 288, 543, 544, 2048}, dg
    offs = {o for t in tags for o, k in zip(t["off"], t["kinds"]) if "off" in k}
    assert set(V.OFF_RESIDUES) <= offs, (dg, sorted(offs))
    for t in tags:
        if "off" in t["kinds"][0] and "off" in t["kinds"][1]:
            assert t["off"][0] % 16 != t["off"][1] % 16, (dg, t)
    assert any(0 < o < t["band"] and o not in V.OFF_RESIDUES for t in tags for o in t["off"]), dg            # one below the band
    assert any(o > t["band"] + 64 * 17 for t in tags for o in t["off"]), dg                                     # one above all a kernel fetches
    assert {t["prefix"] for t in tags} == set(V.PREFIX_KINDS), dg
    assert {t["nbait_dist"] for t in tags if t["prefix"] == "nbait"} == set(V.NBAIT_DIST), dg
    assert {t["nbait_dist"] for t in (c["tag"] for c in V.nbait_cases())} == set(V.NBAIT_DIST), dg
    assert {t["begin"] for t in tags} == set(V.BEGIN_MODES) and {t["tail"] for t in tags} == {"right", "left", "ends", "chain"}, dg
    for cell in V.LONG_CELLS:
        assert sum(1 for t in tags if t["cell"] == cell and t["n"] >= 20000) >= 2, (dg, cell)
    assert all(t["n"] <= 2000 for t in tags if t["cell"] == "wide"), dg
    # rc + off on the same sequence with an N in the window, at every cell that takes N
    for cell, (name, bands, n_mode, env) in V.CELLS.items():
        if n_mode is not False:
            assert any(t["cell"] == cell and t["want_n"] and "rc+off" in t["kinds"] for t in tags), (dg, cell)


def test_at_least_nine_in_ten_cases_of_every_cell_align():
    """In every (kernel cell, view-kind pair) at least 90 % of the cases have oracle status OK and a non-empty alignment; the cases
    that do not align stay in the comparison (by status)."""
    cases = V.matrix_cases() + V.nbait_cases()
    dg = V.digest(cases)
    cells = {}
    for c in cases:
        o, _ = _oracle(c)
        k = (c["cell"], c["group"], c["tag"]["kinds"])
        good, n = cells.get(k, (0, 0))
        cells[k] = (good + (o.status == O.OK and o.length > 0), n + 1)
        assert o.cells == 0 or c["rows"] * (2 * c["band"] + 1) == o.cells, (dg, c["tag"])   # rows_of() is the reference's x_size
    short = {k: v for k, v in cells.items() if v[0] < 0.9 * v[1]}
    assert not short, (dg, short)
    assert len([k for k in cells if k[1] == "main"]) == 16 * len(V.CELLS)


def test_npre_window_has_n_against_brute_force_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "npre_test")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
           os.path.join(ROOT, "gam_ngs_amd", "csrc"), os.path.join(ROOT, "tests", "native", "npre_test.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and ("cannot find" in b.stderr or "unrecognized" in b.stderr):
        pytest.skip("sanitizer runtime not installed: " + b.stderr[-200:])
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "bad 0" in r.stdout


def test_python_mirror_of_the_window_test_against_brute_force():
    """V.block_answer is what the GPU tests predict launches with: never False when the view's window holds an N, False when no N lies
    within the 256-blocks of the stored sequence that the window touches."""
    rng = random.Random(5)
    n_truth = n_clean = 0
    for _ in range(3000):
        n = rng.choice((1, 255, 256, 257, 600, 1025))
        s = bytearray(V.rand_codes(rng, n))
        for _ in range(rng.choice((0, 1, 1, 3))):
            s[rng.randrange(n)] = 4
        s = bytes(s)
        rc, off = rng.random() < 0.5, rng.choice((0, 1, 16, 17, 255, 256, n - 1, n))
        if off > n:
            continue
        lo, hi = rng.randint(-300, n + 10), rng.randint(-10, n + 300)
        view = V.apply_view(s, rc, off)
        idx = range(max(lo, 0), min(hi, len(view) - 1) + 1)
        truth = any(view[p] == 4 for p in idx)
        fpos = [(n - 1 - (off + p)) if rc else off + p for p in idx]
        near = any(4 in s[f // 256 * 256: f // 256 * 256 + 256] for f in fpos)
        got = V.block_answer(s, rc, off, lo, hi)
        assert not (truth and not got) and not (got and not near), (n, rc, off, lo, hi)
        n_truth += truth
        n_clean += not near
    assert n_truth > 100 and n_clean > 500


def test_degenerate_views_are_settled_like_their_copies():
    """off == len, off == len - 1, rc of sequences of length 1 and 0: the pre-checks on the copy's lengths (what prepare_task hands to
    gamdp_task_preflight) give the oracle's status; off > len has no copy and is INVALID by prepare_task's own check.  The Python
    mirror's view (api.Contig) sizes itself the same way."""
    seen = {}
    for c in V.degenerate_cases():
        a, b = V.apply_view(c["stored_a"], *c["va"]), V.apply_view(c["stored_b"], *c["vb"])
        if a is None or b is None:
            seen["no copy"] = seen.get("no copy", 0) + 1
            continue

        class S:   # what Contig.size() reads
            lengths = [len(c["stored_a"]), len(c["stored_b"])]
        assert api.Contig(S, 0, *c["va"]).size() == len(a) and api.Contig(S, 1, *c["vb"]).size() == len(b), c["tag"]
        st, cells = api.task_preflight(len(a), len(b), c["band"], c["begin_a"], c["end_a"], c["begin_b"], c["end_b"], c["fs"], c["fe"])
        o, _ = O.oracle_align(a, b, c["band"], c["begin_a"], c["end_a"], c["begin_b"], c["end_b"], c["fs"], c["fe"], want_ops=False)
        if st == lib.ST_OK:
            assert o.status != O.INVALID and cells == o.cells, c["tag"]
            seen["runs"] = seen.get("runs", 0) + 1
        else:
            assert (st, cells) == (o.status, o.cells), (c["tag"], st, o.status)
            seen[st] = seen.get(st, 0) + 1
    assert seen.get("no copy", 0) >= 36 and seen.get("runs", 0) >= 20 and len(seen) >= 4, seen
