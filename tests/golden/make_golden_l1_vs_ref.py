#!/usr/bin/env python3
"""Generates tests/golden/l1_vs_ref.json.gz: the REFERENCE's merge-block driver's answers (oracle/_ref/libgaml1ref.so:
PctgBuilder::alignMergeBlock and the functions it calls, cut out of the reference's PctgBuilder.cc) to the seeded inputs of
tests/test_l1_oracle_vs_ref.py, with a hash of those inputs and the sha256 of the reference files the functions were
cut from.  Run where the L1 reference library is built (oracle/Makefile, target ref: needs the reference's source tree):

    python tests/golden/make_golden_l1_vs_ref.py              # writes the file (byte-identical when nothing changed)
    python tests/golden/make_golden_l1_vs_ref.py --coverage   # the same inputs through the --coverage build: prints
                                                              # the line coverage of the five functions, writes nothing

Inputs the oracle reports as INVALID (the reference would have undefined behaviour) are not sent to the reference;
their answer is null."""
import gzip
import json
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _l1ref as R  # noqa: E402
import _oracle as O  # noqa: E402
import test_l1_oracle_vs_ref as T  # noqa: E402
from _l1oracle import oracle_mb  # noqa: E402

def answers(lib):
    out = {}
    for group, make in T.GROUPS.items():
        cases = make()
        ans = []
        for k, sc in enumerate(cases):
            if oracle_mb(sc)[0].status == O.INVALID:
                ans.append(None)
            else:
                ans.append(R.answer(sc, full_trail=T.full_trail(group, k), lib_=lib))
        out[group] = dict(inputs_sha=T.digest(cases), answers=ans)
    return out


def coverage():
    """runs every input through the --coverage build in a child process (the counters are written when it exits), then
    gcov; returns the directory of the .gcov files"""
    subprocess.check_call(["make", "-s", "-C", O.ORACLE_DIR, "ref_l1_cov"])
    cov = os.path.join(O.ORACLE_DIR, "_ref", "cov")
    for f in os.listdir(cov):
        if f.endswith(".gcda") or f.endswith(".gcov"):
            os.remove(os.path.join(cov, f))
    code = ("import sys; sys.path[:0] = [%r, %r]; import _l1ref as R; R.PATH = %r; import make_golden_l1_vs_ref as M; "
            "M.answers(R.lib())" % (os.path.dirname(HERE), HERE, os.path.join(cov, "libgaml1ref.so")))
    subprocess.check_call([sys.executable, "-c", code])
    subprocess.check_call(["gcov", "-o", cov, os.path.join(cov, "ref_l1_shim.o")], cwd=cov, stdout=subprocess.DEVNULL)
    return cov


def report(cov):
    """line coverage of the five functions from the .gcov file of the reference's PctgBuilder.cc"""
    path = next(os.path.join(cov, f) for f in os.listdir(cov) if f.startswith("PctgBuilder.cc") and f.endswith(".gcov"))
    lines = {}
    for ln in open(path, encoding="latin-1"):
        m = re.match(r"\s*([^:]+):\s*(\d+):(.*)$", ln)
        if m and int(m.group(2)) > 0:
            lines[int(m.group(2))] = (m.group(1).strip(), m.group(3))
    total = hit = 0
    missed = []
    for n, (count, text) in sorted(lines.items()):
        if count == "-":
            continue
        total += 1
        if count.startswith("#") or count.startswith("="):
            missed.append((n, text.strip()))
        else:
            hit += 1
    print("line coverage of the five reference functions: %d / %d lines" % (hit, total))
    for n, text in missed:
        print("  not reached: PctgBuilder.cc:%d  %s" % (n, text))


def main():
    if "--coverage" in sys.argv[1:]:
        report(coverage())
        return
    lib = R.lib()
    assert lib is not None, "oracle/_ref/libgaml1ref.so is needed (make -C oracle)"
    out = dict(sources_sha256=lib.gamref_l1_sources_sha256().decode(), groups=answers(lib))
    with gzip.GzipFile(T.GOLDEN, "wb", mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":"), sort_keys=True).encode())
    n = sum(len(g["answers"]) for g in out["groups"].values())
    print("wrote", T.GOLDEN, os.path.getsize(T.GOLDEN), "bytes,", n, "answers")


if __name__ == "__main__":
    main()
