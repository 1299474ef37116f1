#!/usr/bin/env python3
"""Generates tests/golden/oracle_vs_ref.json.gz: the REFERENCE's answers (oracle/_ref/libgamref.so) to the seeded inputs
of tests/test_oracle_vs_ref.py -- find_alignment summaries + CRC32 of the edit string, normalisation, reverse
complement, ABlast::findHits lists -- with a hash of those inputs.  Run where oracle/_ref/libgamref.so is built (oracle/Makefile,
target ref: needs the reference's source tree):

    python tests/golden/make_golden_vs_ref.py

Cases the oracle reports as INVALID (the reference would size an impossible matrix) are not sent to the reference,
exactly as the tests skip them; their answer is null."""
import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _oracle as O  # noqa: E402
import test_oracle_vs_ref as T  # noqa: E402


def main():
    assert O.ref() is not None, "oracle/_ref/libgamref.so is needed (make -C oracle)"
    out = {}
    for group, make in T.ALIGN_GROUPS.items():
        cases = make()
        answers = []
        for c in cases:
            r, _ = O.oracle_align(O.encode(c["a"]), O.encode(c["b"]), *[c[k] for k in T.ALIGN_ARGS], want_ops=False)
            answers.append(None if r.status == O.INVALID else T.ref_answer(c))
        out[group] = dict(inputs_sha=T.digest(cases), answers=answers)
    out["normalise"] = dict(inputs_sha=T.digest([T.NORMALISE_INPUT]), answers=[T.ref_normalise(T.NORMALISE_INPUT)])
    rc = T.revcomp_inputs()
    out["revcomp"] = dict(inputs_sha=T.digest(rc), answers=[T.ref_revcomp(s) for s in rc])
    for seed in range(3):
        hits = T.find_hits_inputs(seed)
        out["find_hits_%d" % seed] = dict(inputs_sha=T.digest(hits), answers=[O.ref_find_hits(*h) for h in hits])
    with gzip.GzipFile(T.GOLDEN, "wb", mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":"), sort_keys=True).encode())
    print("wrote", T.GOLDEN, os.path.getsize(T.GOLDEN), "bytes,", sum(len(v["answers"]) for v in out.values()), "answers")


if __name__ == "__main__":
    main()
