"""Pins the oracle's merge-block driver (oracle/gamdp_oracle.c gamdp_oracle_align_merge_block) against the reference's
own PctgBuilder::alignMergeBlock, findBestAlignment, alignBlocks and is_good (cut out of the reference's PctgBuilder.cc
at build time, oracle/l1_extract.py + oracle/ref_l1_shim.cc).

The reference's answers to the seeded inputs below are stored in tests/golden/l1_vs_ref.json.gz (written by
tests/golden/make_golden_l1_vs_ref.py), so the tests stand on the repository alone.  Every answer holds the outcome
(thrown, align_ok, coords_set, align_rev, m_start..s_end), n_dp, cells and the CRC32 of the DP trail -- every
find_alignment call's result in call order -- and some hold the whole trail with each call's windows.  Where the L1
reference build exists (needs_ref), its live answers are compared with the stored ones, and a larger unstored sweep
compares it with the oracle directly.
"""
import gzip
import hashlib
import json
import os

import pytest

import _l1cases
import _l1edges
import _l1ref as R
import _oracle as O
from _l1oracle import oracle_mb

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "l1_vs_ref.json.gz")
AUDIT_CAP = R.TRAIL_CAP
FULL_TRAILS = 40  # answers per group stored with their whole trail (all of the edge cases)
_golden = None

# ---- the inputs (tests/golden/make_golden_l1_vs_ref.py records the reference's answers to exactly these) ----

SEEDED = [(500 + k, 60) for k in range(4)] + [(7100 + k, 105) for k in range(12)]  # 1 500 merge blocks
GAGE = [(31, 400_000), (32, 400_000), (33, 600_000)]


def gage_cases(seed, genome_len):
    import _gage as G
    pb = G.problem(seed, genome_len=genome_len)
    flat, _ = G.merge_blocks(pb)
    return [dict(kind="gage", master=G.to_ascii(pb["master"][mb["m_id"]]["seq"]).decode(),
                 slave=G.to_ascii(pb["slave"][mb["s_id"]]["seq"]).decode(), blocks=[tuple(b) for b in mb["blocks"]],
                 tails=tuple(bool(t) for t in mb["tails"])) for mb in flat]


GROUPS = dict([("seeded_%d" % s, (lambda s=s, n=n: _l1cases.scenarios(s, n))) for s, n in SEEDED] +
              [("gage_%d" % s, (lambda s=s, g=g: gage_cases(s, g))) for s, g in GAGE] +
              [("edges", lambda: _l1edges.cases())])


def digest(cases):
    h = hashlib.sha256()
    for c in cases:
        h.update(repr((c["master"], c["slave"], [tuple(b) for b in c["blocks"]], tuple(bool(t) for t in c["tails"]))).encode())
    return h.hexdigest()[:16]


def full_trail(group, k):
    return group == "edges" or k < FULL_TRAILS


# ---- the stored answers ----

def golden():
    global _golden
    if _golden is None:
        with gzip.open(GOLDEN, "rt") as f:
            _golden = json.load(f)
    return _golden


def stored(group, cases):
    g = golden()["groups"][group]
    assert g["inputs_sha"] == digest(cases), "the inputs of %s changed: regenerate %s" % (group, GOLDEN)
    assert len(g["answers"]) == len(cases)
    return g["answers"]


# ---- comparing one answer ----

OUTCOME = ("thrown", "align_ok", "coords_set", "n_dp", "cells", "trail_crc")
COORDS = ("align_rev", "m_start", "m_end", "s_start", "s_end")


def oracle_answer(sc):
    """the oracle's answer in the stored form, and its trail keys"""
    o, aud = oracle_mb(sc, audit_cap=AUDIT_CAP)
    assert o.n_dp <= AUDIT_CAP
    return dict(thrown=o.status == O.OUT_OF_RANGE, status=o.status, align_ok=bool(o.align_ok), coords_set=bool(o.touched),
                align_rev=bool(o.align_rev) if o.touched else False, m_start=o.m_start, m_end=o.m_end,
                s_start=o.s_start, s_end=o.s_end, n_dp=o.n_dp, cells=o.cells, trail_crc=R.trail_crc(aud)), aud


def differences(got, want, got_trail=None):
    """names of what differs between two answers (coordinates only where the reference wrote them); got_trail: the
    keys of got's DP calls, compared call by call with want's full trail where it has one"""
    out = [k for k in OUTCOME if got[k] != want[k]]
    if want["coords_set"] and got["coords_set"]:
        out += [k for k in COORDS if got[k] != want[k]]
    if got_trail is not None and "trail" in want:
        for i, (g, w) in enumerate(zip(got_trail, want["trail"])):
            if list(g) != w[10:]:
                out.append("trail[%d]" % i)
                break
    return out


def check(sc, want):
    got, aud = oracle_answer(sc)
    d = differences(got, want, aud)
    assert not d, "%s: %s differ(s): oracle %s, reference %s" % (sc["kind"], d, {k: got[k] for k in d if k in got},
                                                                   {k: want[k] for k in d if k in want})
    return got


def check_group(group):
    cases = GROUPS[group]()
    answers = stored(group, cases)
    stats = dict(n=0, ok=0, rev=0, bad=0, thrown=0, tails=0)
    for sc, want in zip(cases, answers):
        if want is None:  # the oracle calls these inputs undefined behaviour for the reference: not sent to it
            assert oracle_mb(sc)[0].status == O.INVALID, sc["kind"]
            continue
        check(sc, want)
        stats["n"] += 1
        stats["ok"] += want["align_ok"]
        stats["rev"] += want["align_ok"] and want["align_rev"]
        stats["bad"] += not want["align_ok"]
        stats["thrown"] += want["thrown"]
        stats["tails"] += want["n_dp"] > len(sc["blocks"]) and want["align_ok"]
    return stats


# ---- tests ----

def test_golden_records_the_extracted_sources():
    g = golden()
    assert set(g["groups"]) == set(GROUPS)
    assert g["sources_sha256"].startswith("PctgBuilder.cc:") and "PctgBuilder.hpp:" in g["sources_sha256"]
    if R.lib() is not None:
        assert R.lib().gamref_l1_sources_sha256().decode() == g["sources_sha256"]


@pytest.mark.parametrize("seed,n", SEEDED)
def test_seeded_merge_blocks_match_the_reference(seed, n):
    stats = check_group("seeded_%d" % seed)
    assert stats["n"] >= n - 2 and stats["ok"] >= n // 8 and stats["bad"] >= n // 8, stats


@pytest.mark.parametrize("seed", [s for s, _ in GAGE])
def test_gage_shaped_merge_blocks_match_the_reference(seed):
    stats = check_group("gage_%d" % seed)
    assert stats["n"] >= 20 and stats["ok"] >= stats["n"] // 2, stats


def test_edge_cases_match_the_reference():
    stats = check_group("edges")
    assert stats["n"] >= 100 and stats["rev"] >= 5 and stats["tails"] >= 10, stats


def _edge(kind):
    cases = GROUPS["edges"]()
    answers = stored("edges", cases)
    return [(sc, a) for sc, a in zip(cases, answers) if sc["kind"].startswith(kind)]


def test_edge_cases_reach_what_they_were_built_for():
    """the stored reference answers show that the hand-built cases sit on the edges they are named after"""
    hom = lambda a: [t[-1] for t in a["trail"]]  # noqa: E731
    # main chain at exactly 95 % passes, one match short fails (one call and three calls)
    for sc, a in _edge("hom95-one"):
        assert hom(a)[0] == 95.0 and a["coords_set"], sc["kind"]
    for sc, a in _edge("hom94-one"):
        assert 90.0 < hom(a)[0] < 95.0 and not a["coords_set"], sc["kind"]
    (sc, a), = _edge("hom95-chain")
    assert hom(a)[:3] == [95.0] * 3 and a["align_ok"]
    for sc, a in _edge("hom94-") + [x for x in _edge("hom94") if "chain" in x[0]["kind"]]:
        assert not a["coords_set"], sc["kind"]
    # tail thresholds: 200 aligns the tail, 199 does not; 100..199 fails in alignMergeBlock; 99 passes untouched
    for t, n_dp, ok in ((200, 2, True), (199, 1, False), (100, 1, False), (99, 1, True)):
        for sc, a in _edge("thr-left-%d" % t) + _edge("thr-right-%d" % t):
            assert (a["n_dp"], a["align_ok"]) == (n_dp, ok), sc["kind"]
    # orientation: a tie keeps the forward try first; no reads at all makes no call; a wrong vote is retried
    assert [a["n_dp"] for _, a in _edge("tie-")] == [2, 4]
    assert [a["n_dp"] for _, a in _edge("no-reads")] == [0, 0]
    assert all(a["n_dp"] == 4 and a["align_ok"] for _, a in _edge("vote-wrong"))
    assert all(a["align_rev"] for _, a in _edge("rev-tails"))
    # the clamp case's second call starts at master base 0 after an empty-ish first call
    (sc, a), = _edge("clamp")
    assert a["trail"][1][4] == 0


def test_compare_reports_each_kind_of_difference():
    """the comparison must notice a flipped orientation, an off-by-one coordinate, a flipped verdict, a missed throw
    and a changed DP call"""
    cases = GROUPS["edges"]()
    answers = stored("edges", cases)
    sc, want = next((sc, a) for sc, a in zip(cases, answers) if a and a["coords_set"] and a["align_ok"] and a["align_rev"])
    got, aud = oracle_answer(sc)
    assert differences(got, want, aud) == []
    assert "align_rev" in differences(dict(got, align_rev=not got["align_rev"]), want)
    for k in ("m_start", "m_end", "s_start", "s_end"):
        assert k in differences(dict(got, **{k: got[k] + 1}), want)
    assert "align_ok" in differences(dict(got, align_ok=not got["align_ok"]), want)
    assert "coords_set" in differences(dict(got, coords_set=False), want)
    thrown = next(a for a in golden()["groups"]["seeded_500"]["answers"] + sum((golden()["groups"]["seeded_%d" % s]["answers"] for s, _ in SEEDED[1:]), [])
                  if a and a["thrown"])
    assert "thrown" in differences(dict(thrown, thrown=False), thrown)
    bent = [list(k) for k in aud]
    bent[-1][1] += 1
    assert "trail[%d]" % (len(bent) - 1) in differences(got, want, bent)
    assert "trail_crc" in differences(dict(got, trail_crc=R.trail_crc(bent)), want)


def test_trail_windows_are_the_oracles_windows():
    """every stored full trail: the L0 oracle, given each recorded window of the reference, returns the recorded result
    (the windows, and so the DP calls the driver makes, are the reference's)"""
    n = 0
    for group in GROUPS:
        if group.startswith("gage"):
            continue
        cases = GROUPS[group]()
        for sc, want in zip(cases, stored(group, cases)):
            if not want or "trail" not in want:
                continue
            v = R.views(sc)
            for t in want["trail"]:
                a_tag, a_off, b_tag, b_off, ba, ea, bb, eb, fs, fe = t[:10]
                if a_tag == "?" or b_tag == "?":
                    continue
                r, _ = O.oracle_align(v[a_tag][a_off:], v[b_tag][b_off:], 150, ba, ea, bb, eb, fs, fe, want_ops=False)
                assert list(r.key()) == t[10:], (sc["kind"], t)
                n += 1
    assert n > 500


# ---- live reference (only where oracle/_ref/libgaml1ref.so was built) ----

needs_ref = pytest.mark.skipif(R.lib() is None, reason="oracle/_ref/libgaml1ref.so not built (needs the reference tree)")


@pytest.mark.needs_ref
@needs_ref
@pytest.mark.parametrize("group", ["seeded_500", "seeded_7100", "gage_31", "edges"])
def test_live_reference_gives_the_stored_answers(group):
    cases = GROUPS[group]()
    for k, (sc, want) in enumerate(zip(cases, stored(group, cases))):
        if want is None:
            continue
        assert R.answer(sc, full_trail=full_trail(group, k)) == want, sc["kind"]


@pytest.mark.needs_ref
@needs_ref
@pytest.mark.parametrize("seed", range(5))
def test_live_reference_matches_the_oracle_on_a_larger_sweep(seed):
    """5 000 more seeded merge blocks, not stored: the live reference against the oracle"""
    n = 0
    for sc in _l1cases.scenarios(90000 + seed, 1000):
        if oracle_mb(sc)[0].status == O.INVALID:
            continue
        check(sc, R.answer(sc))
        n += 1
    assert n >= 990
