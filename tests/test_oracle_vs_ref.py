"""Pins oracle/gamdp_oracle.c against the reference's own code.

Every test feeds the oracle seeded inputs and compares its answers with what the reference returned for exactly those
inputs, stored in tests/golden/oracle_vs_ref.json.gz (written by tests/golden/make_golden_vs_ref.py through
oracle/_ref/libgamref.so), so the tests stand on the repository alone.  Where the reference build is present, its live
answers are compared with the stored ones as well.
"""
import ctypes
import gzip
import hashlib
import json
import os
import random
import zlib

import pytest

import _cases
import _oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_vs_ref.json.gz")
_golden = None


# ---- the inputs (tests/golden/make_golden_vs_ref.py records the reference's answers to exactly these) ----

def random_cases(seed):
    return _cases.cases(1000 + seed, 700)


def out_of_range_cases():
    return _cases.cases(77, 3000, max_len=80, bands=(0, 1, 2, 5, 8))


def beyond_cases():
    return _cases.beyond_cases(31, 1500)


def medium_cases():
    rng = random.Random(5)
    out = []
    for n, band in ((3000, 150), (2500, 512), (4000, 20)):
        a, b = _cases.related_pair(rng, n, n_frac=0.01)
        out.append(dict(a=a.encode(), b=b.encode(), band=band, begin_a=0, end_a=len(a) - 1, begin_b=0,
                        end_b=len(b) - 1, fs=False, fe=False))
    return out


TIE_BANDS, TIE_NS, TIE_PER = _cases.TIE_BANDS, _cases.TIE_NS, _cases.TIE_PER   # (tests/_ties.py takes them from there too)


def tie_window_cases():
    return _cases.tie_window_cases(0, TIE_BANDS, TIE_NS, TIE_PER)


ALIGN_GROUPS = dict([("random_%d" % s, (lambda s=s: random_cases(s))) for s in range(8)] +
                    [("out_of_range", out_of_range_cases), ("beyond", beyond_cases), ("medium", medium_cases),
                     ("tie_windows", tie_window_cases)])

NORMALISE_INPUT = b"acgtnACGTNRYKMxX-*"


def revcomp_inputs():
    rng = random.Random(3)
    return [_cases.rand_seq(rng, n, 0.05).encode() for n in (0, 1, 2, 3, 59, 60, 61, 120, 1001)]


def find_hits_inputs(seed):
    rng = random.Random(4000 + seed)
    out = []
    for _ in range(400):
        word = rng.choice([4, 8, 12, 20])
        la, lb = rng.randint(0, 200), rng.randint(0, 200)
        kind = rng.random()
        if kind < 0.5 and la >= 30:
            a = _cases.rand_seq(rng, la, 0.03 if rng.random() < 0.3 else 0)
            off = rng.randint(0, la // 2)
            b = _cases.mutate(rng, a[off:], 0.01, 0.0, 0.0)
        elif kind < 0.7:
            a = "".join(rng.choice("AC") for _ in range(la))
            b = "".join(rng.choice("AC") for _ in range(lb))
        else:
            a, b = _cases.rand_seq(rng, la), _cases.rand_seq(rng, lb)
        a, b = a.encode(), b.encode()
        a_s, a_e = rng.randint(0, max(0, len(a) // 3)), rng.randint(0, len(a) + 5)
        b_s, b_e = rng.randint(0, max(0, len(b) // 3)), rng.randint(0, len(b) + 5)
        out.append((a, a_s, a_e, b, b_s, b_e, word))
    return out


def digest(items):
    """sha256 of the inputs, stored next to the answers: a changed generator fails loudly instead of comparing
    answers to other questions."""
    h = hashlib.sha256()
    for x in items:
        h.update(repr(sorted(x.items()) if isinstance(x, dict) else x).encode())
    return h.hexdigest()[:16]


ALIGN_ARGS = ("band", "begin_a", "end_a", "begin_b", "end_b", "fs", "fe")


def ref_answer(c):
    """What the reference returns for one case: (key, crc32 of the edit string)."""
    rr, rops = O.ref_align(c["a"], c["b"], *[c[k] for k in ALIGN_ARGS])
    return list(O.ref_key(rr)), zlib.crc32(rops.encode())


# ---- the stored answers ----

def golden():
    global _golden
    if _golden is None:
        with gzip.open(GOLDEN, "rt") as f:
            _golden = json.load(f)
    return _golden


def stored(group, inputs):
    g = golden()[group]
    assert g["inputs_sha"] == digest(inputs), "the inputs of %s changed: regenerate %s" % (group, GOLDEN)
    return g["answers"]


def check_case(c, want):
    a, b = O.encode(c["a"]), O.encode(c["b"])
    r, ops = O.oracle_align(a, b, *[c[k] for k in ALIGN_ARGS])
    if r.status == O.INVALID:
        return "invalid"
    key, crc = want
    assert r.key() == tuple(key), (c, r.key(), key)
    assert zlib.crc32(ops.encode()) == crc, c
    if O.ref() is not None:
        rr, rops = O.ref_align(c["a"], c["b"], *[c[k] for k in ALIGN_ARGS])
        assert O.ref_key(rr) == tuple(key) and ops == rops, (c, O.ref_key(rr), key)
    return r.status


def check_group(group):
    cases = ALIGN_GROUPS[group]()
    return [check_case(c, w) for c, w in zip(cases, stored(group, cases))]


@pytest.mark.parametrize("seed", range(8))
def test_random_cases_match_reference(seed):
    stats = {}
    for s in check_group("random_%d" % seed):
        stats[s] = stats.get(s, 0) + 1
    assert stats.get(O.OK, 0) > 300
    assert stats.get("invalid", 0) == 0


def test_out_of_range_cases_exist_and_match():
    assert sum(1 for s in check_group("out_of_range") if s == O.OUT_OF_RANGE) >= 5


def test_begin_a_at_or_past_the_end_of_a_matches_reference():
    """begin_a >= |a| (up to far past it): the reference's row bound wraps; outcomes are EMPTY / OUT_OF_RANGE only"""
    stats = {}
    for s in check_group("beyond"):
        stats[s] = stats.get(s, 0) + 1
    assert stats.get(O.OUT_OF_RANGE, 0) > 100 and stats.get(O.EMPTY, 0) > 100, stats


def test_medium_pairs_band150_and_512():
    assert check_group("medium") == [O.OK] * 3


def test_tie_rich_windowed_and_forced_long_pairs_match_reference():
    """tests/_cases.py tie_window_cases: windows, force flags and N on the adversarial pairs, 0.7 and 2.6 kb at a band of every
    kernel family.  These are the expected values of tests/test_gpu_tie_windows.py; the conditions below keep a change of the
    generator from hollowing the group out (they hold for the reference's answers alone)."""
    cases = tie_window_cases()
    status = check_group("tie_windows")
    assert len(cases) == len(TIE_BANDS) * len(_cases.ADVERSARIAL_KINDS) * len(TIE_NS) * TIE_PER
    assert "invalid" not in status
    ok = [c for c, s in zip(cases, status) if s == O.OK]
    assert 2 * len(ok) >= len(cases), (len(ok), len(cases))
    for flags in _cases.TIE_FLAGS:
        n_all = sum(1 for c in cases if (c["fs"], c["fe"]) == flags)
        n_ok = sum(1 for c in ok if (c["fs"], c["fe"]) == flags)
        assert n_all > 0 and 4 * n_ok >= n_all, (flags, n_ok, n_all)
    missing = {(k, b) for k in _cases.ADVERSARIAL_KINDS for b in TIE_BANDS} - {(c["tag"][0], c["band"]) for c in ok}
    assert not missing, sorted(missing)
    assert sum(1 for c in ok if b"N" in c["a"] or b"N" in c["b"]) >= 100


def ref_normalise(s):
    buf = ctypes.create_string_buffer(s, len(s))
    O.ref().gamref_normalise(buf, len(s))
    return buf.raw[:len(s)].decode()


def ref_revcomp(s):
    buf = ctypes.create_string_buffer(s, max(1, len(s)))
    O.ref().gamref_reverse_complement(buf, len(s))
    return buf.raw[:len(s)].decode()


def test_iupac_and_lowercase_normalise_like_reference():
    want = stored("normalise", [NORMALISE_INPUT])[0]
    if O.ref() is not None:
        assert ref_normalise(NORMALISE_INPUT) == want
    assert O.decode(O.encode(NORMALISE_INPUT)) == want


def test_reverse_complement_matches_reference():
    inputs = revcomp_inputs()
    for s, want in zip(inputs, stored("revcomp", inputs)):
        if O.ref() is not None:
            assert ref_revcomp(s) == want
        n = len(s)
        codes = ctypes.create_string_buffer(O.encode(s), max(1, n))
        O.oracle().gamdp_oracle_revcomp(codes, n)
        assert O.decode(codes.raw[:n]) == want


@pytest.mark.parametrize("seed", range(3))
def test_find_hits_matches_reference(seed):
    inputs = find_hits_inputs(seed)
    n_nonempty = 0
    for (a, a_s, a_e, b, b_s, b_e, word), want in zip(inputs, stored("find_hits_%d" % seed, inputs)):
        if O.ref() is not None:
            assert O.ref_find_hits(a, a_s, a_e, b, b_s, b_e, word) == want
        got = O.oracle_find_hits(O.encode(a), a_s, a_e, O.encode(b), b_s, b_e, word)
        assert got == want, (a, b, a_s, a_e, b_s, b_e, word)
        n_nonempty += bool(want)
    assert n_nonempty > 50
