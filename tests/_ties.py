"""Tie-rich windowed and forced long pairs (tests/_cases.py tie_window_cases) and what the CPU oracle says about them, for
tests/test_gpu_tie_windows.py and for every other file that sends them through a kernel.  No test collects from here.

Random ACGT hardly ever ties; homopolymers, dinucleotide and tandem repeats, complements do all the time.  The oracle is pinned to the
reference's own code on the whole `tie_windows` group by tests/test_oracle_vs_ref.py.
"""
import functools
import random
from concurrent.futures import ThreadPoolExecutor

import _cases
import _oracle as O
from _gpu import oracle_for

SEED = 0
EXTRA_BANDS = (129, 400)          # the generic widths the group's bands leave out: 5 columns per lane (a direction per cell), 17 (direction-free)
SCORE_ONLY_BANDS = (64,)          # k_score<3>: bands 20, 129 and 150 share k_score<2> and <5>
ALIGN_BANDS = _cases.TIE_BANDS + EXTRA_BANDS
SCORE_BANDS = tuple(b for b in ALIGN_BANDS + SCORE_ONLY_BANDS if b <= 543)
LONG_BANDS = (150, 512)
LONG_KINDS = {150: ("homopolymer", "ac_shift1", "tandem19"), 512: ("homopolymer", "ac_shift1", "tandem17")}   # the 20 kb pairs


# ---- the cases and what the oracle says about them, once per process ------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def band_cases(band):
    """(a): the cases of the `tie_windows` group at one of its bands; 2 windows on the 2.6 kb pairs at the other bands"""
    if band in _cases.TIE_BANDS:
        return tuple(_cases.tie_window_cases(SEED, (band,), _cases.TIE_NS, _cases.TIE_PER))
    return tuple(_cases.tie_window_cases(SEED, (band,), (2600,), 2))


@functools.lru_cache(maxsize=None)
def long_cases(band):
    """(b): 4 windows on every 6 kb pair, 2 on three 20 kb pairs (strips, re-centring, ring refills), each followed by an ordinary
    related pair of the same lengths and the same window, without flags: the tasks that share a wavefront differ."""
    tie = _cases.tie_window_cases(SEED, (band,), (6000,), 4)
    tie += [cs for cs in _cases.tie_window_cases(SEED, (band,), (20000,), 2) if cs["tag"][0] in LONG_KINDS[band]]
    rng = random.Random(7700 + band)
    out = []
    for cs in tie:
        a = _cases.rand_seq(rng, len(cs["a"]))
        b = (_cases.mutate(rng, a) + _cases.rand_seq(rng, 64))[:len(cs["b"])]
        out.append(cs)
        out.append(dict(cs, a=a.encode(), b=b.encode(), fs=False, fe=False, tag=("partner of",) + cs["tag"]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def wants(which, band):
    """[(oracle result, edit string)] of band_cases / long_cases"""
    cases = band_cases(band) if which == "band" else long_cases(band)
    with ThreadPoolExecutor(16) as ex:   # (the oracle's C code runs outside the GIL)
        out = list(ex.map(oracle_for, cases))
    assert all(o.status != O.INVALID for o, _ in out)
    return out


def what(cs):
    return (cs["tag"],) + tuple(cs[k] for k in ("band", "begin_a", "end_a", "begin_b", "end_b", "fs", "fe")) + (len(cs["a"]), len(cs["b"]))
