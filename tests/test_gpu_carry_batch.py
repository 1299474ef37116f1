"""gamdp_carry_batch (k_carry, gam_ngs_amd/csrc/gamdp_carry.hip): the whole result of find_alignment from a fill alone.

The sections the fill-only calls share (tests/_fillonly_sections.py) with the kind bound to "carry": every field -- the key of the result
(status, begin, score, n_match, length, first and last match, homology) and cells -- equals the CPU oracle's, which
tests/test_oracle_golden.py and tests/test_oracle_vs_ref.py pin to the reference (tests/_fillonly.py).  The tie-rich pairs of
tests/_ties.py come on top: the step the traceback takes from a cell (banded_smith_waterman.cc:229-308) is a tie rule, and it is what
this kernel restates.
"""
import pytest

import _fillonly as F
import _fillonly_sections as S
import _ties as W      # the tie-rich windowed and forced pairs, and what the oracle says about them
from _gpu import ctx

pytestmark = pytest.mark.gpu

KIND = "carry"

globals().update(S.tests_for(KIND, names={
    "test_the_other_calls_records_stay_and_kernel_time_grows": "test_launch_info_and_score_info_stay_and_kernel_time_grows",
    "test_a_batch_the_arena_cannot_hold_is_filled_all_the_same": "test_a_batch_the_arena_cannot_hold_is_carried_all_the_same"}))


# ---- ties: the step rule on homopolymers, dinucleotide and tandem repeats, with windows, force flags and N ---------------

def check_ties(cases, want, band):
    got = F.run(KIND, ctx(), cases, ascii=True)
    assert len(got) == len(cases) == len(want)
    for cs, g, (o, _) in zip(cases, got, want):
        assert g == F.got_of(o), (W.what(cs), g, F.got_of(o))
    info = ctx().carry_info()
    assert [r["kernel"] for r in info] == ["k_carry<%d>" % F.cols_for(band)], info


@pytest.mark.parametrize("band", W.SCORE_BANDS)
def test_tie_rich_windows_by_band(band):
    check_ties(W.band_cases(band), W.wants("band", band), band)


@pytest.mark.parametrize("band", W.LONG_BANDS)
def test_tie_rich_long_pairs_with_partners(band):
    cases, want = W.long_cases(band), W.wants("long", band)
    assert {len(cs["a"]) for cs in cases} >= {6000, 20000}
    check_ties(cases, want, band)
