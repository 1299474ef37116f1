"""gamdp_score_batch (k_score, gam_ngs_amd/csrc/gamdp_score.hip): score and end cell of find_alignment without the traceback.

Every test is a section the fill-only calls share (tests/_fillonly_sections.py) for the kind "score"; what is compared -- (score, end
cell, status, cells), the end cell from the expected alignment and its edit string -- is in tests/_fillonly.py.
"""
import pytest

import _fillonly_sections as S

pytestmark = pytest.mark.gpu

globals().update(S.tests_for("score", names={
    "test_the_other_calls_records_stay_and_kernel_time_grows": "test_launch_info_stays_with_align_batch_and_kernel_time_grows",
    "test_a_batch_the_arena_cannot_hold_is_filled_all_the_same": "test_a_batch_the_arena_cannot_hold_is_scored_all_the_same"}))
