"""The launches that make up a decode frame, in order: qtts_dev_profile_frame's
(kind, kernel name, bytes) lists of step 0 and step 1 against
tests/golden/frame_launches.json (tests/frame_launches.py: the cases, and how
the fixture was recorded).  The host code that builds a frame decides this
list and nothing else does, so a change there that drops, adds, reorders or
re-routes a launch fails here by name.  No timing is read.

The cases are the smallest models at which every branch of the sub-talker
chain is taken: plain tiny / tiny_eq (Hs 64, the generic GEMV), the same with
the sub-talker shapes of the lean kernels (the pair pass, the fused attention
+ O and the layer-0 table at batch 1), the two switches that turn those off,
batch 2 (the lock-step chain with split-K) and batch 17 (the wide kernel).
"""
import pytest

from frame_launches import CASES, case_launches, first_difference, fixture

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(CASES))
def test_frame_launches_equal_the_recorded_list(gpu, name):
    want = fixture()[name]
    got = case_launches(name)
    print(f"{name}: {len(got['step0'])} launches in step 0, {len(got['step1'])} in step 1")
    assert first_difference(got, want) is None, first_difference(got, want)
