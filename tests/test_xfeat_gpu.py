"""MI355X: the gfx950 XFeat kernels against the reference module's goldens and tests/xfeat_ref.py (cases in tests/xfeat_cases.py)."""
import pytest

from tests import xfeat_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(cases.GOLDEN_CASES))
def test_xfeat_golden(hip_lib, name):
    cases.golden(hip_lib, "cuda", name)


def test_xfeat_photograph_top_k_4096(hip_lib):
    cases.photo_case(hip_lib, "cuda")


def test_xfeat_batch_is_bit_identical_and_handles_can_be_reused(hip_lib):
    cases.batch_and_reuse(hip_lib, "cuda")


def test_xfeat_range_guard_fires_and_the_guarded_rerun_equals_the_golden(hip_lib):
    cases.guard(hip_lib, "cuda")


@pytest.mark.parametrize("hw", [(32, 32), (64, 96)])
def test_xfeat_selection_rules_on_crafted_maps(hip_lib, hw):
    cases.select_cases(hip_lib, "cuda", hw)


def test_xfeat_feeds_the_nearest_neighbour_matcher(hip_lib):
    cases.chain(hip_lib, "cuda")
