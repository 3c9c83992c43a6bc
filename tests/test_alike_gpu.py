"""MI355X: the gfx950 ALIKE kernels against the reference modules' goldens and tests/alike_ref.py (cases in tests/alike_cases.py)."""
import pytest

from tests import alike_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(cases.GOLDEN_CASES))
def test_alike_golden(hip_lib, name):
    cases.golden(hip_lib, "cuda", name)


@pytest.mark.parametrize("model", ["alike-t", "alike-s", "alike-n", "alike-l"])
def test_alike_trained_weights_at_a_realistic_size_keep_the_range_guard_silent(hip_lib, model):
    cases.trained_realistic(hip_lib, "cuda", model)


def test_alike_default_configuration_of_deep_image_matching(hip_lib):
    cases.dim_default(hip_lib, "cuda")


def test_alike_top_k_fills_up_with_zero_score_pixels(hip_lib):
    cases.zero_fill(hip_lib, "cuda")


@pytest.mark.parametrize("scores_th", [0.0, 0.9999])
def test_alike_mean_threshold_fallback(hip_lib, scores_th):
    cases.mean_threshold(hip_lib, "cuda", scores_th)


@pytest.mark.parametrize("model,big", [("alike-t", False), ("alike-n", True), ("alike-l", True)])
def test_alike_batch_is_bit_identical_and_handles_can_be_reused(hip_lib, model, big):
    cases.batch_and_reuse(hip_lib, "cuda", model, big)


def test_alike_desc_stride_feeds_the_nearest_neighbour_matcher(hip_lib):
    cases.desc_stride_and_matcher(hip_lib, "cuda")
