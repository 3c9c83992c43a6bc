"""MI355X: the gfx950 RIPE kernels against the reference module's goldens and fp64 torch (cases in tests/ripe_cases.py)."""
import pytest

from tests import ripe_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(cases.GOLDEN_CASES))
def test_ripe_golden(hip_lib, name):
    cases.golden(hip_lib, "cuda", name)


def test_ripe_batch_of_three_is_bit_identical_and_handles_can_be_reused(hip_lib):
    cases.batch_and_reuse(hip_lib, "cuda")


def test_ripe_capacity_is_reported_and_no_candidate_raises(hip_lib):
    cases.capacity_and_no_candidate(hip_lib, "cuda")


@pytest.mark.parametrize("shape", cases.DW_SHAPES)
def test_ripe_depthwise_operator_against_fp64(hip_lib, shape):
    cases.op_dw5x5(hip_lib, "cuda", shape)


@pytest.mark.parametrize("channels", [1, 129])
@pytest.mark.parametrize("sizes", cases.RESIZE_SHAPES)
def test_ripe_resize_operator_against_fp64(hip_lib, sizes, channels):
    cases.op_resize(hip_lib, "cuda", sizes, channels)


def test_ripe_nms3_operator_equals_the_torch_expression(hip_lib):
    cases.op_nms3(hip_lib, "cuda")


def test_ripe_hypercolumn_operator_against_fp64(hip_lib):
    cases.op_hypercolumn(hip_lib, "cuda")


def test_ripe_plugin_feeds_the_kornia_matcher(hip_lib):
    cases.chain("cuda")
