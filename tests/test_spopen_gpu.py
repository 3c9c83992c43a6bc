"""GPU: the open SuperPoint extractor on the gfx950 library, on the cases of tests/spopen_cases.py."""
import importlib

import pytest

from tests import spopen_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["keepall", "ragged_pipeline", "topk50", "threshold"])
def test_golden(hip_lib, name):
    cases.golden(hip_lib, "cuda", name)


def test_batch_of_three_and_one_handle_across_sizes(hip_lib):
    cases.batch_and_reuse(hip_lib, "cuda")


def test_sixteen_row_tiles_of_the_production_shapes_equal_the_eight_row_tiles(hip_lib):
    cases.big_tiles(hip_lib, "cuda")


def test_range_guard_sees_negative_values_and_the_fallback_meets_the_bounds(hip_lib):
    cases.range_guard(hip_lib, "cuda")


def test_extractor_plugin_feeds_the_nearest_neighbour_matcher(hip_lib, tmp_path):
    cases.extractor_matcher_chain(importlib.import_module("deep-image-matching_amd.plugins"), tmp_path)


def test_bf16x6_and_unsplit_activation_storage_agree_with_the_default(hip_lib):
    case = cases.CASES["ragged_pipeline"]
    net = cases.make_net(hip_lib, "cuda", case)
    for key, v, back in ((1, 1, 2), (5, 0, 1)):
        try:
            hip_lib.dim_tune_set(key, v)
            out, sat, _ = cases.run_counted(net, cases.image(case))
        finally:
            hip_lib.dim_tune_set(key, back)
        assert sat == 0
        cases.check_against_golden(net, out, "ragged_pipeline", f"ragged_pipeline_cuda_key{key}={v}")
