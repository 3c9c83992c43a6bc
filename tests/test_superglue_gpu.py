"""MI355X: the gfx950 SuperGlue kernels (sg_kernels.hip, sg_api.hip on the LightGlue GEMM / attention kernels) against the reference module's
goldens and the fp64 oracle (cases in tests/superglue_cases.py)."""
import pytest

from tests import superglue_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(cases.GOLDEN_CASES))
def test_superglue_golden(hip_lib, name):
    cases.golden(hip_lib, "cuda", name)


def test_superglue_golden_in_bf16x6(hip_lib):
    cases.golden(hip_lib, "cuda", "wide", arithmetic="bf16x6")


def test_superglue_sinkhorn_potentials_and_marginals_against_fp64(hip_lib):
    cases.sinkhorn_alone(hip_lib, "cuda")


def test_superglue_sinkhorn_at_1100_by_900(hip_lib):
    """35 rows per row group and four 256-column strides per lane, on the GPU only (the emulator would take minutes)."""
    cases.sinkhorn_alone(hip_lib, "cuda", shapes=[(1100, 900)], label="sinkhorn_big")


def test_superglue_edge_counts(hip_lib):
    cases.edge_counts(hip_lib, "cuda")


def test_superglue_batch_equals_singles_and_handles_can_be_reused(hip_lib):
    cases.batch_equals_singles(hip_lib, "cuda")


def test_superglue_range_guard_fires_and_the_guarded_rerun_equals_the_golden(hip_lib):
    cases.guard(hip_lib, "cuda")


def test_superglue_abi(hip_lib):
    cases.abi(hip_lib, "cuda")


def test_superglue_1100_by_900_decides_like_the_fp32_oracle(hip_lib):
    cases.big_pair_against_fp32_oracle(hip_lib, "cuda")


def test_superglue_at_the_shipped_yaml_keypoint_count(hip_lib):
    cases.shipped_yaml_size(hip_lib, "cuda")
