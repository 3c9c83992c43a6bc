"""MI355X: the gfx950 NetVLAD kernels against the reference module's goldens and fp64 (cases in tests/netvlad_cases.py)."""
import pytest

from tests import netvlad_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(cases.GOLDEN_CASES))
def test_netvlad_golden(hip_lib, name):
    cases.golden(hip_lib, "cuda", name)


@pytest.mark.parametrize("n,batch", [(1, 1), (54, 1), (221, 1), (54, 3)])
def test_netvlad_head_operator_against_fp64(hip_lib, n, batch):
    cases.head_op(hip_lib, "cuda", n, batch)


def test_netvlad_head_operator_small_k(hip_lib):
    cases.head_op(hip_lib, "cuda", 54, 1, K=8)


@pytest.mark.parametrize("batch", [1, 3, 16, 17])
def test_netvlad_whitening_operator_against_fp64(hip_lib, batch):
    cases.whiten_op(hip_lib, "cuda", batch)


def test_netvlad_batch_is_bit_identical_and_handles_can_be_reused(hip_lib):
    cases.batch_and_reuse(hip_lib, "cuda")


def test_netvlad_without_whitening_equals_the_head_operator(hip_lib):
    cases.no_whiten_equals_head(hip_lib, "cuda")


def test_retrieval_pair_selector_equals_the_reference_list(hip_lib):
    cases.selector(hip_lib, "cuda")


def test_netvlad_range_guard_fires_and_the_guarded_rerun_is_clean(hip_lib):
    cases.guard(hip_lib, "cuda", nan_pixel=True)


def test_retrieval_pair_selector_downsamples_above_1024(hip_lib):
    cases.selector_resize(hip_lib, "cuda")


def test_retrieval_pair_selector_batches_mixed_sizes_and_keeps_list_order(hip_lib):
    cases.describe_mixed(hip_lib, "cuda")
