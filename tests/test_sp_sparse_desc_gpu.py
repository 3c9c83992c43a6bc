"""GPU (MI355X): SuperPoint's sparse descriptor head (convDa / convDb on the cells that keypoints sample; dim_tune_set key 20) on the cases of
tests/sp_sparse_desc_cases.py: bit-identical to the dense head, row counts, range guard, oracle."""
import pytest

from tests import sp_sparse_desc_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fix_sampling", [0, 1])
def test_ragged_batch_with_edge_keypoints_and_an_image_without_any(hip_lib, fix_sampling):
    cases.ragged_batch(hip_lib, "cuda", fix_sampling)


@pytest.mark.parametrize("capacity", [64, 512])
@pytest.mark.parametrize("open_net", [False, True])
def test_selection_rule_and_both_kinds_of_handle(hip_lib, open_net, capacity):
    cases.selection_rule(hip_lib, "cuda", open_net, capacity)


def test_keypoints_clustered_on_a_few_cells(hip_lib):
    cases.cluster(hip_lib, "cuda")
