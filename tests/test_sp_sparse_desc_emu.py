"""CPU: SuperPoint's sparse descriptor head (convDa / convDb on the cells that keypoints sample; dim_tune_set key 20) compiled against the
test-only emulator, on the cases of tests/sp_sparse_desc_cases.py: bit-identical to the dense head, row counts, range guard, oracle."""
import pytest

from tests import sp_sparse_desc_cases as cases


@pytest.mark.parametrize("fix_sampling", [0, 1])
def test_ragged_batch_with_edge_keypoints_and_an_image_without_any(emu_lib, fix_sampling):
    cases.ragged_batch(emu_lib, "cpu", fix_sampling)


@pytest.mark.parametrize("capacity", [64, 512])
@pytest.mark.parametrize("open_net", [False, True])
def test_selection_rule_and_both_kinds_of_handle(emu_lib, open_net, capacity):
    cases.selection_rule(emu_lib, "cpu", open_net, capacity)


def test_keypoints_clustered_on_a_few_cells(emu_lib):
    cases.cluster(emu_lib, "cpu")
