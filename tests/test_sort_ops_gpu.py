"""GPU: csrc/sort_ops.hip on hardware — the three tests of tests/test_sort_ops_emu.py with the same parametrisations and the same bit-exact comparisons
against numpy / torch, plus two cases that span many workgroups of the compact -> chunk-sort -> merge chain (25 chunks of 4096 keys, five merge passes
with an odd run in the first).  Every case runs twice and must give the same bits: so_compact_kernel orders its output by an atomic counter, so on
hardware the order in which the keys reach the sort differs from run to run (on the emulator it never does), and the result must not."""
import pytest

from tests import test_sort_ops_emu as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,T", [(300, 6), (4096, 16), (9001, 12), (70001, 20)])
def test_group_by_tile_is_the_boolean_mask_order(hip_lib, n, T):
    cases.check_group_by_tile(hip_lib, n, T, device="cuda", runs=2)


@pytest.mark.parametrize("n_live,n_dead,n_slots", [(50, 10, 1), (4096, 0, 3), (5000, 7000, 4), (13000, 100, 5), (0, 64, 2), (70000, 30000, 7)])
def test_unique_match_rows_is_np_unique_per_image_pair(hip_lib, n_live, n_dead, n_slots):
    cases.check_unique_match_rows(hip_lib, n_live, n_dead, n_slots, device="cuda", runs=2)


def test_tile_match_keys(hip_lib):
    cases.check_tile_match_keys(hip_lib, device="cuda")
