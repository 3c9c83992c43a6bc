"""MI355X: the gfx950 LighterGlue kernels (width 96, one head) against the reference module's goldens and the oracle (cases in
tests/lighterglue_cases.py)."""
import pytest

from tests import lighterglue_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(cases.GOLDEN_CASES))
def test_lighterglue_golden(hip_lib, name):
    cases.golden(hip_lib, "cuda", name)


def test_lighterglue_edge_counts(hip_lib):
    cases.edge_counts(hip_lib, "cuda")


def test_lighterglue_batch_equals_singles_and_handles_can_be_reused(hip_lib):
    cases.batch_equals_singles(hip_lib, "cuda")


def test_lighterglue_range_guard_fires_and_the_guarded_rerun_equals_the_golden(hip_lib):
    cases.guard(hip_lib, "cuda")


def test_lighterglue_attention_undamped_against_fp64(hip_lib):
    cases.attention_undamped(hip_lib, "cuda")


def test_lighterglue_adaptive_depth_on_a_96_wide_handle(hip_lib):
    cases.adaptive_depth(hip_lib, "cuda")


def test_lighterglue_plugin_hands_the_network_w_h_on_the_staged_path(hip_lib, monkeypatch):
    mt, got, *_ = cases.plugin_size_table(monkeypatch, {"name": "lighterglue", "allow_synthetic_weights": True, "pruning_min_kpts": -1})
    assert got.dtype.name == "int32" and got.shape[0] > 10 and str(mt._net.device).startswith("cuda")


def test_lighterglue_abi(hip_lib):
    cases.abi(hip_lib, "cuda")


def test_xfeat_feeds_lighterglue(hip_lib):
    cases.chain(hip_lib, "cuda")
