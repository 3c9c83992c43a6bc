"""CPU: the HIP NetVLAD sources on the test emulator against the reference module's goldens and fp64 (cases in tests/netvlad_cases.py), the .mat
loader, and the checks that fail before anything native runs.

The golden cases "blocks" (208 x 272) and "photo" (112 x 160) run on the GPU only: the emulator steps through every MFMA of thirteen VGG16 layers
lane by lane, which takes minutes at those sizes; "blocks"' property (more than one workgroup of locations, a ragged last sub-block) is covered
here by the head operator at n = 221."""
import importlib

import pytest
import torch

from tests import netvlad_cases as cases

weights = importlib.import_module("deep-image-matching_amd.weights")
nv_mod = importlib.import_module("deep-image-matching_amd.netvlad_hip")
capi = importlib.import_module("deep-image-matching_amd.capi")


@pytest.mark.parametrize("name", ["min", "odd", "smallk"])
def test_netvlad_golden(emu_lib, name):
    cases.golden(emu_lib, "cpu", name)


@pytest.mark.parametrize("n,batch", [(1, 1), (54, 1), (221, 1), (54, 3)])
def test_netvlad_head_operator_against_fp64(emu_lib, n, batch):
    cases.head_op(emu_lib, "cpu", n, batch)


def test_netvlad_head_operator_small_k(emu_lib):
    cases.head_op(emu_lib, "cpu", 54, 1, K=8)


@pytest.mark.parametrize("batch", [1, 3])
def test_netvlad_whitening_operator_against_fp64(emu_lib, batch):
    cases.whiten_op(emu_lib, "cpu", batch)


def test_netvlad_mat_file_round_trips(tmp_path):
    from scipy.io import savemat

    sd = cases.weights(8, 256)
    path = tmp_path / "net.mat"
    savemat(str(path), weights.netvlad_state_to_mat(sd), do_compression=False)
    back = weights.load_netvlad_mat(path)
    assert set(back) == set(sd)
    for k in sd:
        assert torch.equal(back[k], sd[k]), k
    plain = weights.load_netvlad_mat(path, whiten=False)
    assert set(plain) == {k for k in sd if not k.startswith("whiten.")}


def test_netvlad_state_is_validated_before_any_native_call(tmp_path):
    from scipy.io import savemat

    good = cases.weights(64, None)
    sd = dict(good)
    sd["netvlad.score_proj.weight"] = sd["netvlad.score_proj.weight"][:63]          # a 63-cluster score matrix
    with pytest.raises(ValueError, match="netvlad.score_proj.weight"):
        weights.validate_netvlad_state(sd)
    with pytest.raises(ValueError, match="netvlad.score_proj.weight"):
        nv_mod.NetVLADHIP(sd, {"whiten": False}, device="cpu", lib=object())         # raised before the library is touched
    sd = dict(good)
    sd["netvlad.centers"] = sd["netvlad.centers"][:, :63]
    with pytest.raises(ValueError, match="netvlad.centers"):
        weights.validate_netvlad_state(sd)
    sd = dict(good)
    sd["backbone.17.weight"] = sd["backbone.17.weight"][:, :200]                    # a truncated convolution
    with pytest.raises(ValueError, match="backbone.17.weight"):
        weights.validate_netvlad_state(sd)
    small = dict(cases.weights(8, 256))
    small["whiten.weight"] = small["whiten.weight"][:, :4095]                        # a whitening one column short (K = 8: 4096 columns)
    with pytest.raises(ValueError, match="whiten.weight"):
        weights.validate_netvlad_state(small)
    sd = dict(good)
    del sd["backbone.28.bias"]
    with pytest.raises(KeyError, match="backbone.28.bias"):
        weights.validate_netvlad_state(sd)
    with pytest.raises(KeyError, match="whiten.weight"):
        nv_mod.NetVLADHIP(good, {"whiten": True}, device="cpu", lib=object())
    # the same checks on a file: the loader names the tensor
    bad = dict(cases.weights(8, 256))
    bad["backbone.5.weight"] = bad["backbone.5.weight"][:, :, :2]
    savemat(str(tmp_path / "bad.mat"), weights.netvlad_state_to_mat(bad), do_compression=False)
    with pytest.raises(ValueError, match="backbone.5.weight"):
        weights.load_netvlad_mat(tmp_path / "bad.mat")


def test_netvlad_whitening_with_32767_columns_is_rejected():
    sd = {k: v for k, v in cases.weights(64, None).items()}
    sd["whiten.weight"] = torch.zeros(16, 32767)
    sd["whiten.bias"] = torch.zeros(16)
    with pytest.raises(ValueError, match="whiten.weight"):
        weights.validate_netvlad_state(sd)


def test_netvlad_create_and_extract_reject_bad_arguments(emu_lib):
    sd = cases.weights(8, 256)
    with pytest.raises(capi.DimHipError, match="max_h 8"):
        nv_mod.NetVLADHIP(sd, {}, max_hw=(8, 64), device="cpu", lib=emu_lib)
    net = nv_mod.NetVLADHIP(sd, {}, max_hw=(16, 32), device="cpu", lib=emu_lib)
    with pytest.raises(capi.DimHipError, match="image 32x32"):
        net.extract_batch(torch.zeros(1, 32, 32, 3))
    with pytest.raises(capi.DimHipError, match="batch 2"):
        net.extract_batch(torch.zeros(2, 16, 16, 3))
    with pytest.raises(capi.DimHipError, match="clusters"):
        nv_mod.netvlad_head(torch.zeros(1, 4, 512), torch.zeros(12, 512), torch.zeros(512, 12), lib=emu_lib)
    with pytest.raises(capi.DimHipError, match="in_dim 1000"):
        nv_mod.netvlad_whiten(torch.zeros(1, 1000), torch.zeros(4, 1000), torch.zeros(4), lib=emu_lib)


def test_netvlad_range_guard_fires_and_the_guarded_rerun_is_clean(emu_lib):
    cases.guard(emu_lib, "cpu")


def test_retrieval_pair_selector_downsamples_above_1024(emu_lib):
    cases.selector_resize(emu_lib, "cpu")


def test_netvlad_create_refuses_an_image_size_it_could_not_run(emu_lib):
    with pytest.raises(capi.DimHipError, match="2 GiB"):
        nv_mod.NetVLADHIP(cases.weights(8, 256), {}, max_hw=(2048, 4096), device="cpu", lib=emu_lib)


def test_retrieval_oracle_applies_both_cuts():
    """tests/netvlad_cases.pairs_from_descriptors on hand-made descriptors: top-k, the min_score cut at 0, duplicates."""
    import numpy as np
    d = np.array([[1.0, 0.0], [0.8, 0.6], [0.6, 0.8], [-1.0, 0.0], [0.0, -1.0]])
    names = list("abcde")
    pairs, _ = cases.pairs_from_descriptors(names, d, 2, 0.0)
    # b and c only repeat pairs that are out already; d keeps e alone (0 is not below the cut, its other similarities are negative); e keeps a (0) and
    # repeats d
    assert pairs == [("a", "b"), ("a", "c"), ("b", "c"), ("d", "e"), ("e", "a")]
    everything, _ = cases.pairs_from_descriptors(names, d, 2, None)
    assert ("d", "c") in everything and ("d", "c") not in pairs   # without the cut d's second neighbour (-0.6) comes out


def test_retrieval_pair_selector_batches_mixed_sizes_and_keeps_list_order(emu_lib):
    cases.describe_mixed(emu_lib, "cpu", n=3)   # three images here: the emulator takes seconds per extraction
