"""CPU: the open SuperPoint extractor (dim_spo_create: BatchNorm in the convolution epilogue of conv_x6.hip) compiled against the test-only
emulator, on the cases of tests/spopen_cases.py, plus the checks that fail before anything native runs."""
import importlib

import pytest

from tests import spopen_cases as cases


@pytest.mark.parametrize("name", ["keepall", "ragged_pipeline", "topk50", "threshold"])
def test_golden(emu_lib, name):
    cases.golden(emu_lib, "cpu", name)


def test_batch_of_three_and_one_handle_across_sizes(emu_lib):
    cases.batch_and_reuse(emu_lib, "cpu")


def test_range_guard_sees_negative_values_and_the_fallback_meets_the_bounds(emu_lib):
    cases.range_guard(emu_lib, "cpu")


def test_loader_validation_names_the_tensor(tmp_path):
    cases.loader_validation(tmp_path)


def test_extractor_plugin_feeds_the_nearest_neighbour_matcher(emu_install, tmp_path):
    cases.extractor_matcher_chain(importlib.import_module("deep-image-matching_amd.plugins"), tmp_path)


def test_unsupported_arithmetic_and_unfused_conv1a_are_clear_errors(emu_lib):
    capi = importlib.import_module("deep-image-matching_amd.capi")
    case = cases.CASES["keepall"]
    with pytest.raises(ValueError, match="fp16x3 / bf16x6"):
        cases.make_net(emu_lib, "cpu", case, arithmetic="fp32")
    net = cases.make_net(emu_lib, "cpu", case)
    x = cases.image(case)[0].contiguous()
    for key, off, on in ((1, 0, 2), (3, 0, 1)):          # precision mode 0 (fp32 MFMA), conv1a as its own kernel
        try:
            emu_lib.dim_tune_set(key, off)
            with pytest.raises(capi.DimHipError, match="open-SuperPoint handle"):
                net.extract_batch(x)
        finally:
            emu_lib.dim_tune_set(key, on)
    assert net.extract_batch(x)[3].item() == cases.gold("keepall")["keypoints"].shape[0]


def test_bf16x6_and_unsplit_activation_storage_agree_with_the_default(emu_lib):
    """The same epilogue in precision mode 1 (what the guard's fallback runs) and in fp16x3 with fp32 activation storage (dim_tune_set key 5 = 0:
    launch_conv3x3_x6's instantiations): keypoints identical, values at the golden's bounds."""
    case = cases.CASES["ragged_pipeline"]
    net = cases.make_net(emu_lib, "cpu", case)
    for key, v, back in ((1, 1, 2), (5, 0, 1)):
        try:
            emu_lib.dim_tune_set(key, v)
            out, sat, _ = cases.run_counted(net, cases.image(case))
        finally:
            emu_lib.dim_tune_set(key, back)
        assert sat == 0
        cases.check_against_golden(net, out, "ragged_pipeline", f"ragged_pipeline_cpu_key{key}={v}")
