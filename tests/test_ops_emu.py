"""CPU: operator-level kernels on the test emulator vs torch / the oracle (bit-exact where integer)."""
import ctypes

import pytest
import torch

from tests import op_cases
from tests.op_cases import _ffn_fused_case, _ffn_ln_gelu_case, p  # noqa: F401  (tests/test_lightglue_gpu.py imports the two cases from here)


@pytest.mark.parametrize("radius", [0, 1, 2, 3, 4, 5, 6])
def test_simple_nms_bit_exact_with_ties_and_plateaus(emu_lib, radius):
    r = op_cases.nms_case(emu_lib, op_cases.nms_tie_map(radius), radius)   # 45 x 70: not multiples of the tile; includes the image border logic
    assert torch.equal(r.out, r.ref) and r.guard_ok


@pytest.mark.parametrize("radius", [1, 3, 4])
def test_simple_nms_64_tiles_bit_exact(emu_lib, radius):
    """The 64 x 64-tile variant (dim_tune_set key 7 = 2 forces it on any map size) on a map with partial tiles on both axes."""
    try:
        emu_lib.dim_tune_set(7, 2)
        r = op_cases.nms_case(emu_lib, op_cases.nms_partial_tile_map(radius), radius)
    finally:
        emu_lib.dim_tune_set(7, 1)
    assert torch.equal(r.out, r.ref) and r.guard_ok


@pytest.mark.parametrize("M,N,K,bt", [(200, 65, 64, 0), (130, 256, 256, 0), (150, 140, 64, 1), (1, 4, 32, 0)])
def test_gemm_mfma(emu_lib, M, N, K, bt):
    r = op_cases.gemm_f32_case(emu_lib, M, N, K, bt)
    assert r.abs_err.max() < 1e-4 and r.guard_ok


@pytest.mark.parametrize("cin,cout,H,W,pool", [(64, 64, 20, 37, 1), (64, 128, 9, 33, 0), (128, 128, 16, 34, 1)])
def test_conv3x3_mfma(emu_lib, cin, cout, H, W, pool):
    r = op_cases.conv3x3_case(emu_lib, cin, cout, H, W, pool)
    assert r.abs_err.max() < 1e-4 and r.guard_ok


@pytest.mark.parametrize("batch,H,W", [(2, 45, 70)])
def test_conv1a_vs_fp64(emu_lib, batch, H, W):
    """conv1a_kernel (1 -> 64 channels, direct VALU convolution; 64-pixel row segments, so W = 70 leaves a ragged second block) against fp64 conv2d + ReLU.
    Bound: an image in [0, 1] and weights of order 0.3 give sums of a few units; nine fmas and a bias add round at most ten times at <= 2^-22 each:
    1e-5 absolute is derived, not measured."""
    r = op_cases.conv1a_case(emu_lib, batch, H, W)
    assert r.abs_err.max() < 1e-5 and r.guard_ok


@pytest.fixture(params=[2, 1], ids=["fp16x3", "bf16x6"])
def split_mode(request, emu_lib):
    """Both split-precision modes of the matrix-core kernels (dim_tune_set key 1); the default is restored."""
    emu_lib.dim_tune_set(1, request.param)
    yield request.param
    emu_lib.dim_tune_set(1, 2)


@pytest.mark.parametrize("M,N,K", [(200, 65, 64), (130, 256, 512), (64, 130, 32)])
def test_gemm_split_precision_is_fp32_accurate(emu_lib, split_mode, M, N, K):
    """bf16x6 (exact 3-way bf16 split, six cross terms) and fp16x3 (2-way fp16 split of the scaled operands,
    three cross terms) on the 16-bit MFMA == fp32-class accuracy (vs fp64)."""
    r = op_cases.gemm_x6_case(emu_lib, M, N, K)
    assert r.rel_err < 4e-7 and r.guard_ok


@pytest.mark.parametrize("M,N,K", [(200, 65, 96), (200, 65, 128), (70, 130, 256), (70, 130, 512)])
def test_gemm_small_problem_kernels_are_fp32_accurate(emu_lib, M, N, K):
    """The four small-problem fp16x3 kernels of launch_gemm_x6 (at most 512 workgroups of 64 rows): K = 96 -> gemm_x6_kernel<2,32,1,4> (K % 128 != 0),
    K = 128 -> gemm_x6_small32_kc64_kernel<true> (run-time K), K = 256 / 512 -> its <true,256> / <true,512> instances; ragged in M and N."""
    r = op_cases.gemm_x6_case(emu_lib, M, N, K, act=1)
    assert r.rel_err < 4e-7 and r.guard_ok


@pytest.mark.parametrize("bias,residual", [(True, True), (False, False)])
def test_gemm_selu_epilogue(emu_lib, bias, residual):
    """act = 2 (SELU, what ALIKED uses) at (200, 65, 64): the pre-activation error bound times SELU's Lipschitz constant plus 4 ulp for expf (op_cases.selu_bound)."""
    r = op_cases.gemm_x6_case(emu_lib, 200, 65, 64, act=2, bias=bias, residual=residual)
    assert bool((r.abs_err <= op_cases.selu_bound(r.scale)).all()) and r.guard_ok
    assert bool((r.ref < 0).any()) and bool((r.ref > 0).any())          # both branches of the activation are exercised


@pytest.mark.parametrize("M,N,K", [(130, 256, 512), (200, 500, 64)])
def test_gemm_wide_blocks_are_bit_identical(emu_lib, M, N, K):
    """The 128 x 256 workgroup block of gemm_x6.hip (dim_tune_set key 6; 2 = forced whatever the problem size) accumulates
    every output in the same order as the 128 x 128 block."""
    outs = []
    try:
        for wide in (0, 2):
            emu_lib.dim_tune_set(6, wide)
            outs.append(op_cases.gemm_x6_case(emu_lib, M, N, K, act=1))
    finally:
        emu_lib.dim_tune_set(6, 1)
    assert torch.equal(outs[0].raws[0], outs[1].raws[0]) and outs[0].guard_ok and outs[1].guard_ok
    assert bool((outs[0].out != op_cases.SENTINEL).all())


@pytest.mark.parametrize("M,N,K", [(130, 256, 512), (200, 500, 64), (70, 128, 256)])
def test_gemm_streaming_k_loop_prototype_is_bit_identical(emu_research_lib, M, N, K):
    """Research build only (dim_tune_set key 14 = 63): the small-problem block with the barrier-free streaming K loop (activation fragments straight from
    global memory, register ring) — same pieces, same term order as the staged loop; measured slower on hardware (profiles/r05_ab_small_gemm_stream.jsonl)."""
    lib = emu_research_lib
    g = torch.Generator().manual_seed(K + M)
    A, W = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g).contiguous()
    bias, R = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    dev, npad = ctypes.c_void_p(), ctypes.c_int()
    assert lib.dim_x3_create(p(W), K, N, ctypes.byref(dev), ctypes.byref(npad)) == 0
    outs = []
    try:
        for kc in (0, 63):
            assert lib.dim_tune_set(14, kc) == 0
            C = torch.full((M, N), -3.0)
            assert lib.dim_op_gemm_x6_f32(p(A), K, dev, npad.value, p(bias), p(R), N, p(C), N, M, N, K, 1, None) == 0, lib.dim_last_error()
            outs.append(C)
    finally:
        lib.dim_tune_set(14, 0)
        lib.dim_x3_destroy(dev)
    assert torch.equal(outs[0], outs[1]) and (outs[0] != -3.0).all()


@pytest.mark.parametrize("cin,cout,H,W,pool", [(64, 64, 20, 37, 1), (64, 128, 9, 33, 0), (128, 128, 16, 34, 1)])
def test_conv3x3_split_precision_is_fp32_accurate(emu_lib, split_mode, cin, cout, H, W, pool):
    r = op_cases.conv3x3_case(emu_lib, cin, cout, H, W, pool, split=True)
    assert r.rel_err < 4e-7 and r.guard_ok


@pytest.mark.parametrize("mode", [2, 0], ids=["fp16x3", "fp32"])
@pytest.mark.parametrize("name", sorted(op_cases.NHWC_CONV_CASES))
def test_nhwc_conv_vs_fp64(emu_lib, name, mode):
    """nhwc_conv_kernel<MODE, NT> (ALIKE's encoder / XFeat's trunk) through dim_nhwc_conv_create + dim_op_nhwc_conv_f32: every operand form, both pools,
    1 .. 4 column tiles, full and partial 16 x 8 tiles, in both arithmetic forms (dim_tune_set key 1)."""
    try:
        emu_lib.dim_tune_set(1, mode)
        r_out, r_pool, N = op_cases.nhwc_conv_case(emu_lib, name)
    finally:
        emu_lib.dim_tune_set(1, 2)
    for r in (r_out, r_pool) if r_pool is not None else (r_out,):
        figure, bound = op_cases.nhwc_conv_figure(r, mode == 2)
        print(f"nhwc_conv {name} mode {mode}: figure {figure:.4g} bound {bound:.4g}")
        assert r.guard_ok
        assert bool((r.out[..., N:] == 0.0).all()), "a padding channel is not exactly zero"
        assert figure < bound


@pytest.mark.parametrize("regime", ["tiny", "large", "overflow"])
def test_fp16x3_range_behaviour(emu_lib, regime):
    """fp16x3's narrow exponent: activations are scaled by 16 and clamped to +-65504 before the split.
    tiny (1e-3): still ~1e-6-accurate relative to sum|a||b|; large (up to 4000): exact range; beyond 4094:
    saturates to a finite value (never inf/nan)."""
    emu_lib.dim_tune_set(1, 2)
    g = torch.Generator().manual_seed(3)
    M, N, K = 64, 64, 256
    scale = {"tiny": 1e-3, "large": 4000.0, "overflow": 1e6}[regime]
    A = (torch.rand(M, K, generator=g) * scale).contiguous()
    W = (torch.randn(K, N, generator=g) * 0.05).contiguous()
    C = torch.zeros(M, N)
    dev, npad = ctypes.c_void_p(), ctypes.c_int()
    assert emu_lib.dim_x3_create(p(W), K, N, ctypes.byref(dev), ctypes.byref(npad)) == 0
    assert emu_lib.dim_op_gemm_x6_f32(p(A), K, dev, npad.value, None, None, 0, p(C), N, M, N, K, 0, None) == 0
    emu_lib.dim_x3_destroy(dev)
    assert torch.isfinite(C).all()
    if regime != "overflow":
        ref, mag = A.double() @ W.double(), A.abs().double() @ W.abs().double()
        assert ((C.double() - ref).abs() / mag).max().item() < (2e-6 if regime == "tiny" else 4e-7)


@pytest.mark.parametrize("M,K", [(64, 512), (150, 512), (67, 256)])
def test_ffn_layernorm_gelu_fused_op_vs_fp64(emu_lib, M, K):
    """LightGlue's ffn.0 -> LayerNorm -> GELU as one kernel (64 x 512 blocks; ragged last block) against an fp64 evaluation."""
    C, ref = _ffn_ln_gelu_case(emu_lib, M, K, seed=M + K)
    assert (C.double() - ref).abs().max().item() < 5e-6


@pytest.mark.parametrize("M,K", [(64, 512), (150, 512), (67, 256)])
def test_ffn_fused_op_vs_fp64(emu_lib, M, K):
    """ffn.0 -> LayerNorm -> GELU -> ffn.3 + residual as one kernel (hidden tile register-resident; ragged last block) vs fp64."""
    C, ref = _ffn_fused_case(emu_lib, M, K, seed=M + K)
    assert (C.double() - ref).abs().max().item() < 1e-5


@pytest.mark.parametrize("M,N,K", [(150, 200, 256), (128, 128, 64), (37, 300, 256)])
def test_gemm_x6_nt_vs_fp64(emu_lib, M, N, K):
    """sim = A B^T with both operands split on the fly (gemm_x6_nt_kernel, LightGlue's similarity) vs fp64; ragged last blocks; a
    guard band around C stays untouched."""
    r = op_cases.gemm_x6_nt_case(emu_lib, M, N, K)
    assert r.rel_err < 5e-7
    assert r.guard_ok


@pytest.mark.parametrize("kf16,df16,dn", [(0, 0, 0), (1, 1, 1), (0, 1, 0), (1, 0, 1)])
def test_lg_stage_features_equals_the_host_conversion(emu_lib, kf16, df16, dn):
    """dim_lg_stage_features: one pair's arrays as features.h5 holds them (float16 or float32, descriptors (N, D) or (D, N)) -> the fp32 (N, D)
    feature table, bit for bit what featuresDict2Lightglue's host path produces (matchers/lightglue.py:38-43,62: transpose, torch.as_tensor(...,
    float32)); rows past the live count are zero; ragged counts incl. 0 and a count that is not a multiple of the 32-row block."""
    import importlib
    import numpy as np
    capi = importlib.import_module("deep-image-matching_amd.capi")
    g = np.random.default_rng(7 + kf16 + 2 * df16 + 4 * dn)
    D, cap = 128, 77
    for n0, n1 in ((77, 45), (0, 33), (64, 0)):
        arrs, descr, keep = [], [], []
        for n in (n0, n1):
            k = (g.random((n, 2)) * 1000).astype(np.float16 if kf16 else np.float32)
            d = g.standard_normal((D, n) if dn else (n, D)).astype(np.float16 if df16 else np.float32)
            kt, dt = torch.from_numpy(np.ascontiguousarray(k)), torch.from_numpy(np.ascontiguousarray(d))
            keep += [kt, dt]
            descr.append(capi.LgRawFeatures(kt.data_ptr(), dt.data_ptr(), n, kf16, df16, dn))
            arrs.append((k.astype(np.float32), (d.T if dn else d).astype(np.float32)))
        ktab, dtab = torch.full((2, cap, 2), -7.0), torch.full((2, cap, D), -7.0)
        assert emu_lib.dim_lg_stage_features(ctypes.byref(descr[0]), ctypes.byref(descr[1]), cap, D, p(ktab), p(dtab), None) == 0, emu_lib.dim_last_error()
        for i, n in enumerate((n0, n1)):
            assert np.array_equal(ktab[i, :n].numpy(), arrs[i][0]) and np.array_equal(dtab[i, :n].numpy(), arrs[i][1])
            assert not ktab[i, n:].any() and not dtab[i, n:].any()


# ---------------------------------------------------------------------------------------------------------------- keypoint selection, descriptor sampling
@pytest.mark.parametrize("case", op_cases.SELECT_CASES, ids=[c[0] for c in op_cases.SELECT_CASES])
def test_select_topk_exact(emu_lib, case):
    """dim_op_select_topk_f32 (count / scan / emit rows -> top-k -> zero fill of sp_post.hip) on crafted maps — ties at the k-th key, all scores
    equal, n = k - 1 / k / k + 1, the 4096 hand-over, mixed batches, the largest tables — bit for bit against op_cases.select_topk_reference."""
    op_cases.run_select_case(emu_lib, case).check()


def test_select_topk_reused_workspace_carries_no_stale_keys(emu_lib):
    for r in op_cases.select_reused_workspace_results(emu_lib):
        r.check()


def test_select_topk_zero_fill_beyond_the_map_is_an_error(emu_lib):
    rc, msg, bufs = op_cases.select_error_case(emu_lib)
    assert rc != 0 and "50" in msg and "4 x 5" in msg, (rc, msg)
    assert all(bool((t == op_cases.SENTINEL).all()) for t in bufs)          # nothing ran (SENTINEL == I32_SENTINEL as a number)


@pytest.mark.parametrize("fix_sampling", [0, 1])
@pytest.mark.parametrize("h,w,batch,capacity,n_kpts", op_cases.SAMPLE_CASES)
def test_sample_descriptors_vs_fp64(emu_lib, h, w, batch, capacity, n_kpts, fix_sampling):
    """sample_desc_kernel at the corner cells, the edges, an all-zero block and random positions, within 4 x the fp32 oracle's own error against fp64
    (op_cases.check_sample)."""
    op_cases.check_sample(op_cases.sample_descriptors_case(emu_lib, h, w, batch, capacity, n_kpts, fix_sampling))
