"""GPU: the operator-level entry points (dim_op_* of include/dim_hip.h) of the matrix-core, convolution, NMS, keypoint-selection and descriptor-sampling
kernels ON HARDWARE against fp64 (NMS and selection: bit-exact against the oracle / the stated rule), through the builders of tests/op_cases.py that the
emulator tests use.

The emulator has no memory model, no caches and no timing: workgroups run one after another and fibers in a fixed order between barriers.  A missing
barrier around an LDS restage or a missing wait after an LDS-DMA is invisible there and shows on hardware only when two workgroups share a CU (the
recorded case: test_lightglue_gpu.test_ffn_layernorm_gelu_fused_op_at_production_rows).  So every kernel gets
  * a small ragged shape (partial last blocks on every axis), and
  * an occupancy shape: the smallest one with >= 512 workgroups (two per CU on 256 CUs) that still has a ragged tail, with K small so that the fp64
    reference stays around a second;
every case runs TWICE on the same inputs and must give the same bits, stay within the bound the emulator test asserts for the operator, and leave the
guard band around its output (op_cases.py) untouched.

Case -> kernel (from launch_gemm / launch_gemm_x6 / launch_gemm_x6_nt / launch_conv3x3 / launch_conv3x3_x6 / launch_conv1a / launch_nhwc_conv / launch_nms; wg = workgroups):

  test_gemm_f32                (200,65,64) (130,256,256) (1,4,32)           gemm_mfma_kernel<0>          4 / 4 / 1 wg
                               (150,140,64) b_is_nk                         gemm_mfma_kernel<1>          4 wg
                               (65573,128,64), and b_is_nk                  gemm_mfma_kernel<0> / <1>    513 wg
  test_gemm_x6_fp16x3          (4101,768,256)                               gemm_x6_small32_kc64_kernel<true,256>    129 x 6 = 774 wg
                               (4101,768,512)                               gemm_x6_small32_kc64_kernel<true,512>    774 wg
                               (4101,768,128)                               gemm_x6_small32_kc64_kernel<true,0>      774 wg
                               (4101,768,96)                                gemm_x6_kernel<2,32,1,4>                 774 wg
                               (65573,65,256)   n_pad 128: never wide       gemm_x6_kernel<2,128,2,2>                513 wg
                               (200,65,64) (64,130,32)                      gemm_x6_kernel<2,32,1,4>                 7 / 4 wg
                               (130,256,512)                                gemm_x6_small32_kc64_kernel<true,512>    10 wg
  test_gemm_x6_large_blocks    (32805,256,64)  key 6 = 0                    gemm_x6_kernel<2,128,2,2>                257 x 2 = 514 wg
                                               key 6 = 2 (forced)           gemm_x6_kernel<2,128,2,4>                257 wg
                               (65573,256,64)  key 6 = 1 (natural: 513 >= 512 wide blocks)  gemm_x6_kernel<2,128,2,4>   513 wg
                                               key 6 = 0                    gemm_x6_kernel<2,128,2,2>                1026 wg
  test_gemm_x6_bf16x6          (200,65,64)                                  gemm_x6_kernel<1,64,2,2>                 4 wg
                               (65573,128,64)                               gemm_x6_kernel<1,128,2,2>                513 wg
  test_gemm_x6_nt              (150,200,256) (128,128,64) (37,300,256)      gemm_x6_nt_kernel<2> / <1>               4 / 1 / 3 wg
                               (2085,4101,64)                               gemm_x6_nt_kernel<2> / <1>               17 x 33 = 561 wg
  test_conv3x3_f32             three small shapes, batch 2, key 0 = 1..4    conv3x3_mfma_kernel<cin,pool,8,0,3> / <..,8,1,2> / <..,8,1,3> / <..,16,0,1>
                               64 -> 256 130 x 250, 128 -> 128 130 x 490 (pool 0 / 1), key 0 = 3      conv3x3_mfma_kernel<cin,pool,8,1,3>   544 wg
  test_conv3x3_x6_fp16x3       the same seven shapes                        conv3x3_x6_kernel<cin,pool,1,false,2,false,false>
  test_conv3x3_x6_bf16x6       the same seven shapes, key 2 = 0 / 1 / 2     conv3x3_x6_kernel<cin,pool,0 / 1 / 2,false,1,false,false>
  test_conv1a                  (2,45,70) / (2,130,150)                      conv1a_kernel                180 / 780 wg
  test_nhwc_conv               batch 2, key 1 = 2 / 0 -> MODE 2 (fp16x3) / 0 (fp32); op_cases.NHWC_CONV_CASES:
                               A 3x3 16 -> 16 9x17, B 3x3 img3 13x19 in a 32x32 frame -> 8 pool 2     nhwc_conv_kernel<MODE,1>     8 / 16 wg
                               C 3x3 32 (+ in2 16) -> 48 12x20 pool 4, F 1x1 unfold8 24x40 -> 64 3x5  nhwc_conv_kernel<MODE,2>     8 / 2 wg
                               D 1x1 48 -> 96 5x7 no ReLU                                              nhwc_conv_kernel<MODE,3>     2 wg
                               E 3x3 stride 2 32 -> 128 11x23 -> 6x12                                  nhwc_conv_kernel<MODE,4>     2 wg
  test_nms_small_maps          radius 0: nms_kernel<0,32,512,8>; 2: <2,32,..>; 5, 6: <5|6,16,512,8>; radius 1, 3, 4: key 7 = 0 nms_kernel<r,32,512,8>,
                               key 7 = 2 nms_kernel<1,64,1024,8> / <3,64,1024,10> / <4,64,1024,12>
  test_nms_large_map           4 x 500 x 500, 8 * 8 * 4 = 256 tiles: the 64-tile kernels by themselves under key 7 = 1, the 32-tile ones under key 7 = 0

  test_select_topk (sp_post.hip; per image: count_rows / emit_rows cdiv(H,4) wg of 4 waves, scan_rows 1 wg, topk_zero_fill 1 wg; the top-k form below)
    equal  1x72x100, k 300 / 4096             topk_kernel, the radix select walks all 8 key bytes                      1 wg
                     k 4097 / 5000            topk_select_big -> topk_chunk_sort -> topk_merge                         1 + 2 + 32 wg
    ties   1x100x132 (6 levels), k 1000 / 4096            topk_kernel, k-th key inside a tie group                     1 wg
                     k 4097 / 8192 / 8193     the chunked form, 2 / 2 / 3 chunks                                       1 + 2|3 + 32|48 wg
    n_near_k 1x96x128, k = n-1, n, n+1        topk_kernel: select / keep-all / sort-everything (+ zero fill of 1)      1 wg
    handover 1x80x100, k 4095 / 4096 / 4097   topk_kernel | the chunked form, n ~ 4800                                 1 | 1 + 2 + 32 wg
    mixed  5x90x124 (empty, sparse, dense, 4 levels, one pixel), k 500 / 4096 / 6000     per-image early returns       5 | 5 + 10 + 160 wg
    keep_all 2x50x70, k -1, capacity 1000 / 4096          topk_keep_all, truncated and not                             2 wg
    wide1300 / wide1301 / w260                count_rows / emit_rows: float4 loop second step, scalar loop, 2nd group  2 / 2 / 20 wg
    tall   2x1030x8                           scan_rows_kernel with two rows per thread                                258 x 2 / 2 wg
    thr_dev 3x60x84                           per-image device thresholds 0.2 / 0.9 / 2.0                              15 x 3 wg
    border_removes_all 1x20x30                topk_zero_fill fills all of k = 50                                       1 wg
    big    1x200x200, k 20000 / 32768         the chunked form at 5 / 8 chunks                                         1 + 5|8 + 80|128 wg
    occupancy 128x64x96 k 1000                topk_kernel x 128, count / emit 16 x 128 = 2048 wg, zero_fill 128 wg
              16x100x132 k 5000               the chunked form: 16 + 2 x 16 + 32 x 16 = 560 wg, count / emit 25 x 16 wg
  test_select_topk_reused_workspace           three calls on one workspace: chunked (2 chunks) -> chunked, sparse + fill -> topk_kernel
  test_sample_descriptors                     sample_desc_kernel, one wave per keypoint: 5x7 (16 x 3 wg), 12x20 (75 x 2 wg), 128x128 (512 x 2 = 1024 wg)

  tests/test_attention_ops_gpu.py (dim_op_lg_attention_f32 / dim_op_lg_qkv_attention_f32; MODE 2 = fp16x3, 1 = bf16x6; wg of the attention kernel, surplus
  workgroups of its XCD-rounded 1-D grid included; the full table with the merge kernels' grids is in that file's docstring)
    small_ragged (A)  2 items, n (70, 130)          attn_kernel 16 wg | kv_prep_kernel<MODE> + attn_x6_kernel<MODE> 16 wg, 64 wg + attn_combine_kernel<4> |
                                                   kv_prep96_kernel<MODE> + attn_d96_kernel<MODE> 16 wg, 64 wg + attn_combine96_kernel
    edge_counts (B)   8 items, nsel 200 < nmax 224  attn_kernel 64 wg | attn_x6_kernel<MODE> 256 wg + attn_combine_kernel<4>, 64 wg | attn_d96_kernel<MODE> 64 wg + combine96, 16 wg
    neighbours (C)    2 | 6 items, four parts       attn_x6_kernel<MODE> 64 | 192 wg, attn_d96_kernel<MODE> 64 | 64 wg
    fused (D)         2 items, nsel 130             gemm_x6_qkv_small_kernel<64,true,256> 60 | 40 wg + attn_x6_kernel<2> with kv_ready
    two_parts (E)     64 items, nsel 100            attn_x6_kernel<MODE> 512 wg + attn_combine_kernel<2>
    many_resident     256: 64 x 260 768 wg (1 part), 32 x 260 768 wg (2 parts), 20 x 260 960 wg (4 parts); 96: 64 x 400 512 wg (2 parts), 128 x 520 640 wg (1 part)

  tests/test_lg_head_ops_gpu.py (dim_op_lg_confidence_f32 / dim_op_lg_decide / dim_op_lg_prune / dim_op_lg_assign_f32 / dim_op_lg_finalize; widths 256 and 96)
    assign            nmax 132: lg_row_stats4<8> + lg_col_stats4 + lg_row_argmax4<8> + lg_col_argmax4; nmax 2052: the <16> forms; nmax 134: the generic four;
                      flat / planted / ramp / ties / dead entries 1e30 / pairs the tag does not select
    many_resident     16 pairs x 260 ragged (0, 1 and nmax among the counts): assign 2080 + 80 + 1040 + 80 wg, prune 32 + 2080 + 2080 wg; a pair alone and among 16
    finalize          5 pairs, nmax 1032 (two rows per thread), out_cap 50 / 1032, done > 0 / 0 / < 0, prune on / off      lg_finalize_kernel 5 wg of 16 waves
    prune             6 pairs, nmax 1032, two rounds            lg_prune_scan 12 wg, gather / copyback 258 x 12 wg (lgl_prune_* at width 96), commit 1 wg
    confidence        n = 1, 31, 32, 33, 130, 64, 50, 50        lg_confidence_kernel / lgl_confidence_kernel 5 x 8 wg;   decide: lg_decide_kernel 1 wg

launch_gemm_x6's gemm_x6_kernel<2,64,2,2> branch is not in the table: a small problem has cdiv(M,128) * cdiv(N,128) < 256 workgroups, so at most
2 * 255 = 510 workgroups of 64 rows, which is never above the 512 that the branch before it accepts.
"""
import contextlib

import pytest
import torch

from tests import op_cases
from tests.test_aliked_gpu import _record   # appends one JSON line to the measured-parity log

pytestmark = pytest.mark.gpu

DEV = "cuda"
TUNE_DEFAULTS = {0: 3, 1: 2, 2: 17, 6: 1, 7: 1}


@contextlib.contextmanager
def tuned(lib, keys):
    """dim_tune_set(key, value) for the duration of a case; the defaults come back whatever happens."""
    try:
        for k, v in keys.items():
            assert lib.dim_tune_set(k, v) == 0, lib.dim_last_error()
        yield
    finally:
        for k in keys:
            lib.dim_tune_set(k, TUNE_DEFAULTS[k])


def check(r, figure, bound):
    """Same bits run to run, an intact guard band, and the accuracy figure (printed before it is asserted) within the bound."""
    print(f"figure {figure:.4g} bound {bound:.4g} repeatable {r.repeatable} guard_ok {r.guard_ok}")
    assert r.repeatable, "two runs on the same inputs differ"
    assert r.guard_ok, "the guard band around the output was written"
    assert figure < bound


def check_gemm_x6(r, act):
    if act == 2:   # SELU: elementwise (op_cases.selu_bound); the figure is the largest ratio to it
        check(r, (r.abs_err / op_cases.selu_bound(r.scale)).max().item(), 1.0 + 1e-12)
        assert bool((r.ref < 0).any()) and bool((r.ref > 0).any())
    else:
        check(r, r.rel_err, 4e-7)


# ---------------------------------------------------------------------------------------------------------------- GEMM
@pytest.mark.parametrize("M,N,K,bt", [(200, 65, 64, 0), (130, 256, 256, 0), (150, 140, 64, 1), (1, 4, 32, 0), (65573, 128, 64, 0), (65573, 128, 64, 1)])
def test_gemm_f32(hip_lib, M, N, K, bt):
    r = op_cases.gemm_f32_case(hip_lib, M, N, K, bt, device=DEV, runs=2)
    check(r, r.abs_err.max().item(), 1e-4)


@pytest.mark.parametrize("M,N,K,act,bias,residual", [
    (4101, 768, 256, 0, True, True),
    (4101, 768, 512, 1, True, False),
    (4101, 768, 128, 2, False, True),
    (4101, 768, 96, 1, False, False),
    (65573, 65, 256, 2, True, False),
    (200, 65, 64, 0, True, True),
    (200, 65, 64, 2, True, True),
    (130, 256, 512, 0, True, True),
    (64, 130, 32, 0, True, True),
])
def test_gemm_x6_fp16x3(hip_lib, M, N, K, act, bias, residual):
    r = op_cases.gemm_x6_case(hip_lib, M, N, K, act=act, bias=bias, residual=residual, device=DEV, runs=2)
    check_gemm_x6(r, act)


@pytest.mark.parametrize("M,N,K,key6,other", [(32805, 256, 64, 0, 2), (65573, 256, 64, 1, 0)])
def test_gemm_x6_large_blocks(hip_lib, M, N, K, key6, other):
    """The large-problem 128 x 128 and 128 x 256 blocks at two workgroups per CU, and the same shape forced to the other block: bit-identical (the hardware
    counterpart of test_ops_emu.test_gemm_wide_blocks_are_bit_identical)."""
    with tuned(hip_lib, {6: key6}):
        r = op_cases.gemm_x6_case(hip_lib, M, N, K, act=1, device=DEV, runs=2)
    with tuned(hip_lib, {6: other}):
        o = op_cases.gemm_x6_case(hip_lib, M, N, K, act=1, device=DEV, runs=1)
    check_gemm_x6(r, 1)
    check_gemm_x6(o, 1)
    assert torch.equal(r.raws[0], o.raws[0]), "the 128 x 128 and the 128 x 256 block differ"


@pytest.mark.parametrize("M,N,K", [(200, 65, 64), (65573, 128, 64)])
def test_gemm_x6_bf16x6(hip_lib, M, N, K):
    with tuned(hip_lib, {1: 1}):
        r = op_cases.gemm_x6_case(hip_lib, M, N, K, device=DEV, runs=2)
    check_gemm_x6(r, 0)


@pytest.mark.parametrize("mode", [2, 1], ids=["fp16x3", "bf16x6"])
@pytest.mark.parametrize("M,N,K", [(150, 200, 256), (128, 128, 64), (37, 300, 256), (2085, 4101, 64)])
def test_gemm_x6_nt(hip_lib, M, N, K, mode):
    with tuned(hip_lib, {1: mode}):
        r = op_cases.gemm_x6_nt_case(hip_lib, M, N, K, device=DEV, runs=2)
    check(r, r.rel_err, 5e-7)


# ---------------------------------------------------------------------------------------------------------------- convolutions
SMALL_CONV = [(64, 64, 20, 37, 1, 2), (64, 128, 9, 33, 0, 2), (128, 128, 16, 34, 1, 2)]                                # (cin, cout, H, W, pool, batch): the emulator's shapes
BIG_CONV = [(64, 256, 130, 250, 0, 1), (64, 256, 130, 250, 1, 1), (128, 128, 130, 490, 0, 1), (128, 128, 130, 490, 1, 1)]  # cdiv(W,32) * cdiv(H,8) * cout/64 = 544 workgroups
# (shape-major order everywhere below: consecutive cases share one cached fp64 reference)


@pytest.mark.parametrize("shape,variant", [(s, v) for s in SMALL_CONV for v in (1, 2, 3, 4)] + [(s, 3) for s in BIG_CONV])
def test_conv3x3_f32(hip_lib, shape, variant):
    cin, cout, H, W, pool, batch = shape
    with tuned(hip_lib, {0: variant}):
        r = op_cases.conv3x3_case(hip_lib, cin, cout, H, W, pool, batch=batch, device=DEV, runs=2)
    check(r, r.abs_err.max().item(), 1e-4)


@pytest.mark.parametrize("shape", SMALL_CONV + BIG_CONV)
def test_conv3x3_x6_fp16x3(hip_lib, shape):
    cin, cout, H, W, pool, batch = shape
    r = op_cases.conv3x3_case(hip_lib, cin, cout, H, W, pool, batch=batch, split=True, device=DEV, runs=2)
    check(r, r.rel_err, 4e-7)


@pytest.mark.parametrize("shape,prefetch", [(s, v) for s in SMALL_CONV + BIG_CONV for v in (0, 1, 2)])
def test_conv3x3_x6_bf16x6(hip_lib, shape, prefetch):
    cin, cout, H, W, pool, batch = shape
    with tuned(hip_lib, {1: 1, 2: prefetch}):
        r = op_cases.conv3x3_case(hip_lib, cin, cout, H, W, pool, batch=batch, split=True, device=DEV, runs=2)
    check(r, r.rel_err, 4e-7)


@pytest.mark.parametrize("batch,H,W", [(2, 45, 70), (2, 130, 150)])
def test_conv1a(hip_lib, batch, H, W):
    """1e-5 absolute: derived in test_ops_emu.test_conv1a_vs_fp64 (nine fmas and a bias on an image in [0, 1], weights of order 0.3)."""
    r = op_cases.conv1a_case(hip_lib, batch, H, W, device=DEV, runs=2)
    check(r, r.abs_err.max().item(), 1e-5)


@pytest.mark.parametrize("name,mode", [(n, m) for n in sorted(op_cases.NHWC_CONV_CASES) for m in (2, 0)])
def test_nhwc_conv(hip_lib, name, mode):
    with tuned(hip_lib, {1: mode}):
        r_out, r_pool, N = op_cases.nhwc_conv_case(hip_lib, name, device=DEV, runs=2)
    for r in (r_out, r_pool) if r_pool is not None else (r_out,):
        check(r, *op_cases.nhwc_conv_figure(r, mode == 2))
        assert bool((r.out[..., N:] == 0.0).all()), "a padding channel is not exactly zero"


# ---------------------------------------------------------------------------------------------------------------- simple_nms
@pytest.mark.parametrize("key7", [0, 2])
@pytest.mark.parametrize("radius", [0, 1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("make_map", [op_cases.nms_tie_map, op_cases.nms_partial_tile_map], ids=["ties45x70", "partial75x130"])
def test_nms_small_maps(hip_lib, make_map, radius, key7):
    with tuned(hip_lib, {7: key7}):
        r = op_cases.nms_case(hip_lib, make_map(radius), radius, device=DEV, runs=2)
    assert r.repeatable and r.guard_ok
    assert torch.equal(r.out, r.ref)


@pytest.mark.parametrize("radius", [1, 2, 3, 4, 6])
def test_nms_large_map(hip_lib, radius):
    """256 tiles of 64 x 64: launch_nms takes the 64-tile kernel by itself (radius 1, 3, 4); key 7 = 0 keeps 32-tile workgroups (1024 of them).  Both == the oracle."""
    s = op_cases.nms_large_map()
    r = op_cases.nms_case(hip_lib, s, radius, device=DEV, runs=2)
    with tuned(hip_lib, {7: 0}):
        o = op_cases.nms_case(hip_lib, s, radius, device=DEV, runs=2)
    assert r.repeatable and r.guard_ok and o.repeatable and o.guard_ok
    assert torch.equal(r.out, r.ref) and torch.equal(o.out, r.ref)
    assert 0 < int((r.ref > 0).sum()) < r.ref.numel() // 2


# ---------------------------------------------------------------------------------------------------------------- keypoint selection
ALL_SELECT = op_cases.SELECT_CASES + op_cases.SELECT_OCCUPANCY_CASES


@pytest.mark.parametrize("case", ALL_SELECT, ids=[c[0] for c in ALL_SELECT])
def test_select_topk(hip_lib, case):
    """Counts, coordinates, score bits, rows past n_out, guard bands and run-to-run bits: all exact (op_cases.SelectResult.check).  On hardware
    the gather's atomics fall in any order and many workgroups run at once; the result must not depend on either."""
    op_cases.run_select_case(hip_lib, case, device=DEV, runs=2).check()


def test_select_topk_reused_workspace(hip_lib):
    for r in op_cases.select_reused_workspace_results(hip_lib, device=DEV, runs=2):
        r.check()


def test_select_topk_zero_fill_beyond_the_map_is_an_error(hip_lib):
    rc, msg, bufs = op_cases.select_error_case(hip_lib, device=DEV)
    assert rc != 0 and "50" in msg and "4 x 5" in msg, (rc, msg)
    assert all(bool((t == op_cases.SENTINEL).all()) for t in bufs)


# ---------------------------------------------------------------------------------------------------------------- descriptor sampling
@pytest.mark.parametrize("fix_sampling", [0, 1])
@pytest.mark.parametrize("h,w,batch,capacity,n_kpts", op_cases.SAMPLE_CASES + [op_cases.SAMPLE_OCCUPANCY_CASE])
def test_sample_descriptors(hip_lib, h, w, batch, capacity, n_kpts, fix_sampling):
    """Within 4 x the fp32 oracle's own error against fp64; the measured pairs are in profiles/sp_post_ops_parity.json."""
    r = op_cases.sample_descriptors_case(hip_lib, h, w, batch, capacity, n_kpts, fix_sampling, device=DEV, runs=2)
    _record({"case": f"sample_descriptors {h}x{w} cells, batch {batch} x {capacity}, fix_sampling {fix_sampling}", "kernel_err": r.err,
             "oracle_fp32_err": r.oracle_err})
    op_cases.check_sample(r)
