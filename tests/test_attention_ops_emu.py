"""CPU: the attention kernels of the three matchers through their operator entry points (dim_op_lg_attention_f32, dim_op_lg_qkv_attention_f32) on the
test emulator against fp64, within 2 x the error of a plain fp32 torch evaluation of the same inputs (tests/op_cases.py: figure, yardstick, cases).
The hardware twin is tests/test_attention_ops_gpu.py; its docstring maps every case to kernel instances and workgroup counts.

What each case reaches:
  A  2 items, n = (70, 130).  split_items 0: one part.  split_items 2: four parts of two key tiles — item 0's parts 2 and 3 are empty (m = -inf, l = 0 in
     the partial record) and part 1 holds six keys.  flat and ramp inputs; the ramp builder asserts that a tile forces a rescale and that one is deferred.
  B  8 items, n = (33, 1, 0, 40, 129, 200, 64, 64), nmax 224 > nsel 200, pair 3 stopped (done = 1 with four parts, done = -1 with one): one key, no
     queries, no keys (exact zeros), one key past a tile, a tile-exact count; untouched rows past n, stopped pair, guard band.
  C  one pair alone and as items 4, 5 of a 6-item call, four parts each: the same bits (no dependence on the neighbours or on the XCD slot).
  D  the fused entry (projection GEMM writes the K | V tile images, attention with kv_ready) against fp64 of the whole composition.
  E  64 items of 0 .. 100 rows: 256 workgroups, the launcher's two-part rule; counts 0, 1, 32, 33 and 100 among them.
"""
import contextlib

import pytest
import torch

from tests import op_cases

VARIANT_IDS = [op_cases.attn_variant_id(v) for v in op_cases.ATTN_VARIANTS]


@contextlib.contextmanager
def arithmetic(lib, mode):
    """dim_tune_set key 1 for the duration of a case; the default (fp16x3) comes back whatever happens."""
    try:
        assert lib.dim_tune_set(1, mode) == 0, lib.dim_last_error()
        yield
    finally:
        lib.dim_tune_set(1, 2)


@pytest.mark.parametrize("family", ["flat", "ramp"])
@pytest.mark.parametrize("split_items", [0, 2], ids=["1part", "4parts"])
@pytest.mark.parametrize("variant", op_cases.ATTN_VARIANTS, ids=VARIANT_IDS)
def test_attention_small_ragged(emu_lib, variant, split_items, family):
    width, kind, mode = variant
    with arithmetic(emu_lib, mode):
        r = op_cases.attn_case_a(emu_lib, width, kind, split_items, family)
    op_cases.check_attention(r, f"A {op_cases.attn_variant_id(variant)} split_items {split_items} {family}")


@pytest.mark.parametrize("done3,split_items", [(1, 8), (-1, 0)], ids=["done1-4parts", "done-1-1part"])
@pytest.mark.parametrize("variant", op_cases.ATTN_VARIANTS, ids=VARIANT_IDS)
def test_attention_edge_counts_and_stopped_pair(emu_lib, variant, done3, split_items):
    width, kind, mode = variant
    with arithmetic(emu_lib, mode):
        r = op_cases.attn_case_b(emu_lib, width, kind, done3, split_items)
    op_cases.check_attention(r, f"B {op_cases.attn_variant_id(variant)} done {done3} split_items {split_items}")


@pytest.mark.parametrize("variant", op_cases.ATTN_VARIANTS, ids=VARIANT_IDS)
def test_attention_item_does_not_depend_on_its_neighbours(emu_lib, variant):
    width, kind, mode = variant
    with arithmetic(emu_lib, mode):
        alone, among = op_cases.attn_case_c(emu_lib, width, kind)
    op_cases.check_attention(alone, f"C alone {op_cases.attn_variant_id(variant)}")
    op_cases.check_attention(among, f"C among {op_cases.attn_variant_id(variant)}")
    assert torch.equal(alone.out, among.out[4:]), "the pair's context rows differ between the 2-item and the 6-item call"


@pytest.mark.parametrize("split_items", [0, 2], ids=["1part", "4parts"])
@pytest.mark.parametrize("kind", [0, 1], ids=["self", "cross"])
def test_attention_fused_projection(emu_lib, kind, split_items):
    """Case D at case A's counts: 2 items x 130 rows x 768 | 512 columns is a small problem of at most 512 blocks of 64 rows, which launch_gemm_x6 runs with the
    32 x 128 block that writes the tile images (gemm_x6_qkv_small_kernel) — the smallest shape of the fused path.  The separate entry on the fp64
    projection rounded to fp32 meets the same bound.  The two are NOT bit-equal: the fused path's q, k, v are the GEMM's fp16x3 sums (a few 1e-7 from
    the rounded fp64 projection), its K image is rotated and split from the accumulators in the GEMM's epilogue, and under kind 1 Q is the K image itself
    with the softmax scale applied to the scores where the separate path scales Q before its split."""
    fused, separate = op_cases.lg_qkv_attention_case(emu_lib, kind, op_cases.attn_items(op_cases.ATTN_A["ns"], 6), 130, 130, split_items, runs=2)
    op_cases.check_attention(fused, f"D fused kind {kind} split_items {split_items}")
    op_cases.check_attention(separate, f"D separate kind {kind} split_items {split_items}")
    assert not torch.equal(fused.out, separate.out)


def test_attention_fused_projection_refuses_an_unfused_shape(emu_lib):
    rc, msg = op_cases.lg_qkv_attention_unfused_error(emu_lib)
    assert rc != 0 and "gemm_x6_fuses_kv" in msg and "36 items of 300 rows" in msg, (rc, msg)
    with arithmetic(emu_lib, 1):
        rc, msg = op_cases.lg_qkv_attention_unfused_error(emu_lib)
    assert rc != 0 and "fp16x3" in msg, (rc, msg)


@pytest.mark.parametrize("mode", [2, 1], ids=["fp16x3", "bf16x6"])
@pytest.mark.parametrize("kind", [0, 1, 2, 3], ids=op_cases.ATTN_KIND_NAMES)
def test_attention_two_parts(emu_lib, kind, mode):
    with arithmetic(emu_lib, mode):
        r = op_cases.attn_case_e(emu_lib, kind)
    op_cases.check_attention(r, f"E kind {kind} mode {mode}")


@pytest.mark.parametrize("variant", op_cases.ATTN_REFUSED, ids=[op_cases.attn_variant_id(v) for v in op_cases.ATTN_REFUSED])
def test_attention_refuses_an_arithmetic_it_does_not_have(emu_lib, variant):
    """SuperGlue and LighterGlue run in the split arithmetics only (dim_sg_match, launch_lgl_attention): an error that says so, nothing launched."""
    width, kind, mode = variant
    with arithmetic(emu_lib, mode):
        rc, msg, clean = op_cases.lg_attention_error(emu_lib, width, kind)
    assert rc != 0 and "split arithmetics" in msg and clean, (rc, msg, clean)


def test_attention_range_guard(emu_lib):
    """A key pair (3000, 3000) that the rotary turns into (0, 4243): past the exact range of the fp16x3 split (4094) although no input is.  fp16x3 reports
    it at the operator site (and is then NOT fp32-accurate, which is what the guard is for); bf16x6 has no range limit and meets the bound on the same
    inputs; the cross layout has no rotation and reports nothing."""
    r, count = op_cases.attn_case_guard(emu_lib, 0)
    assert count > 0, "the rotated key above 4094 was not reported"
    with arithmetic(emu_lib, 1):
        r, count = op_cases.attn_case_guard(emu_lib, 0)
    assert count == 0
    op_cases.check_attention(r, "guard inputs, bf16x6")
    r, count = op_cases.attn_case_guard(emu_lib, 1)
    assert count == 0, "3000 is inside the range: nothing to report without a rotation"
