"""GPU: the attention kernels of the three matchers ON HARDWARE through dim_op_lg_attention_f32 / dim_op_lg_qkv_attention_f32 against fp64, with the
builders, cases and bound (2 x the fp32 torch yardstick) of tests/test_attention_ops_emu.py, every case run twice for the same bits, plus the
occupancy shapes that only hardware can judge (tests/test_ops_gpu.py: the emulator runs workgroups one after another).  The measured (figure,
yardstick) pairs go to the parity log (_record); the committed table is profiles/lg_attention_ops_parity.json.

Case -> kernels (launch_lg_attention / launch_lg_attention_x6 / launch_lgl_attention; MODE 2 = fp16x3, 1 = bf16x6; wg = workgroups of the attention
kernel, surplus ones of the XCD-rounded 1-D grid included, + those of the merge kernel):

  width 256, fp32     lg_rotary_kernel (kind 0) + attn_kernel, grid (cdiv(nmax, 128), 4, items): never split
  width 256, split    kv_prep_kernel<MODE> (tiles, 4, items) + attn_x6_kernel<MODE> [+ attn_combine_kernel<2 | 4> (cdiv(nsel, 16), 4, items)]
  width 96            kv_prep96_kernel<MODE> + attn_d96_kernel<MODE> [+ attn_combine96_kernel (cdiv(nsel, 8), items)]
  A  2 items, nsel 130     256: 1 part 16 wg, 4 parts 64 wg + combine<4> 72 wg (fp32: 16 wg)      96: 1 part 16 wg, 4 parts 64 wg + 34 wg
  B  8 items, nsel 200     256: 4 parts 256 wg + combine<4> 416 wg, 1 part 64 wg (fp32: 64 wg)    96: 4 parts 64 wg + 200 wg, 1 part 16 wg
  C  2 | 6 items, nsel 130 256: 4 parts 64 | 192 wg + combine<4>                                   96: 4 parts 64 | 64 wg + combine96
  D  2 items, nsel 130     gemm_x6_qkv_small_kernel<64,true,256> (5 x 6 x 2 | 5 x 4 x 2 wg) + attn_x6_kernel<2> with kv_ready (no kv_prep), 1 | 4 parts
  E  64 items, nsel 100    256: 2 parts 512 wg + combine<2> 1792 wg
  occupancy (ramp, ragged counts 0 .. nsel incl. nsel, 0, 1, nsel - 1)
     256: 64 items x 260   1 part  768 wg                     fp16x3 kinds 0, 1, 3; bf16x6 kind 0
          32 items x 260   2 parts 768 wg + combine<2>        fp16x3 kinds 0, 1
          20 items x 260   4 parts 960 wg + combine<4>        fp16x3 kinds 0, 1
     96:  64 items x 400   2 parts 512 wg + combine96         fp16x3 kinds 0, 1
          128 items x 520  1 part  640 wg                     fp16x3 kinds 0, 1
"""
import contextlib

import pytest
import torch

from tests import op_cases
from tests.test_aliked_gpu import _record   # appends one JSON line to the measured-parity log

pytestmark = pytest.mark.gpu

DEV = "cuda"
VARIANT_IDS = [op_cases.attn_variant_id(v) for v in op_cases.ATTN_VARIANTS]


@contextlib.contextmanager
def arithmetic(lib, mode):
    try:
        assert lib.dim_tune_set(1, mode) == 0, lib.dim_last_error()
        yield
    finally:
        lib.dim_tune_set(1, 2)


def check(r, what):
    _record({"case": "lg_attention_op " + what, "figure": r.figure, "yardstick_fp32": r.yardstick})
    op_cases.check_attention(r, what)


@pytest.mark.parametrize("family", ["flat", "ramp"])
@pytest.mark.parametrize("split_items", [0, 2], ids=["1part", "4parts"])
@pytest.mark.parametrize("variant", op_cases.ATTN_VARIANTS, ids=VARIANT_IDS)
def test_attention_small_ragged(hip_lib, variant, split_items, family):
    width, kind, mode = variant
    with arithmetic(hip_lib, mode):
        r = op_cases.attn_case_a(hip_lib, width, kind, split_items, family, device=DEV)
    check(r, f"A {op_cases.attn_variant_id(variant)} split_items {split_items} {family}")


@pytest.mark.parametrize("done3,split_items", [(1, 8), (-1, 0)], ids=["done1-4parts", "done-1-1part"])
@pytest.mark.parametrize("variant", op_cases.ATTN_VARIANTS, ids=VARIANT_IDS)
def test_attention_edge_counts_and_stopped_pair(hip_lib, variant, done3, split_items):
    width, kind, mode = variant
    with arithmetic(hip_lib, mode):
        r = op_cases.attn_case_b(hip_lib, width, kind, done3, split_items, device=DEV)
    check(r, f"B {op_cases.attn_variant_id(variant)} done {done3} split_items {split_items}")


@pytest.mark.parametrize("variant", op_cases.ATTN_VARIANTS, ids=VARIANT_IDS)
def test_attention_item_does_not_depend_on_its_neighbours(hip_lib, variant):
    width, kind, mode = variant
    with arithmetic(hip_lib, mode):
        alone, among = op_cases.attn_case_c(hip_lib, width, kind, device=DEV)
    check(alone, f"C alone {op_cases.attn_variant_id(variant)}")
    check(among, f"C among {op_cases.attn_variant_id(variant)}")
    assert torch.equal(alone.out, among.out[4:]), "the pair's context rows differ between the 2-item and the 6-item call"


@pytest.mark.parametrize("split_items", [0, 2], ids=["1part", "4parts"])
@pytest.mark.parametrize("kind", [0, 1], ids=["self", "cross"])
def test_attention_fused_projection(hip_lib, kind, split_items):
    """Case D (why fused and separate are not bit-equal: tests/test_attention_ops_emu.py)."""
    fused, separate = op_cases.lg_qkv_attention_case(hip_lib, kind, op_cases.attn_items(op_cases.ATTN_A["ns"], 6), 130, 130, split_items, device=DEV, runs=2)
    check(fused, f"D fused kind {kind} split_items {split_items}")
    check(separate, f"D separate kind {kind} split_items {split_items}")
    assert not torch.equal(fused.out, separate.out)


def test_attention_fused_projection_refuses_an_unfused_shape(hip_lib):
    rc, msg = op_cases.lg_qkv_attention_unfused_error(hip_lib, device=DEV)
    assert rc != 0 and "gemm_x6_fuses_kv" in msg, (rc, msg)


@pytest.mark.parametrize("mode", [2, 1], ids=["fp16x3", "bf16x6"])
@pytest.mark.parametrize("kind", [0, 1, 2, 3], ids=op_cases.ATTN_KIND_NAMES)
def test_attention_two_parts(hip_lib, kind, mode):
    with arithmetic(hip_lib, mode):
        r = op_cases.attn_case_e(hip_lib, kind, device=DEV)
    check(r, f"E kind {kind} {op_cases.ATTN_MODE_NAMES[mode]}")


OCCUPANCY = [(shape, kind, 2) for shape in op_cases.ATTN_OCCUPANCY for kind in (0, 1)] + [(op_cases.ATTN_OCCUPANCY[0], 3, 2), (op_cases.ATTN_OCCUPANCY[0], 0, 1)]


@pytest.mark.parametrize("shape,kind,mode", OCCUPANCY,
                         ids=[f"w{s[0]}-{s[1]}x{s[2]}-{s[4]}parts-{op_cases.ATTN_KIND_NAMES[k]}-{op_cases.ATTN_MODE_NAMES[m]}" for s, k, m in OCCUPANCY])
def test_attention_many_resident_workgroups(hip_lib, shape, kind, mode):
    width, items, nsel, split_items, parts, wgs = shape
    with arithmetic(hip_lib, mode):
        r = op_cases.attn_case_occupancy(hip_lib, width, kind, items, nsel, split_items, parts, wgs, device=DEV)
    check(r, f"occupancy w{width} {items} x {nsel} {parts} parts kind {kind} {op_cases.ATTN_MODE_NAMES[mode]}")


@pytest.mark.parametrize("variant", op_cases.ATTN_REFUSED, ids=[op_cases.attn_variant_id(v) for v in op_cases.ATTN_REFUSED])
def test_attention_refuses_an_arithmetic_it_does_not_have(hip_lib, variant):
    width, kind, mode = variant
    with arithmetic(hip_lib, mode):
        rc, msg, clean = op_cases.lg_attention_error(hip_lib, width, kind, device=DEV)
    assert rc != 0 and "split arithmetics" in msg and clean, (rc, msg, clean)


def test_attention_range_guard(hip_lib):
    """tests/test_attention_ops_emu.py::test_attention_range_guard on hardware."""
    r, count = op_cases.attn_case_guard(hip_lib, 0, device=DEV)
    assert count > 0, "the rotated key above 4094 was not reported"
    with arithmetic(hip_lib, 1):
        r, count = op_cases.attn_case_guard(hip_lib, 0, device=DEV, runs=2)
    assert count == 0
    check(r, "guard inputs, bf16x6")
    r, count = op_cases.attn_case_guard(hip_lib, 1, device=DEV)
    assert count == 0, "3000 is inside the range: nothing to report without a rotation"
