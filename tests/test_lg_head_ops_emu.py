"""CPU: the kernels that turn the LightGlue / LighterGlue network output into the integers a caller sees (csrc/lg_kernels.hip, the 96-wide forms in
lgl_kernels.hip), each through its operator entry point on the test emulator against a plain fp64 torch reference written from the operation
(tests/op_cases.py, "LightGlue head": figures, yardsticks, margins, cases).  The hardware twin is tests/test_lg_head_ops_gpu.py.

  dim_op_lg_confidence_f32   lg_confidence_kernel / lgl_confidence_kernel            n = 1, 31, 32, 33, 130: around the 32 rows of a workgroup
  dim_op_lg_decide           lg_decide_kernel                                         early, last, neither; counters reset; stopped pairs keep their layer
  dim_op_lg_prune            lg_prune_scan / gather / copyback / commit, lgl_prune_*  n = 130 and 1030 (two rows per scan thread), pruning_min and + 1, nothing
                                                                                      and everything pruned, a stopped pair, two rounds (ind no longer the identity)
  dim_op_lg_assign_f32       fast8:   lg_row_stats4<8> / col_stats4 / row_argmax4<8> / col_argmax4       nmax 132
                             fast16:  the same with rows in 16 registers per lane                         nmax 2052, (37, 2049) and (2049, 37)
                             generic: lg_row_stats / col_stats / row_argmax / col_argmax                  nmax 134 (no multiple of 4)
                             families flat, planted, ramp (a column's running maximum moves at every step of lg_col_stats4_kernel), ties (first index wins)
  dim_op_lg_finalize         lg_finalize_kernel                                       1030 x 37 and transpose (two rows per thread), pruned 130 x 130, out_cap,
                                                                                      done > 0 / 0 / < 0, prune on / off, and an arg of 0x7fffffff (emulator only)
"""
import pytest
import torch

from tests import op_cases

WIDTHS = [256, 96]
TIES = [("fast8", "lanes"), ("fast8", "float4"), ("fast16", "lanes"), ("fast16", "float4"), ("fast16", "lane16"), ("generic", "lanes"), ("generic", "lane")]


@pytest.mark.parametrize("family", ["flat", "planted", "ramp"])
@pytest.mark.parametrize("path", ["fast8", "fast16", "generic"])
@pytest.mark.parametrize("width", WIDTHS)
def test_assign_families(emu_lib, width, path, family):
    op_cases.check_head(op_cases.assign_path_case(emu_lib, width, path, family), f"assign w{width} {path} {family}")


@pytest.mark.parametrize("path,ties", TIES, ids=[f"{a}-{b}" for a, b in TIES])
@pytest.mark.parametrize("width", WIDTHS)
def test_assign_first_index_wins_a_tie(emu_lib, width, path, ties):
    """Two bit-identical columns (different lanes / one float4 / one lane) and two bit-identical rows in different row groups: arg is the lower index, which the
    builder asserts to be some row's / column's maximum."""
    op_cases.check_head(op_cases.assign_path_case(emu_lib, width, path, "flat", ties=ties), f"assign w{width} {path} ties {ties}")


@pytest.mark.parametrize("width", WIDTHS)
def test_assign_fast_and_generic_agree(emu_lib, width):
    """The same pairs at row stride 132 (16-byte kernels) and 134 (generic kernels): each within the fp64 bound (above) and the same arg."""
    fast = op_cases.assign_path_case(emu_lib, width, "fast8", "planted", runs=1)
    generic = op_cases.assign_path_case(emu_lib, width, "generic", "planted", runs=1)
    live = fast.out["live"]
    assert torch.equal(fast.out["arg"][live], generic.out["arg"][:, :132][live])


@pytest.mark.parametrize("path", ["fast8", "fast16", "generic"])
@pytest.mark.parametrize("width", WIDTHS)
def test_assign_masks_the_dead_columns(emu_lib, width, path):
    """The dead entries of sim hold 1e30 instead of NaN (a NaN drops out of fmaxf and of a compare by itself, a finite value does not)."""
    op_cases.check_head(op_cases.assign_path_case(emu_lib, width, path, "flat", pad=1e30), f"assign w{width} {path} flat, dead entries 1e30")


@pytest.mark.parametrize("tag", [5, 0], ids=["tag5", "tag0"])
@pytest.mark.parametrize("width", WIDTHS)
def test_assign_skips_the_pairs_its_tag_does_not_select(emu_lib, width, tag):
    op_cases.check_head(op_cases.assign_stopped_case(emu_lib, width, tag), f"assign w{width} stopped tag {tag}")


@pytest.mark.parametrize("prune_enabled", [0, 1])
@pytest.mark.parametrize("out_cap", [50, 1032])
def test_finalize(emu_lib, out_cap, prune_enabled):
    r = op_cases.finalize_case(emu_lib, out_cap, prune_enabled)
    op_cases.check_head(r, f"finalize out_cap {out_cap} prune {prune_enabled}")
    assert r.out["n_matches"].tolist()[2] == min(out_cap, r.out["exp"][2][2].shape[0]) and r.out["exp"][2][2].shape[0] > 50   # (the cap cuts pair 2)


def test_finalize_follows_no_index_outside_the_other_side(emu_lib):
    """One row and one column of pair 2 carry 0x7fffffff, what the argmax kernels leave where no score compares greater than -inf: "no match" for both,
    the rest as the reference has it, nothing written outside."""
    r = op_cases.finalize_case(emu_lib, 1032, 1, bad=True)
    op_cases.check_head(r, "finalize with the index sentinel")
    ind0, ind1 = op_cases._finalize_pair(130, 130, 150, 141, False, True, 52)[:2]
    assert int(r.out["mfull"][2, 0, ind0[7]]) == -1 and float(r.out["msfull"][2, 0, ind0[7]]) == 0.0
    assert int(r.out["mfull"][2, 1, ind1[11]]) == -1 and float(r.out["msfull"][2, 1, ind1[11]]) == 0.0


@pytest.mark.parametrize("use_token", [1, 0])
@pytest.mark.parametrize("width", WIDTHS)
def test_prune_two_rounds(emu_lib, width, use_token):
    r1, r2, s1, s2 = op_cases.prune_case(emu_lib, width, use_token)
    op_cases.check_head(r1, f"prune w{width} token {use_token} round 1")
    op_cases.check_head(r2, f"prune w{width} token {use_token} round 2")
    pm = op_cases.PRUNE_MIN
    assert not r1.out["moved"][2] and int(r1.out["n_new"][2]) == pm, "n == pruning_min is not pruned"
    assert int(r1.out["dest"][3, 0]) != -2, "n == pruning_min + 1 is"
    assert not r1.out["moved"][4] and int(s1["n_cur"][4]) == 130 and bool((s1["prune"][4, :130] == 2).all()), "nothing pruned: only the counters move"
    assert int(s1["n_cur"][6]) == 0 and int(s1["done"][3]) == -(2 + 2), "a side pruned to nothing leaves through the no-keypoints exit"
    assert int(s1["done"][4]) == 3 and int(s2["done"][4]) == 3
    assert not torch.equal(s1["ind"][0, :int(s1["n_cur"][0])], torch.arange(int(s1["n_cur"][0]), dtype=torch.int32)), "round 2 starts from a non-identity ind"
    assert any(r2.out["moved"])


@pytest.mark.parametrize("use_token", [1, 0])
@pytest.mark.parametrize("width", WIDTHS)
def test_confidence(emu_lib, width, use_token):
    op_cases.check_head(op_cases.confidence_case(emu_lib, width, use_token), f"confidence w{width} token {use_token}")


@pytest.mark.parametrize("early,last", [(1, 0), (0, 1), (0, 0)], ids=["early", "last", "neither"])
def test_decide(emu_lib, early, last):
    op_cases.check_head(op_cases.decide_case(emu_lib, early, last), f"decide early {early} last {last}")


def test_head_ops_refuse_bad_arguments(emu_lib):
    op_cases._bind_head(emu_lib)
    hs = op_cases.LgHeadState(128, 1, 8, 8)
    assert emu_lib.dim_op_lg_decide(hs, 0, 0.9, 1, 0, None) != 0 and b"width" in emu_lib.dim_last_error()
    hs = op_cases.LgHeadState(256, 1, 8, 9)
    assert emu_lib.dim_op_lg_decide(hs, 0, 0.9, 1, 0, None) != 0 and b"nsel" in emu_lib.dim_last_error()
    hs = op_cases.LgHeadState(256, 1, 8, 8)
    assert emu_lib.dim_op_lg_decide(hs, 0, 0.9, 1, 0, None) != 0 and b"null n_orig" in emu_lib.dim_last_error()
    assert emu_lib.dim_op_lg_finalize(hs, 9, 0, 0.1, 8, None, None, None, None, None, None, None, None) != 0 and b"null" in emu_lib.dim_last_error()
    assert emu_lib.dim_op_lg_prune_workspace_bytes(128, 2, 8) == 0 and emu_lib.dim_op_lg_prune_workspace_bytes(96, 2, 8) == op_cases.prune_ws_layout(96, 2, 8)[3]
