"""GPU: confidence, decide, prune, assign and finalize of LightGlue / LighterGlue ON HARDWARE through their operator entry points against fp64, with the
builders, cases and bounds of tests/test_lg_head_ops_emu.py (its docstring maps the cases to kernels), every case run twice for the same bits, plus the
shapes that only hardware can judge (tests/test_ops_gpu.py: the emulator runs workgroups one after another): 16 pairs x nmax 260 with ragged counts
(0 on one side, 1 and nmax among them) for assign and prune, and a pair alone against the same pair among 16.  The measured (figure, yardstick) pairs go
to the parity log (_record); the committed table is profiles/lg_head_ops_parity.json.  No live similarity or descriptor is non-finite here (only the dead rows, which
no kernel may use, hold NaN) and no arg is out of range: those are emulator cases.

Workgroups at 16 pairs x 260: row passes cdiv(260, 4) x 32 (stats) / x 16 (argmax) = 2080 / 1040 of 4 waves, column passes cdiv(260, 64) x 16 = 80 of 16 waves,
prune gather / copy-back 65 x 32 = 2080, scan 32 of 16 waves.
"""
import pytest
import torch

from tests import op_cases
from tests.test_aliked_gpu import _record   # appends one JSON line to the measured-parity log

pytestmark = pytest.mark.gpu

DEV = "cuda"
WIDTHS = [256, 96]
TIES = [("fast8", "lanes"), ("fast8", "float4"), ("fast16", "lanes"), ("fast16", "float4"), ("fast16", "lane16"), ("generic", "lanes"), ("generic", "lane")]


def check(r, what):
    for k, (f, y) in r.figures.items():
        _record({"case": f"lg_head_op {what} {k}", "figure": f, "yardstick_fp32": y})
    op_cases.check_head(r, what)


@pytest.mark.parametrize("family", ["flat", "planted", "ramp"])
@pytest.mark.parametrize("path", ["fast8", "fast16", "generic"])
@pytest.mark.parametrize("width", WIDTHS)
def test_assign_families(hip_lib, width, path, family):
    check(op_cases.assign_path_case(hip_lib, width, path, family, device=DEV), f"assign w{width} {path} {family}")


@pytest.mark.parametrize("path,ties", TIES, ids=[f"{a}-{b}" for a, b in TIES])
@pytest.mark.parametrize("width", WIDTHS)
def test_assign_first_index_wins_a_tie(hip_lib, width, path, ties):
    check(op_cases.assign_path_case(hip_lib, width, path, "flat", ties=ties, device=DEV), f"assign w{width} {path} ties {ties}")


@pytest.mark.parametrize("width", WIDTHS)
def test_assign_fast_and_generic_agree(hip_lib, width):
    fast = op_cases.assign_path_case(hip_lib, width, "fast8", "planted", device=DEV, runs=1)
    generic = op_cases.assign_path_case(hip_lib, width, "generic", "planted", device=DEV, runs=1)
    live = fast.out["live"]
    assert torch.equal(fast.out["arg"][live], generic.out["arg"][:, :132][live])


@pytest.mark.parametrize("path", ["fast8", "fast16", "generic"])
@pytest.mark.parametrize("width", WIDTHS)
def test_assign_masks_the_dead_columns(hip_lib, width, path):
    """The dead entries of sim hold 1e30 instead of NaN (a NaN drops out of fmaxf and of a compare by itself, a finite value does not)."""
    check(op_cases.assign_path_case(hip_lib, width, path, "flat", pad=1e30, device=DEV), f"assign w{width} {path} flat, dead entries 1e30")


@pytest.mark.parametrize("tag", [5, 0], ids=["tag5", "tag0"])
@pytest.mark.parametrize("width", WIDTHS)
def test_assign_skips_the_pairs_its_tag_does_not_select(hip_lib, width, tag):
    check(op_cases.assign_stopped_case(hip_lib, width, tag, device=DEV), f"assign w{width} stopped tag {tag}")


@pytest.mark.parametrize("width", WIDTHS)
def test_assign_many_resident_workgroups(hip_lib, width):
    check(op_cases.assign_occupancy_case(hip_lib, width, device=DEV), f"assign w{width} 16 pairs x 260 ragged planted")


@pytest.mark.parametrize("width", WIDTHS)
def test_assign_pair_does_not_depend_on_its_neighbours(hip_lib, width):
    alone, among = op_cases.assign_alone_and_among(hip_lib, width, device=DEV)
    check(alone, f"assign w{width} pair alone")
    check(among, f"assign w{width} pair among 16")
    for k in ("zls", "rmax", "rlse", "best", "arg"):
        assert op_cases._bits_equal(alone.out[k], among.out[k][18:20]), k
    assert op_cases._bits_equal(alone.out["dense"][0], among.out["dense"][9])


@pytest.mark.parametrize("prune_enabled", [0, 1])
@pytest.mark.parametrize("out_cap", [50, 1032])
def test_finalize(hip_lib, out_cap, prune_enabled):
    r = op_cases.finalize_case(hip_lib, out_cap, prune_enabled, device=DEV)
    check(r, f"finalize out_cap {out_cap} prune {prune_enabled}")
    assert r.out["n_matches"].tolist()[2] == min(out_cap, r.out["exp"][2][2].shape[0])


@pytest.mark.parametrize("use_token", [1, 0])
@pytest.mark.parametrize("width", WIDTHS)
def test_prune_two_rounds(hip_lib, width, use_token):
    r1, r2, s1, s2 = op_cases.prune_case(hip_lib, width, use_token, device=DEV)
    check(r1, f"prune w{width} token {use_token} round 1")
    check(r2, f"prune w{width} token {use_token} round 2")
    assert int(s1["done"][3]) == -4 and int(s1["done"][4]) == 3 and not r1.out["moved"][4] and any(r2.out["moved"])


@pytest.mark.parametrize("width", WIDTHS)
def test_prune_many_resident_workgroups(hip_lib, width):
    r1, r2, s1, s2 = op_cases.prune_case(hip_lib, width, 1, pairs=op_cases.prune_ragged_pairs(16, 260, 8), nmax=260, nsel=260, device=DEV)
    check(r1, f"prune w{width} 16 pairs x 260 ragged round 1")
    check(r2, f"prune w{width} 16 pairs x 260 ragged round 2")
    assert int(s1["done"][1]) == -4, "the pair with an empty side leaves"


@pytest.mark.parametrize("use_token", [1, 0])
@pytest.mark.parametrize("width", WIDTHS)
def test_confidence(hip_lib, width, use_token):
    check(op_cases.confidence_case(hip_lib, width, use_token, device=DEV), f"confidence w{width} token {use_token}")


@pytest.mark.parametrize("early,last", [(1, 0), (0, 1), (0, 0)], ids=["early", "last", "neither"])
def test_decide(hip_lib, early, last):
    check(op_cases.decide_case(hip_lib, early, last, device=DEV), f"decide early {early} last {last}")
