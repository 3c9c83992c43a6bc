"""CPU: the HIP ALIKED sources on the test emulator vs the oracle (which is pinned bit-exactly
against the reference's aliked.py by oracle/make_golden.py) and vs the reference golden."""
import importlib
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import aliked_ref
from tests import golden_cases as gc
from tests import selection_mode_cases

al_mod = importlib.import_module("deep-image-matching_amd.aliked_hip")
GOLD = Path(__file__).parent / "golden"


def compare_aliked(out, ref, kp_tol=1e-3, desc_tol=1e-3, score_tol=1e-3, max_missing=0, label=None, ref_score_map=None, threshold=0.2,
                   tie_tol=2e-5, nms_radius=3, n_limit=None):
    """north_star's bar: keypoint set exact, descriptors / scores within 1e-3 (keypoint coordinates likewise: they are
    sub-pixel soft-argmax outputs in pixels).  Every measured maximum is returned and, with ``label``, appended to
    gpurun_out/parity_measured.jsonl so that the numbers behind the assertion are on record."""
    # keypoints are sub-pixel (NMS pixel + soft-argmax offset, which can exceed half a pixel): pair each output keypoint with the
    # NEAREST reference keypoint (rounding to the pixel grid would split a pair whose offset sits at x.5) and require a bijection
    from scipy.spatial import cKDTree
    ko, kr = out["keypoints"].numpy().astype(np.float64), ref["keypoints"].numpy().astype(np.float64)
    pairs = []
    if len(ko) and len(kr):
        dist, nn = cKDTree(kr).query(ko)
        used = set()
        for i, (d, j) in enumerate(zip(dist, nn)):
            if d <= 0.05 and int(j) not in used:       # 0.05 px: far below the NMS spacing, far above any rounding difference
                used.add(int(j)); pairs.append((i, int(j)))
    res = {"n_out": len(ko), "n_ref": len(kr), "common": len(pairs)}
    ia = torch.tensor([p[0] for p in pairs], dtype=torch.long); ib = torch.tensor([p[1] for p in pairs], dtype=torch.long)
    only_out = sorted(set(range(len(ko))) - {p[0] for p in pairs}); only_ref = sorted(set(range(len(kr))) - {p[1] for p in pairs})
    res["kp"] = (out["keypoints"][ia] - ref["keypoints"][ib]).abs().max().item() if pairs else 0.0       # (an image without detections: nothing to compare)
    res["score"] = (out["scores"][ia] - ref["scores"][ib]).abs().max().item() if pairs else 0.0
    res["desc"] = (out["descriptors"][:, ia] - ref["descriptors"][:, ib]).abs().max().item() if pairs else 0.0
    if label is not None:
        import json
        d = Path(__file__).resolve().parents[1] / "gpurun_out"
        try:
            d.mkdir(exist_ok=True)
            with open(d / "parity_measured.jsonl", "a") as f:
                f.write(json.dumps({"case": label, **res}) + "\n")
        except OSError:
            pass
    if (only_out or only_ref) and ref_score_map is not None:
        # The keypoint SET must be exact except for numerical near-ties of the selection itself: DKD keeps the n_limit highest
        # NMS maxima above the threshold (ALN:170-186), so a keypoint found on one side only must sit — in the REFERENCE's own
        # score map — within tie_tol of the weakest selected score (the n_limit cut), of the threshold, or of another pixel of
        # its own NMS window (an exact-equality tie of simple_nms).  (The reference is
        # not stable there either: its fp32 and fp64 evaluations of tests/golden case gray_limit differ in 5 of 60 keypoints.)
        sm = ref_score_map.reshape(ref_score_map.shape[-2], ref_score_map.shape[-1])
        # the NMS pixel of a refined keypoint is the local maximum within one pixel of its rounded position
        def nms_score(xy):
            x, y = int(round(xy[0])), int(round(xy[1]))
            return float(sm[max(0, y - 1): y + 2, max(0, x - 1): x + 2].max())
        def nms_tie(xy, radius=nms_radius):
            """a second pixel inside the NMS window within tie_tol of the maximum: simple_nms compares floats with == (ALN:66-89), so
            on a plateau (the sigmoid saturates near 1) the reference keeps BOTH pixels while a 1e-7 difference keeps one"""
            x, y = int(round(xy[0])), int(round(xy[1]))
            win = sm[max(0, y - radius): y + radius + 1, max(0, x - radius): x + radius + 1].reshape(-1)
            top = torch.topk(win, 2).values
            return float(top[0] - top[1])
        # the n_limit cut of the REFERENCE: the n_limit-th largest NMS maximum above the threshold (DKD, ALN:150-186)
        nms = aliked_ref._simple_nms(ref_score_map.reshape(1, 1, *sm.shape), nms_radius)[0, 0].clone()
        nms[:nms_radius] = 0; nms[-nms_radius:] = 0; nms[:, :nms_radius] = 0; nms[:, -nms_radius:] = 0
        cand = torch.sort(sm[nms > threshold], descending=True).values
        cut = float(cand[n_limit - 1]) if n_limit is not None and len(cand) > n_limit else threshold
        res["one_sided"] = {"out": [(ko[i].tolist(), nms_score(ko[i]), nms_tie(ko[i])) for i in only_out],
                            "ref": [(kr[j].tolist(), nms_score(kr[j]), nms_tie(kr[j])) for j in only_ref], "cut": cut}
        for xy in [ko[i] for i in only_out] + [kr[j] for j in only_ref]:
            v = nms_score(xy)
            assert min(abs(v - cut), abs(v - threshold), nms_tie(xy)) <= tie_tol, (tuple(xy), v, cut, nms_tie(xy), res)
        res["near_tie_keypoints"] = max(len(only_out), len(only_ref))
        max_missing = max(max_missing, res["near_tie_keypoints"])
    assert len(ko) == len(kr) and len(pairs) >= len(kr) - max_missing, res
    assert res["kp"] <= kp_tol and res["score"] <= score_tol and res["desc"] <= desc_tol, res
    return res


@pytest.mark.parametrize("name", list(gc.AL_CASES))
def test_aliked_emulated_vs_oracle_and_golden(emu_lib, name):
    case = gc.AL_CASES[name]
    sd, img = gc.al_weights(case), gc.al_image(case)
    net = al_mod.AlikedHIP(sd, case["cfg"], max_batch=1, max_hw=(case["H"], case["W"]), capacity=4096, device="cpu", lib=emu_lib)
    out = {k: v.cpu() for k, v in net(img).items()}
    ref = aliked_ref.aliked_forward(img, sd, case["cfg"], taps=True)
    taps = net.debug_taps()
    pt, pl = taps["pad"]
    H, W = case["H"], case["W"]
    fm = torch.nn.functional.normalize(taps["x1234"][0, pt:pt + H, pl:pl + W].permute(2, 0, 1), dim=0)
    assert (fm - ref["feature_map"][0]).abs().max().item() < 1e-3
    res = compare_aliked(out, ref)
    g = np.load(GOLD / f"al_{name}.npz")
    gold = {k: torch.from_numpy(g[k]) for k in ("keypoints", "scores", "descriptors")}
    compare_aliked(out, gold)


def test_aliked_top_k_mode_vs_oracle(emu_lib):
    selection_mode_cases.aliked_top_k_mode_vs_oracle(emu_lib, "cpu")


def test_aliked_mean_threshold_mode_vs_oracle(emu_lib):
    selection_mode_cases.aliked_mean_threshold_mode_vs_oracle(emu_lib, "cpu")


def test_aliked_top_k_mode_fills_up_with_zero_score_pixels(emu_lib):
    selection_mode_cases.aliked_top_k_mode_fills_up_with_zero_score_pixels(emu_lib, "cpu")


def test_aliked_more_than_4096_keypoints(emu_lib):
    selection_mode_cases.aliked_more_than_4096_keypoints(emu_lib, "cpu")


REAL_ALIKED = Path(__file__).parent / "assets" / "aliked-n16rot.pth"   # byte copy of the reference's thirdparty/ALIKED/models/aliked-n16rot.pth
REAL_ALIKED_N32 = Path(__file__).parent / "assets" / "aliked-n32.pth"  # likewise (md5 fb7434eaaf6c52604541322d7e0fde58)


@pytest.mark.parametrize("model", ["aliked-n16rot", "aliked-n32", "aliked-t16"])
def test_aliked_real_checkpoint_through_the_hip_sources(emu_lib, model):
    """The REAL aliked-n16rot.pth / aliked-n32.pth that ship inside the reference tree (tests/assets holds byte copies: data files, md5
    bfec5e8086e9f6bf68ffeb90ca7a793a / fb7434eaaf6c52604541322d7e0fde58, so that the GPU tests can use them too) through the HIP sources
    on the emulator, vs the oracle that oracle/make_golden.py pins bit-exact against the reference's aliked.py with the same files.  Real
    weights have the trained dynamic range (BatchNorm scales, score head) that the seeded synthetic ones lack."""
    path = Path(__file__).parent / "assets" / f"{model}.pth"
    if not path.exists():
        pytest.skip(f"{model}.pth asset not present")
    weights = importlib.import_module("deep-image-matching_amd.weights")
    sd = weights.load_aliked_state_dict(str(path), model_name=model)
    cfg = {"model_name": model, "max_num_keypoints": 200, "detection_threshold": 0.2, "nms_radius": 2}
    yy, xx = torch.meshgrid(torch.arange(64.0), torch.arange(96.0), indexing="ij")
    img = (0.5 + 0.25 * torch.sin(xx / 5.0) * torch.cos(yy / 7.0))[None, None].repeat(1, 3, 1, 1) \
        + 0.2 * torch.rand(1, 3, 64, 96, generator=torch.Generator().manual_seed(3))
    img = img.clamp(0, 1)
    net = al_mod.AlikedHIP(sd, cfg, max_batch=1, max_hw=(64, 96), capacity=4096, device="cpu", lib=emu_lib)
    out = {k: v.cpu() for k, v in net(img).items()}
    ref = aliked_ref.aliked_forward(img, sd, cfg, taps=True)
    taps = net.debug_taps()
    pt, pl = taps["pad"]
    fm = torch.nn.functional.normalize(taps["x1234"][0, pt:pt + 64, pl:pl + 96].permute(2, 0, 1), dim=0)
    assert (fm - ref["feature_map"][0]).abs().max().item() < 1e-3
    res = compare_aliked(out, ref)
    assert res["n_out"] >= 8   # (the n32 checkpoint finds 9 keypoints on this 64 x 96 pattern, n16rot 37)
