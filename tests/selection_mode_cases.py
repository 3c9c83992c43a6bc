"""Shared by the emulator and the GPU tests: the selection modes of the extractors that only crafted configurations reach — DKD's top-k mode
with and without zero fill, its mean-score threshold, more than 4096 keypoints, SuperPoint's keep-all regrow.  Every case takes (lib, device): the
emulator build with "cpu", or the gfx950 library with "cuda"."""
from __future__ import annotations

import importlib

import numpy as np
import torch

from oracle import aliked_ref, superpoint_ref
from tests import golden_cases as gc

al_mod = importlib.import_module("deep-image-matching_amd.aliked_hip")
plugins = importlib.import_module("deep-image-matching_amd.plugins")


def compare_aliked(*args, **kw):
    from tests.test_aliked_emu import compare_aliked as compare   # (that module imports this one)
    return compare(*args, **kw)


def aliked_top_k_mode_vs_oracle(lib, device):
    """detection_threshold <= 0 = DKD's top-k mode (ALN:602, 150-151): the max_num_keypoints highest NMS maxima, whatever their score."""
    case = gc.AL_CASES["rgb_pad"]
    cfg = {**case["cfg"], "detection_threshold": -1.0, "max_num_keypoints": 50}
    sd, img = gc.al_weights(case), gc.al_image(case)
    net = al_mod.AlikedHIP(sd, cfg, max_batch=1, max_hw=(case["H"], case["W"]), capacity=64, device=device, lib=lib)
    out = {k: v.cpu() for k, v in net(img.to(device)).items()}
    ref = aliked_ref.aliked_forward(img, sd, cfg, taps=True)
    assert ref["keypoints"].shape[0] == 50
    res = compare_aliked(out, ref, ref_score_map=ref["score_map"], threshold=0.0, nms_radius=cfg["nms_radius"], n_limit=50)
    assert res["n_out"] == 50
    # with the default threshold the same image keeps 336 keypoints (golden rgb_pad): the 50 are its highest maxima, none below 0.2 is needed
    thr = {**cfg, "detection_threshold": 0.2}
    net2 = al_mod.AlikedHIP(sd, thr, max_batch=1, max_hw=(case["H"], case["W"]), capacity=64, device=device, lib=lib)
    out2 = {k: v.cpu() for k, v in net2(img.to(device)).items()}
    assert {tuple(r) for r in out["keypoints"].round().int().tolist()} == {tuple(r) for r in out2["keypoints"].round().int().tolist()}


def aliked_mean_threshold_mode_vs_oracle(lib, device):
    """detection_threshold <= 0 AND max_num_keypoints <= 0: the reference's top_k is then <= 0 and DKD keeps every NMS maximum above
    the image's MEAN score (ALN:161-163) — at most n_limit_max = 20000 of them (ALN:571), which is the slot size of the keep-all modes."""
    case = gc.AL_CASES["rgb_pad"]
    cfg = {**case["cfg"], "detection_threshold": -1.0, "max_num_keypoints": -1}
    sd, img = gc.al_weights(case), gc.al_image(case)
    net = al_mod.AlikedHIP(sd, cfg, max_batch=1, max_hw=(case["H"], case["W"]), device=device, lib=lib)
    assert net.capacity == aliked_ref.N_LIMIT_MAX == 20000
    out = {k: v.cpu() for k, v in net(img.to(device)).items()}
    ref = aliked_ref.aliked_forward(img, sd, cfg, taps=True)
    mean = float(ref["score_map"].mean())
    assert ref["keypoints"].shape[0] > 100
    res = compare_aliked(out, ref, ref_score_map=ref["score_map"], threshold=mean, nms_radius=cfg["nms_radius"])
    assert res["n_out"] == ref["keypoints"].shape[0]


def _fill_reference(img, sd, cfg, ref_full, k):
    """What DKD's top-k mode returns when the image has FEWER NMS maxima than top_k (ALN:150-151), with the zero-score fill pixels fixed to
    the first non-maximum pixels in row-major order (which pixels torch.topk takes among the equal zeros is an accident of its sort: libstdc++'s
    heap / introselect on the CPU, a radix select on CUDA): the reference's arithmetic (oracle dkd_refine + SDDH) at those indices."""
    r = cfg["nms_radius"]
    nms = aliked_ref.dkd_nms_map(ref_full["score_map"], r).reshape(-1)
    maxima = (nms > 0).nonzero()[:, 0]
    order = torch.sort(nms[maxima], descending=True, stable=True)[1]
    fill = (nms <= 0).nonzero()[:k - len(maxima), 0]
    idx = torch.cat([maxima[order], fill])
    return aliked_ref.aliked_forward(img, sd, cfg, taps=True, idx=idx), len(maxima)


def aliked_top_k_mode_fills_up_with_zero_score_pixels(lib, device):
    """DKD's top-k mode on an image with fewer NMS maxima than max_num_keypoints: the reference's torch.topk still returns top_k indices — the
    maxima, score-descending, then zero-score pixels (ALN:150-151).  Count, order of the maxima and the values at every returned pixel must be
    the reference's; the fill pixels' identity is pinned to row-major order (see _fill_reference)."""
    case = gc.AL_CASES["rgb_pad"]
    sd, img = gc.al_weights(case), gc.al_image(case)
    base = {**case["cfg"], "detection_threshold": -1.0}
    ref_all = aliked_ref.aliked_forward(img, sd, {**base, "max_num_keypoints": -1}, taps=True)
    n_max = int((aliked_ref.dkd_nms_map(ref_all["score_map"], base["nms_radius"]) > 0).sum())
    k = n_max + 37
    cfg = {**base, "max_num_keypoints": k}
    ref_torch = aliked_ref.aliked_forward(img, sd, cfg)
    assert ref_torch["keypoints"].shape[0] == k          # the reference's count: top_k, not the number of maxima
    net = al_mod.AlikedHIP(sd, cfg, max_batch=1, max_hw=(case["H"], case["W"]), device=device, lib=lib)
    out = {kk: v.cpu() for kk, v in net(img.to(device)).items()}
    assert out["keypoints"].shape[0] == k
    ref, m = _fill_reference(img, sd, cfg, ref_all, k)
    assert m == n_max
    # the maxima: the reference's own torch.topk output (paired by position: near-equal scores may swap neighbours in the order)
    part = lambda d, a, b: {kk: d[kk][..., a:b] if kk == "descriptors" else d[kk][a:b] for kk in ("keypoints", "scores", "descriptors")}  # noqa: E731
    res = compare_aliked(part(out, 0, m), part(ref_torch, 0, m))
    assert res["common"] == m
    # the fill, in order
    assert (out["keypoints"][m:] - ref["keypoints"][m:]).abs().max().item() <= 1e-3
    assert (out["scores"][m:] - ref["scores"][m:]).abs().max().item() <= 1e-3
    assert (out["descriptors"][:, m:] - ref["descriptors"][:, m:]).abs().max().item() <= 1e-3
    # score-descending order of the maxima (torch.topk sorts).  The true keypoint scores are not exported (Q8): pair every output keypoint with
    # its twin in `ref` (whose maxima are in stable score-descending order) and read the NMS score there
    from scipy.spatial import cKDTree
    nms = aliked_ref.dkd_nms_map(ref_all["score_map"], base["nms_radius"]).reshape(-1)
    v_sorted = torch.sort(nms[nms > 0], descending=True, stable=True)[0]
    dist, twin = cKDTree(ref["keypoints"][:m].numpy().astype(np.float64)).query(out["keypoints"][:m].numpy().astype(np.float64))
    assert dist.max() <= 0.05 and len(set(twin.tolist())) == m
    v = v_sorted[torch.from_numpy(twin)]
    assert (v[1:] <= v[:-1] + 2e-5).all()


def aliked_more_than_4096_keypoints(lib, device):
    """config/aliked.yaml asks for max_num_keypoints 8000 and ALN:571 allows 20000: above 4096 the selection runs as radix select -> 4096-key
    chunk sorts -> rank merge (sp_post.hip).  128 x 192 noise at nms_radius 1 has ~4400 maxima: k = 4200 takes the select path (n > k), k = 5000
    the sort-everything + zero-fill path (n < k), both across two chunks."""
    case = gc.AL_CASES["rgb_pad"]
    sd = gc.al_weights(case)
    H, W = 128, 192
    img = torch.rand(1, 3, H, W, generator=torch.Generator().manual_seed(5))
    base = {**case["cfg"], "nms_radius": 1, "detection_threshold": -1.0}
    ref_all = aliked_ref.aliked_forward(img, sd, {**base, "max_num_keypoints": -1}, taps=True)
    n_max = int((aliked_ref.dkd_nms_map(ref_all["score_map"], 1) > 0).sum())
    assert 4200 < n_max < 5000, n_max
    for k in (4200, 5000):
        cfg = {**base, "max_num_keypoints": k}
        net = al_mod.AlikedHIP(sd, cfg, max_batch=1, max_hw=(H, W), device=device, lib=lib)
        out = {kk: v.cpu() for kk, v in net(img.to(device)).items()}
        assert out["keypoints"].shape[0] == k
        if k < n_max:
            ref = aliked_ref.aliked_forward(img, sd, cfg, taps=True)
            res = compare_aliked(out, ref, ref_score_map=ref["score_map"], threshold=0.0, nms_radius=1, n_limit=k)
            assert res["n_out"] == k and res["common"] >= k - 4, res
        else:
            ref, m = _fill_reference(img, sd, cfg, ref_all, k)
            res = compare_aliked({kk: v[..., :m] if kk == "descriptors" else v[:m] for kk, v in out.items()},
                                 {kk: ref[kk][..., :m] if kk == "descriptors" else ref[kk][:m] for kk in ("keypoints", "scores", "descriptors")},
                                 ref_score_map=ref_all["score_map"], threshold=0.0, nms_radius=1)
            assert res["common"] >= m - 4, res
            if res["common"] == m:   # identical maxima sets: the fill pixels are then the same row-major prefix on both sides
                assert (out["keypoints"][m:] - ref["keypoints"][m:]).abs().max().item() <= 1e-3
                assert (out["descriptors"][:, m:] - ref["descriptors"][:, m:]).abs().max().item() <= 1e-3


def keep_all_mode_never_drops_keypoints(lib, device):
    """with max_keypoints = -1 an image with more candidates than the slot is re-extracted with a larger
    slot, so every keypoint the reference returns is returned.  The plugin takes its library and device from the package loader (the
    emulator tests route it with the emu_install fixture); lib and device are only here for the common signature."""
    cfg = {"general": {}, "extractor": {"name": "superpoint", "nms_radius": 1, "keypoint_threshold": 0.0, "max_keypoints": -1,
                                        "remove_borders": 1, "allow_synthetic_weights": True}}
    ex = plugins.SuperPointExtractor(cfg)
    img = (torch.rand(48, 64, generator=torch.Generator().manual_seed(9)) * 255).numpy().astype(np.float32)
    ex._ensure(48, 64)
    ex._net = None
    ex._capacity = lambda H, W: max(ex._min_capacity, 64)   # force a slot that is too small for the first call
    f = ex._extract(img)
    ref = superpoint_ref.superpoint_forward(torch.tensor(img / 255.0, dtype=torch.float)[None, None], ex._sd, ex._net_cfg)
    assert ref["keypoints"].shape[0] > 64
    assert f["keypoints"].shape[0] == ref["keypoints"].shape[0]
    assert np.array_equal(f["keypoints"], ref["keypoints"].numpy())  # row-major order, like torch.nonzero
