"""Shared by the emulator and the GPU tests of the ALIKE extractor (tests/test_alike_emu.py, tests/test_alike_gpu.py).  Every case takes
(lib, device): the emulator build with "cpu", or the gfx950 library with "cuda".

Inputs are crops of tests/assets/config1/sacre_coeur_A.jpg (480 x 640, decoded with PIL); weights are the trained checkpoints
tests/golden/alike/alike-{t,s,n,l}.pth.<i> — byte copies of the reference's thirdparty/alike/models/*.pth (plain state dicts of tensors: data
files), cut into parts of at most PART bytes because no file of this repository may exceed 1 MiB; the parts are joined in memory and the md5 of
the whole (ALIKE_MD5 below) is checked on load.  They are distributed under the ALIKE licence (BSD 3-Clause, Copyright (c) 2022, Zhao Xiaoming;
thirdparty/alike/LICENSE in the reference tree).

The references: tests/golden/alike_<case>.npz hold the REFERENCE MODULES' outputs (scripts/make_alike_golden.py, which also asserts that
tests/alike_ref.py equals those modules bit for bit); everything else is compared against tests/alike_ref.py.
"""
from __future__ import annotations

import functools
import hashlib
import importlib
from pathlib import Path

import numpy as np
import torch

from tests import alike_ref, nn_ref

ak_mod = importlib.import_module("deep-image-matching_amd.alike_hip")
capi = importlib.import_module("deep-image-matching_amd.capi")
weights_mod = importlib.import_module("deep-image-matching_amd.weights")
nn_mod = importlib.import_module("deep-image-matching_amd.nn_hip")

HERE = Path(__file__).parent
GOLD = HERE / "golden"
PART = 1000000
ALIKE_MD5 = {"alike-t": "c3c95bdaf94374ad63ba9732b30f3f42", "alike-s": "e760838803f8678f0eb1c6b5bb947dc3",
             "alike-n": "6b740ef6061b140bc160494deed96987", "alike-l": "a23f181c1840a102f033df37747ebd81"}
TIE_TOL = 2e-5   # the project's near-tie bar (tests/test_aliked_emu.py compare_aliked)
MAX_NEAR_TIES = 4

GOLDEN_CASES = {
    # 75 x 110 is padded to 96 x 128: 3 x 4 cells at 1/32, every pyramid level present
    "t_pad": {"cfg": {"model": "alike-t", "top_k": -1, "scores_th": 0.2, "n_limit": 5000}, "crop": (200, 275, 300, 410), "n": 90},
    "s_topk": {"cfg": {"model": "alike-s", "top_k": 64, "scores_th": 0.2, "n_limit": 5000}, "crop": (200, 296, 300, 428), "n": 64},
    "n_limit": {"cfg": {"model": "alike-n", "top_k": -1, "scores_th": 0.2, "n_limit": 40}, "crop": (200, 296, 300, 428), "n": 40},
    "l_head": {"cfg": {"model": "alike-l", "top_k": -1, "scores_th": 0.2, "n_limit": 5000}, "crop": (200, 296, 300, 428), "n": 90},
}


@functools.lru_cache(maxsize=None)
def photo() -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.open(HERE / "assets" / "config1" / "sacre_coeur_A.jpg").convert("RGB"))


def crop(case) -> np.ndarray:
    y0, y1, x0, x1 = case["crop"]
    return photo()[y0:y1, x0:x1].copy()


@functools.lru_cache(maxsize=None)
def weights(model: str):
    return weights_mod.load_alike_state_dict(checkpoint_file(model), model)


def checkpoint_file(model: str):
    """The checkpoint's bytes, joined from its parts and verified, as a file object torch.load accepts."""
    import io
    parts = sorted((GOLD / "alike").glob(f"{model}.pth.*"), key=lambda p: int(p.suffix[1:]))
    data = b"".join(p.read_bytes() for p in parts)
    assert hashlib.md5(data).hexdigest() == ALIKE_MD5[model], f"{model}.pth: the parts under tests/golden/alike do not add up to the checkpoint"
    return io.BytesIO(data)


@functools.lru_cache(maxsize=None)
def _reference(model, top_k, scores_th, n_limit, crop_key, dtype_name="float32"):
    """alike_ref on a crop of the photograph, computed once and shared (treat as read-only)."""
    y0, y1, x0, x1 = crop_key
    cfg = {"model": model, "top_k": top_k, "scores_th": scores_th, "n_limit": n_limit}
    return alike_ref.alike_forward(np.ascontiguousarray(photo()[y0:y1, x0:x1]), weights(model), cfg, taps=True, dtype=getattr(torch, dtype_name))


def reference(cfg, crop_key, dtype_name="float32"):
    return _reference(cfg["model"], int(cfg["top_k"]), float(cfg["scores_th"]), int(cfg["n_limit"]), tuple(crop_key), dtype_name)


def record(label, **res):
    """Measured figures behind an assertion go where the suite keeps them (the recorder of tests/test_aliked_gpu.py: parity_measured.jsonl)."""
    from tests.test_aliked_gpu import _record
    _record({"case": label, **{k: (v if isinstance(v, (int, float, str, bool)) else str(v)) for k, v in res.items()}})


def make_net(lib, device, cfg, hw, max_batch=1, capacity=None):
    return ak_mod.AlikeHIP(weights(cfg["model"]), dict(cfg), max_batch=max_batch, max_hw=hw, capacity=capacity, device=device, lib=lib)


def run(net, img_u8, device):
    """One uint8 H x W x 3 image through extract_batch with the range-guard counters read: (feature dict on the CPU, guard total)."""
    x = (torch.from_numpy(img_u8).to(torch.float32) / 255.0)[None].contiguous().to(device)
    capi.check(net.lib, net.lib.dim_saturation_reset(net._stream()))
    kp, sc, de, n = net.extract_batch(x)
    total, sites = capi.saturation(net.lib, net._stream(), reset=True)
    k = int(n[0].item())
    return {"keypoints": kp[0, :k].cpu(), "scores": sc[0, :k].cpu(), "descriptors": de[0, :k].t().cpu()}, total


def selection_cut(ref_score_map, cfg):
    """(cut, threshold, nms map) of the REFERENCE's selection on its own score map: the weakest selected maximum (top-k / n_limit) or the threshold."""
    sm = ref_score_map.reshape(1, 1, *ref_score_map.shape[-2:])
    nms = alike_ref.nms_map(sm)[0, 0]
    if cfg["top_k"] > 0:
        cand = torch.sort(nms[nms > 0], descending=True).values
        thr = 0.0
        cut = float(cand[cfg["top_k"] - 1]) if len(cand) >= cfg["top_k"] else 0.0
    else:
        thr = float(cfg["scores_th"])
        if thr <= 0 or int((nms > thr).sum()) == 0:
            thr = float(sm.mean())
        cand = torch.sort(nms[nms > thr], descending=True).values
        cut = float(cand[cfg["n_limit"] - 1]) if len(cand) > cfg["n_limit"] else thr
    return cut, thr, nms


def reference_row_values(ref, ref_score_map):
    """The NMS value behind every reference row: the raw score at its selected pixel (tests/alike_ref.py hands the pixel indices out), or — for a
    golden, which holds keypoints only — the local maximum next to the refined position."""
    sm = ref_score_map.reshape(*ref_score_map.shape[-2:])
    if "indices" in ref:
        return sm.reshape(-1)[ref["indices"]].double()
    kr = ref["keypoints"].numpy().astype(np.float64)
    return torch.tensor([float(sm[max(0, int(round(y)) - 1): int(round(y)) + 2, max(0, int(round(x)) - 1): int(round(x)) + 2].max()) for x, y in kr],
                        dtype=torch.float64)


def compare_alike(out, ref, cfg=None, ref_score_map=None, label=None, tol=1e-3, max_one_sided=0, order=None):
    """Keypoints paired by nearest neighbour within 0.05 px (a bijection); values within `tol`.  A keypoint present on one side only must sit, in
    the REFERENCE's score map, within TIE_TOL of the selection cut, of the threshold, or of another pixel of its 5 x 5 NMS window.
    ``order``: "sorted" (top-k, the n_limit cut: score-descending) — output row i must pair with reference row i; it may pair with another row j
    only when the reference's NMS values of rows i and j differ by at most TIE_TOL (an order the reference's own arithmetic does not pin);
    "row_major" (threshold mode below n_limit) — output row i pairs with reference row i; the paired rows keep their order in any case."""
    from scipy.spatial import cKDTree
    ko, kr = out["keypoints"].numpy().astype(np.float64), ref["keypoints"].numpy().astype(np.float64)
    pairs, used = [], set()
    if len(ko) and len(kr):
        dist, nn = cKDTree(kr).query(ko)
        for i, (d, j) in enumerate(zip(dist, nn)):
            if d <= 0.05 and int(j) not in used:
                used.add(int(j)); pairs.append((i, int(j)))
    ia = torch.tensor([p[0] for p in pairs], dtype=torch.long); ib = torch.tensor([p[1] for p in pairs], dtype=torch.long)
    only_out = sorted(set(range(len(ko))) - {p[0] for p in pairs}); only_ref = sorted(set(range(len(kr))) - used)
    res = {"n_out": len(ko), "n_ref": len(kr), "common": len(pairs), "one_sided": max(len(only_out), len(only_ref))}
    res["kp"] = (out["keypoints"][ia] - ref["keypoints"][ib]).abs().max().item() if pairs else 0.0
    res["score"] = (out["scores"][ia] - ref["scores"][ib]).abs().max().item() if pairs else 0.0
    res["desc"] = (out["descriptors"][:, ia] - ref["descriptors"][:, ib]).abs().max().item() if pairs else 0.0
    if label is not None:
        record(label, **res)
    if only_out or only_ref:
        assert ref_score_map is not None and cfg is not None, res
        cut, thr, _ = selection_cut(ref_score_map, cfg)
        sm = ref_score_map.reshape(*ref_score_map.shape[-2:])
        for xy in [ko[i] for i in only_out] + [kr[j] for j in only_ref]:
            x, y = int(round(xy[0])), int(round(xy[1]))
            v = float(sm[max(0, y - 1): y + 2, max(0, x - 1): x + 2].max())   # the NMS pixel of a refined keypoint: the local maximum next to it
            top = torch.topk(sm[max(0, y - 2): y + 3, max(0, x - 2): x + 3].reshape(-1), 2).values
            assert min(abs(v - cut), abs(v - thr), float(top[0] - top[1])) <= TIE_TOL, (tuple(xy), v, cut, thr, res)
    assert len(ko) == len(kr) and res["one_sided"] <= max_one_sided, res
    if order == "row_major":
        js = [j for _, j in pairs]      # (pairs are in output-row order; a near-tie row present on one side only shifts the rest by one)
        assert js == sorted(js) and (res["one_sided"] > 0 or all(i == j for i, j in pairs)), ("row-major order differs", [q for q in pairs if q[0] != q[1]][:5], res)
    elif order == "sorted":
        assert ref_score_map is not None
        v = reference_row_values(ref, ref_score_map)
        assert bool((v[1:] <= v[:-1]).all()) or "indices" not in ref, "the reference rows are not score-descending"
        moved = [(i, j, float(v[i]), float(v[j])) for i, j in pairs if i != j]
        res["rows_out_of_place"] = len(moved)
        assert all(abs(a - b) <= TIE_TOL for _, _, a, b in moved), ("score-descending order differs beyond near ties", moved[:5], res)
    else:
        assert order is None, order
    assert res["kp"] <= tol and res["score"] <= tol and res["desc"] <= tol, res
    return res


def _gold(name):
    g = np.load(GOLD / f"alike_{name}.npz")
    return {k: torch.from_numpy(g[k]) for k in ("keypoints", "scores", "descriptors", "score_map")}, g["image"]


# ---- 1. goldens ---------------------------------------------------------------------------------------------------------------------------
def golden(lib, device, name):
    case = GOLDEN_CASES[name]
    cfg, img = case["cfg"], crop(case)
    gold, gold_img = _gold(name)
    assert np.array_equal(gold_img, img)
    H, W = img.shape[:2]
    net = make_net(lib, device, cfg, (H, W), capacity=max(cfg["top_k"], 0) or cfg["n_limit"])
    out, sat = run(net, img, device)
    assert sat == 0, f"range guard fired ({sat}) on trained weights"
    assert out["keypoints"].shape[0] == case["n"] == gold["keypoints"].shape[0]
    ref = reference(cfg, case["crop"])
    # (restatement == module bit for bit is asserted where the golden is made, scripts/make_alike_golden.py: torch's CPU kernels differ from
    # host to host in the last bit, so here the two are only close)
    assert (ref["score_map"][0, 0] - gold["score_map"]).abs().max().item() <= 1e-5
    # order: row-major (threshold mode with fewer survivors than n_limit) or score-descending (top-k, the n_limit cut)
    order = "row_major" if cfg["top_k"] <= 0 and case["n"] < cfg["n_limit"] else "sorted"
    compare_alike(out, gold, cfg, gold["score_map"], label=f"alike_{name}_{device}_golden", order=order)
    compare_alike(out, ref, cfg, ref["score_map"], order=order)
    # score map against fp64: at most twice the fp32 restatement's own error on the same input
    tap = net.debug_taps()["score_map"][0].double()
    sm64 = reference(cfg, case["crop"], "float64")["score_map"][0, 0]
    err_dev = (tap - sm64).abs().max().item()
    err_ref = (ref["score_map"][0, 0].double() - sm64).abs().max().item()
    print(f"alike {name} {device}: score map max abs error vs fp64: device {err_dev:.3e}, fp32 restatement {err_ref:.3e}")
    record(f"alike_{name}_{device}_score_map_vs_fp64", device=err_dev, fp32_restatement=err_ref)
    assert err_dev <= 2.0 * err_ref, (err_dev, err_ref)


# ---- 2. trained weights at a realistic size -----------------------------------------------------------------------------------------------
REAL_CROP = (0, 300, 0, 410)


def trained_realistic(lib, device, model):
    cfg = {"model": model, "top_k": -1, "scores_th": 0.2, "n_limit": 400}
    img = crop({"crop": REAL_CROP})
    net = make_net(lib, device, cfg, img.shape[:2], capacity=400)
    out, sat = run(net, img, device)
    assert sat == 0, f"range guard fired ({sat})"
    ref = reference(cfg, REAL_CROP)
    assert ref["keypoints"].shape[0] == 400 and out["keypoints"].shape[0] == 400
    res = compare_alike(out, ref, cfg, ref["score_map"], label=f"alike_real_{model}_{device}", max_one_sided=MAX_NEAR_TIES, order="sorted")
    assert res["one_sided"] <= MAX_NEAR_TIES


# ---- 3. deep-image-matching's default configuration ---------------------------------------------------------------------------------------
def dim_default(lib, device):
    cfg = {"model": "alike-s", "top_k": 15000, "scores_th": 0.2, "n_limit": 15000}
    full = (0, 480, 0, 640)
    img = crop({"crop": full})
    net = make_net(lib, device, cfg, (480, 640))
    out, sat = run(net, img, device)
    assert sat == 0
    ref = reference(cfg, full)
    assert out["descriptors"].shape == (96, 15000) and ref["keypoints"].shape[0] == 15000
    cut, _, nms = selection_cut(ref["score_map"], cfg)
    assert int((nms > 0).sum()) > 15000                      # no zero fill on this image
    near_cut = int(((nms > 0) & ((nms - cut).abs() <= TIE_TOL)).sum())
    res = compare_alike(out, ref, cfg, ref["score_map"], label=f"alike_dim_default_{device}", max_one_sided=near_cut, order="sorted")
    record(f"alike_dim_default_{device}_ties", near_cut=near_cut, one_sided=res["one_sided"])


# ---- 4. zero fill -------------------------------------------------------------------------------------------------------------------------
def zero_fill(lib, device):
    case = GOLDEN_CASES["s_topk"]
    cfg = {"model": "alike-t", "top_k": 1000, "scores_th": 0.2, "n_limit": 5000}
    img = crop(case)
    H, W = img.shape[:2]
    ref_all = reference({**cfg, "top_k": -1, "scores_th": 0.0}, case["crop"])          # (only its maps are used)
    nms = ref_all["nms_map"][0, 0].reshape(-1)
    maxima = (nms > 0).nonzero()[:, 0]
    n_pos = len(maxima)
    assert 500 < n_pos < 1000, n_pos
    # the library's documented fill rule: the first non-candidate pixels in row-major order
    idx = torch.cat([maxima[torch.sort(nms[maxima], descending=True, stable=True)[1]], (nms <= 0).nonzero()[: 1000 - n_pos, 0]])
    ref = alike_ref.alike_forward(img, weights("alike-t"), cfg, taps=True, idx=idx)
    net = make_net(lib, device, cfg, (H, W))
    out, sat = run(net, img, device)
    assert sat == 0 and out["keypoints"].shape[0] == 1000
    part = lambda d, a, b: {k: (d[k][:, a:b] if k == "descriptors" else d[k][a:b]) for k in ("keypoints", "scores", "descriptors")}  # noqa: E731
    # the first n_pos rows: the reference's first n_pos, in its (score-descending) order
    compare_alike(part(out, 0, n_pos), {**part(ref, 0, n_pos), "indices": idx[:n_pos]}, {**cfg, "top_k": n_pos}, ref["score_map"],
                  label=f"alike_zero_fill_{device}", order="sorted")
    # the fill rows, in order: the reference's arithmetic at those pixels, each of them a zero of the library's own NMS map
    for k in ("keypoints", "scores"):
        assert (out[k][n_pos:] - ref[k][n_pos:]).abs().max().item() <= 1e-3, k
    assert (out["descriptors"][:, n_pos:] - ref["descriptors"][:, n_pos:]).abs().max().item() <= 1e-3
    tap = net.debug_taps()["nms_map"][0].reshape(-1)
    assert (tap[idx[n_pos:]] == 0).all() and int((tap > 0).sum()) == n_pos


# ---- 5. mean-threshold fallback -----------------------------------------------------------------------------------------------------------
def mean_threshold(lib, device, scores_th):
    case = GOLDEN_CASES["s_topk"]
    cfg = {"model": "alike-t", "top_k": -1, "scores_th": scores_th, "n_limit": 5000}
    img = crop(case)
    ref = reference(cfg, case["crop"])
    if scores_th > 0:
        assert int((ref["nms_map"] > scores_th).sum()) == 0     # nothing passes: the mean takes over
    assert ref["keypoints"].shape[0] > 100
    net = make_net(lib, device, cfg, img.shape[:2])
    out, _ = run(net, img, device)
    compare_alike(out, ref, cfg, ref["score_map"], label=f"alike_mean_{scores_th}_{device}", max_one_sided=MAX_NEAR_TIES, order="row_major")


# ---- 6. batch and handle reuse ------------------------------------------------------------------------------------------------------------
def _raw(net, imgs, device):
    x = torch.stack([torch.from_numpy(i).to(torch.float32) / 255.0 for i in imgs]).contiguous().to(device)
    kp, sc, de, n = net.extract_batch(x)
    outs = []
    for b in range(len(imgs)):
        k = int(n[b].item())
        outs.append((kp[b, :k].cpu().clone(), sc[b, :k].cpu().clone(), de[b, :k].cpu().clone()))
    return outs


def _same(a, b):
    return all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


def batch_and_reuse(lib, device, model="alike-n", big=False):
    cfg = {"model": model, "top_k": -1, "scores_th": 0.2, "n_limit": 300}
    if big:
        a, b = crop({"crop": (0, 300, 0, 410)}), crop({"crop": (100, 400, 200, 610)})
    else:
        a, b = crop({"crop": (200, 296, 300, 428)}), crop({"crop": (300, 396, 100, 228)})
    hw = a.shape[:2]
    two = _raw(make_net(lib, device, cfg, hw, max_batch=2, capacity=300), [a, b], device)
    one_a = _raw(make_net(lib, device, cfg, hw, capacity=300), [a], device)[0]
    one_b = _raw(make_net(lib, device, cfg, hw, capacity=300), [b], device)[0]
    assert len(one_a[0]) > 20 and len(one_b[0]) > 20
    assert _same(two[0], one_a) and _same(two[1], one_b), "a batch of 2 differs from the two single calls"
    if not big:
        small = crop(GOLDEN_CASES["t_pad"])                 # 75 x 110 inside the same 96 x 128 padded frame: stale padded-frame scratch
        net = make_net(lib, device, cfg, hw, capacity=300)
        first, mid, again = _raw(net, [a], device)[0], _raw(net, [small], device)[0], _raw(net, [a], device)[0]
        fresh_small = _raw(make_net(lib, device, cfg, hw, capacity=300), [small], device)[0]
        assert _same(first, one_a) and _same(again, one_a) and _same(mid, fresh_small), "a reused handle differs from fresh handles"


# ---- 7. desc_stride and the nearest-neighbour matcher -------------------------------------------------------------------------------------
def desc_stride_and_matcher(lib, device):
    cfg = {"model": "alike-s", "top_k": -1, "scores_th": 0.2, "n_limit": 300, "desc_stride": 128}
    a, b = crop({"crop": (200, 296, 300, 428)}), crop({"crop": (216, 312, 324, 452)})     # shifted by (16, 24)
    net = make_net(lib, device, cfg, a.shape[:2], max_batch=2, capacity=300)
    x = torch.stack([torch.from_numpy(i).to(torch.float32) / 255.0 for i in (a, b)]).contiguous().to(device)
    out = (torch.zeros(2, 300, 2, device=device), torch.zeros(2, 300, device=device), torch.zeros(2, 300, 128, device=device),
           torch.zeros(2, dtype=torch.int32, device=device))
    kp, sc, de, n = net.extract_batch(x, out=out)
    n0, n1 = int(n[0].item()), int(n[1].item())
    assert n0 > 30 and n1 > 30 and de.shape == (2, 300, 128)
    assert (de[0, :n0, 96:] == 0).all() and (de[1, :n1, 96:] == 0).all()
    d0, d1 = de[0, :n0, :96].cpu(), de[1, :n1, :96].cpu()
    assert (d0.norm(dim=1) - 1).abs().max().item() < 1e-5
    matcher = nn_mod.NearestNeighborHIP("smnn", 0.95, dim=128, max_pairs=1, max_kpts=300, device=device, lib=lib)
    m = matcher.match_batch_guarded(kp, de, n)
    got = m["matches"][0, : int(m["n_matches"][0].item())].cpu().numpy()
    d2 = nn_ref.d2_fp64(d0, d1)
    must, may = nn_ref.classify_fp64(d0, d1, "smnn", 0.95, nn_ref.measured_tol(d0, d1, d2), d2)
    assert len(must) >= 5, len(must)
    nn_ref.check_rule(got, must, may, "alike-s 96-d descriptors padded to 128")
