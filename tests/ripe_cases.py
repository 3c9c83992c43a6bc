"""Shared by the emulator and the GPU tests of the RIPE extractor (tests/test_ripe_emu.py, tests/test_ripe_gpu.py).  Every case takes
(lib, device): the emulator build with "cpu", or the gfx950 library with "cuda".

Weights are seeded synthetic ones (weights.synthetic_ripe_state_dict: ripe_weights.pth is downloaded by the reference at run time).
tests/golden/ripe_<case>.npz hold the REFERENCE MODULE's outputs on seeded images, the fp64 evaluation of tests/ripe_ref.py and the module's own
fp32 error against it (scripts/make_ripe_golden.py, which also asserts that tests/ripe_ref.py equals the module bit for bit).

Bounds.  Heat map, scores, descriptors: device error against fp64 <= 2 x the fp32 module's own error against fp64 on the same input.  The tie
tolerance of a case is 4 x the module's maximum heat-map error against fp64 as stored in its golden file.  Operator tests: device error against
fp64 torch <= 2 x fp32 torch's error against fp64 torch on the same operands.
"""
from __future__ import annotations

import functools
import importlib
import json
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

from tests import nn_ref, ripe_ref

rp_mod = importlib.import_module("deep-image-matching_amd.ripe_hip")
capi = importlib.import_module("deep-image-matching_amd.capi")
weights_mod = importlib.import_module("deep-image-matching_amd.weights")

HERE = Path(__file__).parent
GOLD = HERE / "golden"
PARITY = HERE.parent / "profiles" / "ripe_parity.json"
WEIGHT_SEED = 41
MAX_NEAR_TIE_SHARE = 0.02

# seeded uniform-noise images (0..255 integers); shape (H, W) = a 2-D gray image.  The depthwise and the detection kernels work on 16 x 16 tiles:
# "tiles" (72 x 88, levels 36 x 44, 18 x 22, 9 x 11) spans two or more of them in both directions with ragged edges at scales 1, 2 and 4.
GOLDEN_CASES = {
    "min": {"shape": (16, 16, 3), "seed": 1, "top_k": 4096, "threshold": 0.5},
    "odd": {"shape": (50, 75, 3), "seed": 2, "top_k": 4096, "threshold": 0.5},
    "tiles": {"shape": (72, 88, 3), "seed": 5, "top_k": 4096, "threshold": 0.5},
    "topk": {"shape": (72, 88, 3), "seed": 5, "top_k": 25, "threshold": 0.5},
    "gray": {"shape": (52, 70), "seed": 4, "top_k": 4096, "threshold": 0.5},
}


def image(case) -> np.ndarray:
    """uint8 image of the case."""
    rng = np.random.default_rng(case["seed"])
    return rng.integers(0, 256, size=case["shape"]).astype(np.uint8)


def to_tensor(img: np.ndarray) -> torch.Tensor:
    """RIPEExtractor._frame2tensor: [1, C, H, W] float32 in 0..1."""
    a = img[None, None] if img.ndim == 2 else img.transpose(2, 0, 1)[None]
    return torch.from_numpy(np.ascontiguousarray(a)).float().div_(255.0)


def to_nhwc(t: torch.Tensor) -> torch.Tensor:
    x = t[0].permute(1, 2, 0)
    return (x.repeat(1, 1, 3) if x.shape[2] == 1 else x).contiguous()[None]


@functools.lru_cache(maxsize=None)
def weights(seed: int = WEIGHT_SEED):
    return weights_mod.synthetic_ripe_state_dict(seed)


def record(label, **res):
    """Measured figures behind an assertion: profiles/ripe_parity.json, one entry per label (rewritten in place)."""
    try:
        data = json.loads(PARITY.read_text()) if PARITY.exists() else {}
        data[label] = {k: (v if isinstance(v, (int, float, str, bool)) else str(v)) for k, v in res.items()}
        PARITY.write_text(json.dumps(data, indent=1, sort_keys=True) + "\n")
    except OSError:
        pass


def make_net(lib, device, hw, top_k=4096, threshold=0.5, max_batch=1, capacity=None, sd=None, **cfg):
    return rp_mod.RipeHIP(sd if sd is not None else weights(), {"top_k": top_k, "threshold": threshold, **cfg}, max_batch=max_batch, max_hw=hw,
                          capacity=capacity, device=device, lib=lib)


def run(net, x, device):
    """x [1, H, W, 3] -> (feature dict on the CPU, range-guard total)."""
    capi.check(net.lib, net.lib.dim_saturation_reset(net._stream()))
    kp, sc, de, n = net.extract_batch(x.to(device))
    total, _ = capi.saturation(net.lib, net._stream(), reset=True)
    k = int(n[0].item())
    return {"keypoints": kp[0, :k].cpu(), "scores": sc[0, :k].cpu(), "descriptors": de[0, :k].cpu()}, total


# ---- near ties ---------------------------------------------------------------------------------------------------------------------------
def near_decisions(heat64, thr, tol):
    """Pixels of a heat map whose selection hangs on a near tie (tests/xfeat_cases.near_decisions for a 3 x 3 window): a (near) window maximum
    within tol of the threshold, or a (near) candidate whose window holds another value within tol of it.  Returns a bool map."""
    m = heat64.reshape(1, 1, *heat64.shape[-2:]).double()
    H, W = m.shape[-2:]
    pad = F.pad(m, (1, 1, 1, 1), value=-float("inf"))
    win = pad.unfold(2, 3, 1).unfold(3, 3, 1).reshape(H, W, 9)
    top = torch.topk(win, 2, dim=-1).values
    v = m[0, 0]
    is_max = v >= top[..., 0] - tol
    near_thr = is_max & ((v - thr).abs() <= tol)
    near_nb = is_max & (v > thr - tol) & ((top[..., 0] - top[..., 1]) <= tol)
    return near_thr | near_nb


def candidates(heat64, thr):
    """Values of the fp64 map's candidates, descending."""
    xy = ripe_ref.nms(heat64, thr)
    return torch.sort(heat64[xy[:, 1], xy[:, 0]], descending=True).values


def tie_budget(heat64, thr, top_k, tol):
    """(near map, cut or None, number of pixels at a near-tie decision: the cap on one-sided keypoints)."""
    near = near_decisions(heat64, thr, tol)
    cand = candidates(heat64, thr)
    cut = float(cand[top_k - 1]) if len(cand) > top_k else None
    n_cut = int(((cand - cut).abs() <= tol).sum()) - 1 if cut is not None else 0
    return near, cut, int(near.sum()) + max(0, n_cut)


def compare_ripe(out, ref, heat64, thr, top_k, tol, label=None):
    """Keypoints pair exactly (integer pixels), a bijection up to keypoints at a near-tie decision of the fp64 heat map (within tol of the threshold,
    of a 3 x 3 neighbour or of the top-k cut), whose number is capped by the count of such pixels; rows score-descending on both sides and out of
    place only within tol of each other in the fp64 map.  Returns (figures, index pairs)."""
    po = [(int(x), int(y)) for x, y in out["keypoints"].tolist()]
    pr = [(int(x), int(y)) for x, y in ref["keypoints"].tolist()]
    assert out["keypoints"].dtype == torch.float32 and bool((out["keypoints"] == out["keypoints"].round()).all())
    where = {p: j for j, p in enumerate(pr)}
    assert len(where) == len(pr) and len(set(po)) == len(po), "duplicate keypoints"
    pairs = [(i, where[p]) for i, p in enumerate(po) if p in where]
    only_out = [po[i] for i in sorted(set(range(len(po))) - {p[0] for p in pairs})]
    only_ref = [pr[j] for j in sorted(set(range(len(pr))) - {p[1] for p in pairs})]
    near, cut, budget = tie_budget(heat64, thr, top_k, tol)
    res = {"n_out": len(po), "n_ref": len(pr), "common": len(pairs), "one_sided": max(len(only_out), len(only_ref)), "near_tie_pixels": budget, "tie_tol": tol,
           "rows_out_of_place": len([1 for i, j in pairs if i != j])}
    if label is not None:
        record(label, **res)
    for x, y in only_out + only_ref:
        at_cut = cut is not None and abs(float(heat64[y, x]) - cut) <= tol
        assert bool(near[y, x]) or at_cut, ("a keypoint on one side only that is no near tie", (x, y), float(heat64[y, x]), res)
    assert res["one_sided"] <= budget, res
    assert bool((ref["scores"][1:] <= ref["scores"][:-1]).all()), "the reference rows are not score-descending"
    assert bool((out["scores"][1:] <= out["scores"][:-1]).all()), "the output rows are not score-descending"
    moved = [(float(heat64[po[i][1], po[i][0]]), float(heat64[pr[i][1], pr[i][0]])) for i, j in pairs if i != j and i < len(pr)]
    assert all(abs(a - b) <= tol for a, b in moved), ("score-descending order differs beyond near ties", moved[:5], res)
    ia = torch.tensor([p[0] for p in pairs], dtype=torch.long)
    ib = torch.tensor([p[1] for p in pairs], dtype=torch.long)
    return res, ia, ib


def _gold(name):
    g = np.load(GOLD / f"ripe_{name}.npz")
    return {k: torch.from_numpy(np.asarray(g[k])) for k in g.files}


# ---- 1. goldens ---------------------------------------------------------------------------------------------------------------------------
def golden(lib, device, name):
    case = GOLDEN_CASES[name]
    img, gold = image(case), _gold(name)
    assert np.array_equal(gold["image"].numpy(), img)
    t = to_tensor(img)
    H, W = img.shape[:2]
    thr, top_k = case["threshold"], case["top_k"]
    net = make_net(lib, device, (H, W), top_k=top_k, threshold=thr)
    out, sat = run(net, to_nhwc(t), device)
    assert sat == 0, f"range guard fired ({sat})"
    heat64 = gold["heat"].double() + gold["heat_res64"].double()
    err_mod = {k: float(gold[f"err_{k}"]) for k in ("heat", "scores", "descriptors")}
    tol = 4.0 * err_mod["heat"]
    assert 20 <= gold["keypoints"].shape[0] <= 200
    ref = {"keypoints": gold["keypoints"], "scores": gold["scores"], "descriptors": gold["descriptors"]}
    res, ia, ib = compare_ripe(out, ref, heat64, thr, top_k, tol, label=f"ripe_{name}_{device}_golden")
    assert res["near_tie_pixels"] < MAX_NEAR_TIE_SHARE * res["n_ref"], res   # a condition on the inputs, asserted where the golden is made as well
    assert out["descriptors"].shape == (res["n_out"], 256)
    heat_dev = net.debug_taps()["heat"][0]
    err = {"heat": (heat_dev.double() - heat64).abs().max().item(),
           "scores": (out["scores"][ia].double() - gold["scores64"][ib]).abs().max().item(),
           "descriptors": (out["descriptors"][ia].double() - gold["descriptors64"][ib]).abs().max().item()}
    print(f"ripe {name} {device}: " + ", ".join(f"{k} device {err[k]:.3e} / module {err_mod[k]:.3e}" for k in err) + f"; keypoints {res['n_out']} / {res['n_ref']}")
    record(f"ripe_{name}_{device}_vs_fp64", **{f"{k}_device": v for k, v in err.items()}, **{f"{k}_fp32_module": v for k, v in err_mod.items()})
    for k in err:
        assert err[k] <= 2.0 * err_mod[k], (k, err[k], err_mod[k])
    norms = out["descriptors"].double().norm(dim=1)
    assert float((norms - 1).abs().max()) < 1e-6


# ---- 2. batch, handle reuse, capacity, no candidate -----------------------------------------------------------------------------------------
def _noise(seed, hw):
    return to_nhwc(to_tensor(np.random.default_rng(seed).integers(0, 256, size=(*hw, 3)).astype(np.uint8)))


def _raw(net, xs, device):
    kp, sc, de, n = net.extract_batch(torch.cat(xs).contiguous().to(device))
    outs = []
    for b in range(len(xs)):
        k = int(n[b].item())
        outs.append((kp[b, :k].cpu().clone(), sc[b, :k].cpu().clone(), de[b, :k].cpu().clone()))
    return outs


def _same(a, b):
    return all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


def batch_and_reuse(lib, device):
    hw = (50, 75)
    xs = [_noise(s, hw) for s in (11, 12, 13)]
    three = _raw(make_net(lib, device, hw, max_batch=3), xs, device)
    singles = [_raw(make_net(lib, device, hw), [x], device)[0] for x in xs]
    counts = [len(s[0]) for s in singles]
    assert min(counts) >= 10 and len(set(counts)) > 1, counts
    assert all(_same(a, b) for a, b in zip(three, singles)), "a batch of 3 differs from the three single calls"
    small = xs[0][:, :24, :40].contiguous()
    net = make_net(lib, device, hw)
    first, mid, again = _raw(net, [xs[0]], device)[0], _raw(net, [small], device)[0], _raw(net, [xs[0]], device)[0]
    fresh_small = _raw(make_net(lib, device, (24, 40)), [small], device)[0]
    assert len(mid[0]) > 0
    assert _same(first, singles[0]) and _same(again, singles[0]) and _same(mid, fresh_small), "a reused handle differs from fresh handles"


def capacity_and_no_candidate(lib, device):
    import pytest

    hw = (24, 32)
    x = _noise(21, hw)
    full = _raw(make_net(lib, device, hw), [x], device)[0]
    assert len(full[0]) > 8
    # capacity below top_k: reported by the library, nothing is written
    net = make_net(lib, device, hw, top_k=64, capacity=8)
    with pytest.raises(capi.DimHipError, match="top_k 64"):
        net.extract_batch(x.to(device))
    # capacity = top_k below the candidate count: exactly the first rows
    cut = _raw(make_net(lib, device, hw, top_k=8, capacity=8), [x], device)[0]
    assert len(cut[0]) == 8 and _same(cut, tuple(t[:8] for t in full))
    # no candidate: the reference raises RuntimeError("No keypoints detected")
    net = make_net(lib, device, hw, threshold=1.0e6)
    kp, sc, de, n = net.extract_batch(x.to(device))
    assert int(n[0].item()) == 0
    with pytest.raises(RuntimeError, match="No keypoints detected"):
        net(x.permute(0, 3, 1, 2).contiguous())
    with pytest.raises(capi.DimHipError, match="threshold"):
        make_net(lib, device, hw, threshold=-0.5).extract_batch(x.to(device))


# ---- 3. operators ---------------------------------------------------------------------------------------------------------------------------
def _bound(dev, ref32, ref64, what):
    e_dev, e_ref = (dev.double() - ref64).abs().max().item(), (ref32.double() - ref64).abs().max().item()
    record(what, device=e_dev, fp32_torch=e_ref)
    assert e_dev <= 2.0 * e_ref, (what, e_dev, e_ref)
    return e_dev, e_ref


DW_SHAPES = [(64, 16, 16), (64, 3, 5), (512, 2, 2), (512, 1, 1), (128, 21, 37)]   # the last: two tiles in both directions, ragged


def op_dw5x5(lib, device, shape, batch=2):
    """Depthwise 5 x 5 + BatchNorm (a third of the gammas negative) + ReLU against fp64 torch."""
    C, H, W = shape
    g = torch.Generator().manual_seed(100 + C + H)
    x = torch.randn(batch, C, H, W, generator=g)
    w, b = torch.randn(C, 1, 5, 5, generator=g) * 0.3, 0.1 * torch.randn(C, generator=g)
    gamma = 0.6 + 0.8 * torch.rand(C, generator=g)
    gamma[1::3] *= -1.0
    beta, mean, var = 0.1 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)

    def ref(dt):
        y = F.conv2d(x.to(dt), w.to(dt), b.to(dt), padding=2, groups=C)
        return F.relu(F.batch_norm(y, mean.to(dt), var.to(dt), gamma.to(dt), beta.to(dt), False, 0.1, 1e-5))

    sc = gamma.double() / torch.sqrt(var.double() + 1e-5)
    wf = (w.double().reshape(C, 25) * sc[:, None]).t().contiguous().float()            # [25][C]
    bf = ((b.double() - mean.double()) * sc + beta.double()).float()
    out = rp_mod.dw5x5(x.permute(0, 2, 3, 1).contiguous().to(device), wf.to(device), bf.to(device), lib).cpu().permute(0, 3, 1, 2)
    r64 = ref(torch.float64)
    assert bool((r64 > 0).any()) and bool((r64 == 0).any())
    return _bound(out, ref(torch.float32), r64, f"ripe_op_dw5x5_{C}x{H}x{W}_{device}")


RESIZE_SHAPES = [((6, 9), (12, 18)), ((12, 18), (25, 37)), ((1, 1), (2, 3))]


def op_resize(lib, device, sizes, C):
    (h, w), (H, W) = sizes
    g = torch.Generator().manual_seed(200 + h + C)
    ld, off = C + 1, 1                                    # the decoder's layout: channel 0 is the logit, the context follows
    x = torch.randn(2, h, w, ld, generator=g)
    src = x[..., off:].permute(0, 3, 1, 2).contiguous()
    out = rp_mod.resize_bilinear(x.to(device), (H, W), off, C, lib).cpu().permute(0, 3, 1, 2)
    r64, r32 = (F.interpolate(src.to(dt), size=(H, W), mode="bilinear", align_corners=False) for dt in (torch.float64, torch.float32))
    assert out.shape == r64.shape
    return _bound(out, r32, r64, f"ripe_op_resize_{h}x{w}_to_{H}x{W}_c{C}_{device}")


def op_nms3(lib, device, hw=(21, 37)):
    """Crafted maps against the torch expression, as exact sets."""
    H, W = hw
    thr = 0.5

    def check(heat, expect=None):
        key = rp_mod.nms3(heat[None].contiguous().to(device), thr, lib).cpu()[0]
        ref = ripe_ref.nms(heat, thr)
        got = key.nonzero().flip(-1)
        assert {tuple(p) for p in got.tolist()} == {tuple(p) for p in ref.tolist()}, (got.tolist(), ref.tolist())
        assert torch.equal(key[key > 0], heat[key > 0])
        if expect is not None:
            assert {tuple(p) for p in got.tolist()} == expect, (got.tolist(), expect)

    base = torch.full((H, W), 0.25)
    a = base.clone()
    a[10, 10] = a[10, 11] = 0.75                         # a plateau of two equal adjacent maxima: both stay
    a[5, 20] = 0.5                                       # exactly the threshold: rejected
    a[15, 30] = 0.5000001
    check(a, {(10, 10), (11, 10), (30, 15)})
    b = base.clone()
    b[0, 0] = 0.9; b[0, W - 1] = 0.8; b[H - 1, 0] = 0.7; b[H - 1, W - 1] = 0.6   # corners
    b[0, 17] = 0.95; b[H - 1, 18] = 0.85; b[9, 0] = 0.65; b[11, W - 1] = 0.55    # borders
    b[16, 16] = 1.0; b[16, 15] = 0.99                    # across a tile edge: only the larger one
    check(b, {(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (17, 0), (18, H - 1), (0, 9), (W - 1, 11), (16, 16)})
    check(base)                                          # a flat map below the threshold: nothing
    check(torch.full((H, W), 0.75))                      # a flat map above it: every pixel
    g = torch.Generator().manual_seed(5)
    check(torch.randn(H, W, generator=g) + 0.5)


def op_hypercolumn(lib, device, hw=(50, 75)):
    """Level sizes with odd members; keypoints on the image corners (they land exactly on level corners) and inside."""
    H, W = hw
    g = torch.Generator().manual_seed(300)
    feats = [torch.randn(1, 64 << l, H >> l, W >> l, generator=g) for l in range(4)]
    kp = torch.tensor([[0, 0], [W - 1, H - 1], [W - 1, 0], [0, H - 1], [37, 21], [1, 1], [W - 2, H - 2], [40, 49], [74, 30], [13, 7]], dtype=torch.long)
    n, cap = kp.shape[0], 16
    kpf = torch.zeros(1, cap, 2)
    kpf[0, :n] = kp.float()
    rows = rp_mod.hypercolumn([f.permute(0, 2, 3, 1).contiguous().to(device) for f in feats], kpf.to(device), torch.tensor([n], dtype=torch.int32, device=device),
                              (H, W), lib).cpu()[0]
    r64 = ripe_ref.hypercolumns([f.double() for f in feats], kp, H, W)
    r32 = ripe_ref.hypercolumns(feats, kp, H, W)
    assert bool((rows[n:] == 0).all())
    off = 0
    for l, f in enumerate(feats):   # the corners are exact copies of the level's corner pixels
        c = f.shape[1]
        assert torch.equal(rows[0, off:off + c], f[0, :, 0, 0]) and torch.equal(rows[1, off:off + c], f[0, :, -1, -1]) and torch.equal(rows[2, off:off + c], f[0, :, 0, -1])
        off += c
    return _bound(rows[:n], r32, r64, f"ripe_op_hypercolumn_{device}")


# ---- 4. the matcher chain -----------------------------------------------------------------------------------------------------------------
def shifted_pair():
    """Two 64 x 80 crops of one smooth-plus-noise scene, shifted by (8, 8)."""
    rng = np.random.default_rng(31)
    coarse = torch.from_numpy(rng.random((1, 3, 14, 16)).astype(np.float32))
    base = F.interpolate(coarse, size=(112, 128), mode="bicubic", align_corners=False)[0].permute(1, 2, 0).numpy()
    scene = np.clip(255.0 * (0.75 * base + 0.25 * rng.random((112, 128, 3))), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(scene[10:74, 12:92]), np.ascontiguousarray(scene[18:82, 20:100]), np.array([8.0, 8.0])


CHAIN_CONF = {"general": {}, "extractor": {"name": "ripe", "max_keypoints": 4096, "detect_threshold": 0.5, "allow_synthetic_weights": True},
              "matcher": {"name": "kornia_matcher", "match_mode": "smnn", "th": 0.95}}   # the reference's "ripe+kornia_matcher" entry


def chain(device):
    """RIPEExtractor._extract -> KorniaMatcher._match_pairs (the library the package loader returns) on the shifted pair: the share of matches at
    the true shift against the fp32 restatement's share through nn_ref, less the share of that pair's near ties."""
    plugins = importlib.import_module("deep-image-matching_amd.plugins")
    a, b, shift = shifted_pair()
    ex, mt = plugins.RIPEExtractor(CHAIN_CONF), plugins.KorniaMatcher(CHAIN_CONF)
    assert ex._default_conf == {"name": "ripe", "max_keypoints": 4000, "detect_threshold": 0.5}
    assert ex.required_inputs == [] and ex.grayscale is False and ex.descriptor_size == 128
    f0, f1 = ex._extract(a), ex._extract(b)
    for f in (f0, f1):
        n = f["keypoints"].shape[0]
        assert n > 20 and f["keypoints"].dtype == np.float32 and f["descriptors"].shape == (256, n) and f["scores"].shape == (n,)
    got = mt._match_pairs(f0, f1)
    k0, k1 = f0["keypoints"], f1["keypoints"]
    share = float(np.mean(np.abs(k0[got[:, 0]] - k1[got[:, 1]] - shift).max(axis=1) < 0.5)) if len(got) else 0.0
    sd = weights_mod.synthetic_ripe_state_dict(WEIGHT_SEED)
    refs, near = [], 0
    for img in (a, b):
        t = to_tensor(img)
        r = ripe_ref.ripe_forward(t, sd, torch.float32, 0.5, 4096)
        h64, _ = ripe_ref.heat_map(t, sd, torch.float64)
        near += tie_budget(h64, 0.5, 4096, 4.0 * float((r["heat"].double() - h64).abs().max()))[2]
        refs.append(r)
    d0, d1 = refs[0]["descriptors"], refs[1]["descriptors"]
    d2 = nn_ref.d2_fp64(d0, d1)
    must, may = nn_ref.classify_fp64(d0, d1, "smnn", 0.95, nn_ref.measured_tol(d0, d1, d2), d2)
    rk0, rk1 = refs[0]["keypoints"].numpy(), refs[1]["keypoints"].numpy()
    prs = [tuple(p) for p in must] + [tuple(p) for p in may]
    ref_share = sum(1 for i, j in prs if np.abs(rk0[i] - rk1[j] - shift).max() < 0.5) / max(1, len(prs))
    slack = (len(may) + near) / max(1, len(prs))
    print(f"ripe chain {device}: share at the true shift {share:.4f} ({len(got)} matches), reference {ref_share:.4f} ({len(prs)}), near-tie share {slack:.4f}")
    record(f"ripe_chain_{device}", share=share, matches=int(len(got)), reference_share=ref_share, reference_matches=len(prs), near_tie_share=slack)
    assert got.dtype == np.int64 and len(got) >= 10 and len(prs) >= 10
    assert share >= ref_share - slack, (share, ref_share, slack)
