"""Shared by the emulator and the GPU tests of the open SuperPoint extractor (tests/test_spopen_emu.py, tests/test_spopen_gpu.py).  Every case
takes (lib, device): the emulator build with "cpu", or the gfx950 library with "cuda".

The trained checkpoint (superpoint_v6_from_tf.pth) is not in this repository: everything runs on the seeded synthetic weights of
weights.synthetic_superpoint_open_state_dict, about 30 % of whose BatchNorm gammas are negative.  Inputs are seeded images built with integer
arithmetic only (the same bytes on every host).  The references are tests/golden/spopen_<case>.npz: the outputs and intermediate maps of the
REFERENCE's own network module on those weights and images, written by scripts/make_spopen_golden.py, which also evaluates the module in fp64
and asserts that every committed case has the same keypoints in fp32 and fp64 and that no fp64 score lies within 1e-4 of a decision.

Bounds (the project's own, from the SuperPoint tests): score map within 1e-5 of the reference; the device's NMS map bit-equal to
oracle.simple_nms of the device's OWN score map; keypoints identical to the golden in set and order; scores and descriptors within 1e-3;
the dense taps (conv1b, encoder, dense descriptors) within atol 2e-4 + rtol 1e-4 (tests/test_superpoint_emu.py's encoder bound).
"""
from __future__ import annotations

import functools
import hashlib
import importlib
import json
from pathlib import Path

import numpy as np
import torch

from oracle import superpoint_ref
from tests import nn_ref

sp_mod = importlib.import_module("deep-image-matching_amd.superpoint_hip")
capi = importlib.import_module("deep-image-matching_amd.capi")
weights_mod = importlib.import_module("deep-image-matching_amd.weights")

HERE = Path(__file__).parent
GOLD = HERE / "golden"
WEIGHT_SEED = 4321
GUARD_LAYER, GUARD_NEXT, GUARD_CHANNEL, GUARD_FACTOR = "backbone.1.0", "backbone.1.1", 5, 32768.0

CASES = {
    # 1. keep-all, every size a multiple of 8
    "keepall": {"H": 64, "W": 96, "seed": 3, "cfg": {"nms_radius": 4, "keypoint_threshold": 0.005, "max_keypoints": -1, "remove_borders": 4}},
    # 2. the pipeline's configuration on 100 x 150, padded to 104 x 152: the levels are 52 x 76, 26 x 38, 13 x 19 (odd / ragged tiles everywhere)
    "ragged_pipeline": {"H": 100, "W": 150, "seed": 5, "cfg": {"nms_radius": 5, "keypoint_threshold": 0.005, "max_keypoints": 4096, "remove_borders": 4}},
    # 3. more candidates than k: the output is score-descending
    "topk50": {"H": 120, "W": 160, "seed": 18, "cfg": {"nms_radius": 3, "keypoint_threshold": 0.005, "max_keypoints": 50, "remove_borders": 4}},
    # 4. a threshold near the median NMS score (at 0.005 it rejects nothing on these weights)
    "threshold": {"H": 64, "W": 96, "seed": 3, "cfg": {"nms_radius": 4, "keypoint_threshold": 0.05, "max_keypoints": -1, "remove_borders": 4}},
    # 6. one channel of conv2a's BatchNorm with gamma x -32768 (beta = mean = 0: its outputs are <= 0 and reach far below -4094) and conv2b's weights
    #    of that input channel x 1 / 32768 (a power of two: the network computes what it computed with gamma x -1): the fp16x3 range guard must fire
    "guard": {"H": 64, "W": 96, "seed": 3, "guard": True, "cfg": {"nms_radius": 4, "keypoint_threshold": 0.005, "max_keypoints": -1, "remove_borders": 4}},
}


def padded(n: int) -> int:
    return -(-n // 8) * 8


def image_u8(H: int, W: int, seed: int) -> np.ndarray:
    """Seeded H x W uint8 image, integer arithmetic only: 0.7 x a 5 x 5 box blur of uniform noise + 0.3 x fresh noise (smooth enough for the
    detector to have separated maxima, the same bytes on every host)."""
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, size=(H + 4, W + 4)).astype(np.int64)
    b = rng.randint(0, 256, size=(H, W)).astype(np.int64)
    c = np.zeros((H + 5, W + 5), np.int64)
    c[1:, 1:] = a.cumsum(0).cumsum(1)
    box = c[5:, 5:] - c[:-5, 5:] - c[5:, :-5] + c[:-5, :-5]       # (H, W) sums over 5 x 5
    return ((7 * box + 75 * b) // 250).astype(np.uint8)


def blocks_u8(H: int, W: int, seed: int, b: int = 4) -> np.ndarray:
    """Seeded H x W uint8 image of b x b blocks of uniform grey levels: corners everywhere."""
    a = np.random.RandomState(seed).randint(0, 256, size=(H // b + 1, W // b + 1))
    return np.kron(a, np.ones((b, b), np.int64))[:H, :W].astype(np.uint8)


def image(case) -> torch.Tensor:
    """[1, 1, Hp, Wp] float32: image / 255, zero-padded at the bottom and the right to multiples of 8 (what the extractor hook feeds the network)."""
    H, W = case["H"], case["W"]
    x = torch.zeros(1, 1, padded(H), padded(W))
    x[0, 0, :H, :W] = torch.from_numpy(image_u8(H, W, case["seed"]).astype(np.float32) / 255.0)
    return x


@functools.lru_cache(maxsize=None)
def _weights(guard: bool):
    sd = weights_mod.synthetic_superpoint_open_state_dict(WEIGHT_SEED)
    if guard:
        c = GUARD_CHANNEL
        sd[GUARD_LAYER + ".bn.weight"][c] = -GUARD_FACTOR * sd[GUARD_LAYER + ".bn.weight"][c].abs()
        sd[GUARD_LAYER + ".bn.bias"][c] = 0.0
        sd[GUARD_LAYER + ".bn.running_mean"][c] = 0.0
        sd[GUARD_NEXT + ".conv.weight"][:, c] /= GUARD_FACTOR
    return sd


def weights(case):
    """The case's state dict (shared: treat as read-only)."""
    return _weights(bool(case.get("guard")))


def state_dict_sha1(sd) -> str:
    h = hashlib.sha1()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


@functools.lru_cache(maxsize=None)
def gold(name: str):
    """The golden file of a case as torch tensors / python scalars (shared: treat as read-only)."""
    g = np.load(GOLD / f"spopen_{name}.npz")
    d = {k: (torch.from_numpy(g[k]) if g[k].ndim else g[k].item()) for k in g.files}
    for k in ("scores", "descriptors", "score_map"):   # the fp64 evaluation is stored as its float32 residual from the fp32 one
        d[k + "64"] = d[k].double() + d.pop(k + "64_res").double()
    return d


_measured = {}


def record(label: str, **res):
    """Measured distances (recorded, not gated): merged into spopen_parity.json under $DIM_PARITY_OUT (default: the system's temporary directory);
    profiles/spopen_parity.json is a copy of the file a run on the GPU wrote."""
    import os
    import tempfile
    _measured[label] = {k: (v if isinstance(v, (int, float, str, bool)) else str(v)) for k, v in res.items()}
    d = Path(os.environ.get("DIM_PARITY_OUT") or tempfile.gettempdir())
    try:
        d.mkdir(parents=True, exist_ok=True)
        p = d / "spopen_parity.json"
        old = json.loads(p.read_text()) if p.exists() else {}
        old.update(_measured)
        p.write_text(json.dumps(old, indent=1, sort_keys=True) + "\n")
    except (OSError, ValueError):
        pass


def make_net(lib, device, case, max_batch=1, hw=None, capacity=4096, **kw):
    hw = hw or (padded(case["H"]), padded(case["W"]))
    return sp_mod.SuperPointOpenHIP(weights(case), dict(case["cfg"]), max_batch=max_batch, max_hw=hw, capacity=capacity, device=device, lib=lib, **kw)


def run_counted(net, img):
    """One [1,1,H,W] image through extract_batch with the range-guard counters read: (feature dict on the CPU, guard total, sites)."""
    x = img.reshape(1, img.shape[-2], img.shape[-1]).contiguous().to(net.device)
    capi.check(net.lib, net.lib.dim_saturation_reset(net._stream()))
    kp, sc, de, n = net.extract_batch(x)
    total, sites = capi.saturation(net.lib, net._stream(), reset=True)
    k = int(n[0].item())
    return {"keypoints": kp[0, :k].cpu(), "scores": sc[0, :k].cpu(), "descriptors": de[0, :k].t().cpu()}, total, sites


def check_against_golden(net, out, name, label):
    """Taps and outputs of the last call on ``net`` against the golden of case ``name``."""
    case, g = CASES[name], gold(name)
    Hp, Wp = padded(case["H"]), padded(case["W"])
    assert (g["H"], g["W"], g["Hp"], g["Wp"], g["seed"]) == (case["H"], case["W"], Hp, Wp, case["seed"])
    taps = net.debug_taps()
    dense = lambda a, b: np.testing.assert_allclose(a.numpy(), b.numpy(), atol=2e-4, rtol=1e-4)  # noqa: E731
    # stage 1: fused conv1a + its BatchNorm, conv1b + BatchNorm (negative gammas) + pool, at the golden's sample of rows and columns (borders + every 3rd)
    c1 = net.debug_conv1b(1, Hp, Wp)
    assert c1.shape == (1, Hp // 2, Wp // 2, 64)
    dense(c1[0][g["conv1b_rows"].long()][:, g["conv1b_cols"].long()], g["conv1b"])
    dense(taps["encoder"][0], g["encoder"])
    dense(taps["dense_desc"][0], g["dense_desc"])
    err_map = (taps["score_map"][0] - g["score_map"]).abs().max().item()
    print(f"spopen {label}: score map max abs distance from the reference {err_map:.3e}")
    assert err_map <= 1e-5, err_map
    nms_on_ours = superpoint_ref.simple_nms(taps["score_map"], case["cfg"]["nms_radius"])
    assert torch.equal(nms_on_ours[0], taps["nms_map"][0]), "the NMS map is not oracle.simple_nms of the device's own score map"
    # outputs: the same keypoints in the same order, no exclusions
    assert out["keypoints"].shape == g["keypoints"].shape and torch.equal(out["keypoints"], g["keypoints"]), (out["keypoints"].shape, g["keypoints"].shape)
    assert out["descriptors"].shape == (256, g["keypoints"].shape[0])
    err_s = (out["scores"] - g["scores"]).abs().max().item()
    err_d = (out["descriptors"] - g["descriptors"]).abs().max().item()
    # distances from the fp64 evaluation of the reference module: the device's and the fp32 reference's own (recorded, not gated)
    record(label, n=int(g["keypoints"].shape[0]), score_map_vs_ref=err_map, scores_vs_ref=err_s, desc_vs_ref=err_d,
           score_map_dev_vs_fp64=(taps["score_map"][0].double() - g["score_map64"]).abs().max().item(),
           score_map_ref_vs_fp64=(g["score_map"].double() - g["score_map64"]).abs().max().item(),
           scores_dev_vs_fp64=(out["scores"].double() - g["scores64"]).abs().max().item(),
           scores_ref_vs_fp64=(g["scores"].double() - g["scores64"]).abs().max().item(),
           desc_dev_vs_fp64=(out["descriptors"].double() - g["descriptors64"]).abs().max().item(),
           desc_ref_vs_fp64=(g["descriptors"].double() - g["descriptors64"]).abs().max().item())
    assert err_s <= 1e-3 and err_d <= 1e-3, (err_s, err_d)
    return taps


# ---- 1 - 4. goldens -----------------------------------------------------------------------------------------------------------------------
def golden(lib, device, name):
    case = CASES[name]
    g = gold(name)
    assert state_dict_sha1(weights(case)) == g["state_dict_sha1"], "the synthetic weights differ from the ones the golden was made with"
    net = make_net(lib, device, case)
    out, sat, sites = run_counted(net, image(case))
    assert sat == 0, f"range guard fired on benign weights: {sites}"
    check_against_golden(net, out, name, f"{name}_{device}")
    n = out["keypoints"].shape[0]
    k = case["cfg"]["max_keypoints"]
    if name == "topk50":
        cand = int(net.candidate_counts(1)[0])
        assert n == k and cand > k, (n, cand)
        assert bool((out["scores"][1:] <= out["scores"][:-1]).all()), "top-k output is not score-descending"
    else:   # row-major
        lin = out["keypoints"][:, 1] * 10000 + out["keypoints"][:, 0]
        assert n > 20 and bool((lin[1:] > lin[:-1]).all())
    if name == "threshold":   # the threshold really rejects: between a quarter and three quarters of what 0.005 admits
        n_all = gold("keepall")["keypoints"].shape[0]
        assert 0.25 * n_all <= n <= 0.75 * n_all, (n, n_all)
    if name == "ragged_pipeline":
        assert (padded(case["H"]), padded(case["W"])) == (104, 152)


# ---- 5. batch of 3 and one handle across sizes --------------------------------------------------------------------------------------------
def _raw(net, imgs):
    x = torch.stack([i[0, 0] for i in imgs]).contiguous().to(net.device)
    kp, sc, de, n = net.extract_batch(x)
    return [tuple(t[b, : int(n[b].item())].cpu().clone() for t in (kp, sc, de)) for b in range(len(imgs))]


def _same(a, b):
    return all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


def batch_and_reuse(lib, device):
    case = CASES["keepall"]
    big = {**case, "H": 72, "W": 104}
    imgs = [image({**big, "seed": s}) for s in (11, 12, 13)]
    small = image(case)
    net = make_net(lib, device, big, max_batch=3)
    first = _raw(net, [small])[0]                                   # 64 x 96 on a 72 x 104 handle
    three = _raw(net, imgs)                                         # grow: batch of 3 at the handle's full size
    again = _raw(net, [small])[0]                                   # shrink: stale maps of the larger call lie behind the smaller one's
    one = make_net(lib, device, big)
    singles = [_raw(one, [i])[0] for i in imgs]
    assert all(len(s[0]) > 50 for s in singles)
    for b in range(3):
        assert _same(three[b], singles[b]), f"image {b} of a batch of 3 differs from its single call"
    fresh = _raw(make_net(lib, device, case), [small])[0]
    assert _same(first, fresh) and _same(again, fresh), "a reused handle differs from a fresh one"
    assert torch.equal(fresh[0], gold("keepall")["keypoints"])


# ---- 5b. the 16-row tiles of the production shapes (GPU only: four 1024 x 1024 images) ------------------------------------------------------
def big_tiles(lib, device):
    """launch_conv3x3_x6_planes takes the 16-row tile kernels only when they fill the chip (>= 256 workgroups): 1024 x 1024 x batch 4 is the
    smallest production-like shape at which EVERY encoder layer does.  A 16-row tile accumulates each output in the order of the 8-row tile
    (the goldens above pin those), so switching bit 4 of dim_tune_set key 2 off must change nothing, bit for bit."""
    case = {**CASES["ragged_pipeline"], "H": 1024, "W": 1024}
    x = torch.stack([image({**case, "seed": s})[0, 0] for s in (31, 32, 33, 34)]).contiguous().to(device)
    net = make_net(lib, device, case, max_batch=4)
    try:
        capi.check(lib, lib.dim_saturation_reset(net._stream()))
        a = [t.clone() for t in net.extract_batch(x)]
        ta = net.debug_taps(4)
        total, sites = capi.saturation(lib, net._stream(), reset=True)
        lib.dim_tune_set(2, 1)
        b = [t.clone() for t in net.extract_batch(x)]
        tb = net.debug_taps(4)
    finally:
        lib.dim_tune_set(2, 1 | 16)
    assert total == 0, sites
    for k in ("encoder", "score_map", "dense_desc"):
        assert torch.equal(ta[k], tb[k]), k
    assert torch.equal(a[3], b[3]) and int(a[3].min()) == 4096
    for i in range(4):
        assert all(torch.equal(u[i], v[i]) for u, v in zip(a[:3], b[:3]))
    # and the maps are sane: a softmax without its dustbin, unit descriptors
    assert 0.0 <= float(ta["score_map"].min()) and float(ta["score_map"].max()) < 1.0
    assert (a[2][0].norm(dim=1) - 1).abs().max().item() < 1e-5


# ---- 6. range guard on signed activations -------------------------------------------------------------------------------------------------
def range_guard(lib, device):
    case = CASES["guard"]
    g = gold("guard")
    assert state_dict_sha1(weights(case)) == g["state_dict_sha1"]
    assert g["guard_min"] < -4094.0 and g["guard_max"] <= 4094.0     # the reference's own conv2a output: far below the range, never above it
    net = make_net(lib, device, case, on_saturation="fallback")
    _, sat, sites = run_counted(net, image(case))
    assert sat > 0 and sites.get("sp_encoder", 0) > 0, f"values below -4094 did not trip the guard (a guard on v instead of |v|?): {sites}"
    out = net(image(case))                                              # the guarded call: repeats in bf16x6
    out = {k: v.cpu() for k, v in out.items()}
    check_against_golden(net, out, "guard", f"guard_{device}")
    net_raise = make_net(lib, device, case, on_saturation="raise")
    try:
        net_raise(image(case))
    except capi.SaturationError:
        pass
    else:
        raise AssertionError("on_saturation='raise' did not raise")


# ---- 7. loader validation (CPU only: nothing native is reached) ---------------------------------------------------------------------------
def loader_validation(tmp_path):
    import pytest
    sd = weights_mod.synthetic_superpoint_open_state_dict(WEIGHT_SEED)
    ok = tmp_path / "ok.pth"
    torch.save(sd, ok)
    back = weights_mod.load_superpoint_open_state_dict(str(ok))
    assert set(back) == set(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    with pytest.raises(weights_mod.MissingWeightsError):
        weights_mod.load_superpoint_open_state_dict(None)

    def broken(change):
        d = {k: v.clone() for k, v in sd.items()}
        change(d)
        p = tmp_path / "broken.pth"
        torch.save(d, p)
        return str(p), d

    p, d = broken(lambda d: d.pop("backbone.2.1.bn.running_var"))
    with pytest.raises(KeyError, match=r"backbone\.2\.1\.bn\.running_var"):
        weights_mod.load_superpoint_open_state_dict(p)
    with pytest.raises(KeyError, match=r"backbone\.2\.1\.bn\.running_var"):
        sp_mod.SuperPointOpenHIP(d, {}, device="cpu", lib=None)        # validated before the library is even opened
    p, d = broken(lambda d: d.__setitem__("detector.1.conv.weight", torch.zeros(64, 256, 1, 1)))
    with pytest.raises(ValueError, match=r"detector\.1\.conv\.weight"):
        weights_mod.load_superpoint_open_state_dict(p)
    p, d = broken(lambda d: d["descriptor.0.bn.running_var"].__setitem__(3, -0.5))
    with pytest.raises(ValueError, match=r"descriptor\.0\.bn\.running_var"):
        weights_mod.load_superpoint_open_state_dict(p)
    p, d = broken(lambda d: d.__setitem__("backbone.0.0.conv.extra", torch.zeros(1)))
    with pytest.raises(KeyError, match=r"backbone\.0\.0\.conv\.extra"):
        weights_mod.load_superpoint_open_state_dict(p)


# ---- 8. SuperPointOpenExtractor -> KorniaMatcher ------------------------------------------------------------------------------------------
SHIFT = (16, 8)   # (x, y) pixels: multiples of 8, so both views see the same cells


def extractor_matcher_chain(plugins, tmp_path):
    """The `superpoint_open+kornia_matcher` pipeline's configuration (nms 5, threshold 0.005, 4096 keypoints, smnn 0.95) through the two plugin hooks
    on a view and the same view shifted by SHIFT: the match list obeys tests/nn_ref.py's rule on the very features the matcher saw, and at least
    90 % of the matches have the true shift within 1 px."""
    H, W = 118, 157                                   # not multiples of 8: the hook pads to 120 x 160
    canvas = blocks_u8(H + SHIFT[1], W + SHIFT[0], 21).astype(np.float32)
    v0, v1 = canvas[:H, :W], canvas[SHIFT[1]:, SHIFT[0]:]
    # He-normal kernels see ~80 px around a pixel, most of a view this small, and the two views differ beyond their borders: centre-heavy kernels in
    # the deep layers (off_centre; weights.synthetic_superpoint_open_state_dict) keep the descriptors local.  Checked on the reference's own network and
    # fp32 matcher with these weights and views: 0.94 - 0.97 of its matches have the true shift; what remains lies in the strip only one view sees.
    wpath = tmp_path / "spopen_local.pth"
    torch.save(weights_mod.synthetic_superpoint_open_state_dict(WEIGHT_SEED, off_centre=0.03), wpath)
    general = {"geom_verification": "NONE"}
    ex = plugins.SuperPointOpenExtractor({"general": general, "extractor": {"name": "superpoint_open", "nms_radius": 5, "keypoint_threshold": 0.005,
                                                                             "max_keypoints": 4096, "remove_borders": 4, "weights_path": str(wpath)}})
    assert plugins.SuperPointOpenExtractor._default_conf == {"name": "superpoint", "nms_radius": 4, "keypoint_threshold": 0.005, "max_keypoints": -1,
                                                             "remove_borders": 4, "fix_sampling": False}
    assert ex.grayscale is True and ex.descriptor_size == 256 and ex.required_inputs == ["image"] and ex.detection_noise == 2.0
    f0, f1 = ex._extract(v0), ex._extract(v1)
    for f in (f0, f1):
        n = f["keypoints"].shape[0]
        assert n > 50 and f["keypoints"].dtype == np.float32 and f["scores"].shape == (n,) and f["descriptors"].shape == (256, n)
        assert f["keypoints"][:, 0].max() < 160 and f["keypoints"][:, 1].max() < 120
    mt = plugins.KorniaMatcher({"general": general, "matcher": {"name": "kornia_matcher", "match_mode": "smnn", "th": 0.95}})
    m = mt._match_pairs(f0, f1)
    a, b = torch.from_numpy(np.ascontiguousarray(f0["descriptors"].T)), torch.from_numpy(np.ascontiguousarray(f1["descriptors"].T))
    d2 = nn_ref.d2_fp64(a, b)
    must, may = nn_ref.classify_fp64(a, b, "smnn", 0.95, nn_ref.measured_tol(a, b, d2), d2)
    nn_ref.check_rule(m, must, may, "superpoint_open + kornia_matcher")
    if not may:
        assert np.array_equal(m, nn_ref.reference_fp32(a, b, "smnn", 0.95)[0])
    assert len(m) >= 20, len(m)
    d = f0["keypoints"][m[:, 0]] - f1["keypoints"][m[:, 1]] - np.asarray(SHIFT, np.float32)
    good = float((np.abs(d).max(1) <= 1.0).mean())
    print(f"superpoint_open + kornia_matcher: {len(m)} matches, {good:.3f} at the true shift")
    assert good >= 0.9, (len(m), good)
    # keep-all through the hook (the class default max_keypoints = -1, where the reference's network raises): every candidate, row-major
    ex_all = plugins.SuperPointOpenExtractor({"general": general, "extractor": {"name": "superpoint_open", "allow_synthetic_weights": True}})
    fa = ex_all._extract(v0)
    lin = fa["keypoints"][:, 1] * 10000 + fa["keypoints"][:, 0]
    assert fa["keypoints"].shape[0] >= f0["keypoints"].shape[0] and bool((lin[1:] > lin[:-1]).all())
