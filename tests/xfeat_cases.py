"""Shared by the emulator and the GPU tests of the XFeat extractor (tests/test_xfeat_emu.py, tests/test_xfeat_gpu.py).  Every case takes
(lib, device): the emulator build with "cpu", or the gfx950 library with "cuda".

Weights are seeded synthetic ones (weights.synthetic_xfeat_state_dict: the trained xfeat.pt is not distributed with the reference tree).
tests/golden/xfeat_<case>.npz hold the REFERENCE MODULE's outputs on seeded images (scripts/make_xfeat_golden.py, which also asserts that
tests/xfeat_ref.py equals the module bit for bit, that fp32 and fp64 select the same pixels and that at most MAX_NEAR_TIES decisions are near
ties); everything else is compared against tests/xfeat_ref.py.
"""
from __future__ import annotations

import ctypes
import functools
import importlib
import json
from pathlib import Path

import numpy as np
import torch

from tests import nn_ref, xfeat_ref

xf_mod = importlib.import_module("deep-image-matching_amd.xfeat_hip")
capi = importlib.import_module("deep-image-matching_amd.capi")
weights_mod = importlib.import_module("deep-image-matching_amd.weights")
nn_mod = importlib.import_module("deep-image-matching_amd.nn_hip")

HERE = Path(__file__).parent
GOLD = HERE / "golden"
PARITY = HERE.parent / "profiles" / "xfeat_parity.json"
TIE_TOL = 2e-5   # the project's near-tie bar (tests/alike_cases.py)
MAX_NEAR_TIES = 4
THRESHOLD = 0.05  # the network's own default: extractors/xfeat.py never hands detect_threshold on
WEIGHT_SEED = 21

# seeded uniform-noise images (0..255, float32 values of integers); shape (H, W) = single channel
GOLDEN_CASES = {
    "min32": {"shape": (32, 32, 3), "seed": 1, "top_k": 4000},
    "ragged": {"shape": (100, 150, 3), "seed": 2, "top_k": 4000},
    "gray": {"shape": (40, 70), "seed": 3, "top_k": 4000},
    "topk": {"shape": (128, 160, 3), "seed": 4, "top_k": 100},
}


def image(case) -> np.ndarray:
    rng = np.random.default_rng(case["seed"])
    return rng.integers(0, 256, size=case["shape"]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def weights(seed: int = WEIGHT_SEED):
    return weights_mod.synthetic_xfeat_state_dict(seed)


@functools.lru_cache(maxsize=None)
def photo() -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.open(HERE / "assets" / "config1" / "sacre_coeur_A.jpg").convert("RGB"))


def record(label, **res):
    """Measured figures behind an assertion: profiles/xfeat_parity.json, one entry per label (rewritten in place)."""
    try:
        data = json.loads(PARITY.read_text()) if PARITY.exists() else {}
        data[label] = {k: (v if isinstance(v, (int, float, str, bool)) else str(v)) for k, v in res.items()}
        PARITY.write_text(json.dumps(data, indent=1, sort_keys=True) + "\n")
    except OSError:
        pass


def make_net(lib, device, hw, top_k=4000, max_batch=1, capacity=None, sd=None, **cfg):
    return xf_mod.XFeatHIP(sd if sd is not None else weights(), {"top_k": top_k, **cfg}, max_batch=max_batch, max_hw=hw, capacity=capacity,
                           device=device, lib=lib)


def run(net, img, device, guarded=False):
    """One H x W (x C) float image through extract_batch with the range-guard counters read: (feature dict on the CPU, guard total)."""
    x = torch.from_numpy(np.ascontiguousarray(img.reshape(img.shape[0], img.shape[1], -1)))[None].contiguous().to(device)
    if guarded:
        kp, sc, de, n = net.extract_batch_guarded(x)
        total = 0
    else:
        capi.check(net.lib, net.lib.dim_saturation_reset(net._stream()))
        kp, sc, de, n = net.extract_batch(x)
        total, _ = capi.saturation(net.lib, net._stream(), reset=True)
    k = int(n[0].item())
    return {"keypoints": kp[0, :k].cpu(), "scores": sc[0, :k].cpu(), "descriptors": de[0, :k, :64].cpu()}, total


def near_decisions(K1h, thr=THRESHOLD, tol=TIE_TOL):
    """Pixels of a keypoint heat map whose selection hangs on a near tie: a (near) window maximum within tol of the threshold, or a candidate
    whose 5 x 5 window holds another value within tol of it.  Returns a bool map."""
    m = K1h.reshape(1, 1, *K1h.shape[-2:]).double()
    H, W = m.shape[-2:]
    pad = torch.nn.functional.pad(m, (2, 2, 2, 2), value=-1.0)
    win = pad.unfold(2, 5, 1).unfold(3, 5, 1).reshape(H, W, 25)
    top = torch.topk(win, 2, dim=-1).values
    v = m[0, 0]
    is_max = v >= top[..., 0] - tol
    near_thr = is_max & ((v - thr).abs() <= tol)
    near_nb = is_max & (v > thr - tol) & ((top[..., 0] - top[..., 1]) <= tol)
    return near_thr | near_nb


def compare_xfeat(out, ref, K1h_ref, scale, label=None, tol=1e-3, max_one_sided=0, key_ref=None, cut=None):
    """tests/alike_cases.compare_alike for XFeat's outputs (descriptor ROWS): keypoints paired exactly (they are integer pixels times (rw, rh)),
    a bijection; rows in score-descending order, out of place only within TIE_TOL of each other in the REFERENCE's scores; a keypoint on one side
    only must sit at a near-tie decision of the REFERENCE's map (near_decisions) or within TIE_TOL of the top-k cut; values within `tol`."""
    ko, kr = out["keypoints"].numpy().astype(np.float64), ref["keypoints"].numpy().astype(np.float64)
    rw, rh = scale
    pix = lambda k: [(int(round(x / rw)), int(round(y / rh))) for x, y in k]  # noqa: E731
    po, pr = pix(ko), pix(kr)
    where = {p: j for j, p in enumerate(pr)}
    assert len(where) == len(pr) and len(set(po)) == len(po), "duplicate keypoints"
    pairs = [(i, where[p]) for i, p in enumerate(po) if p in where]
    ia = torch.tensor([p[0] for p in pairs], dtype=torch.long); ib = torch.tensor([p[1] for p in pairs], dtype=torch.long)
    only_out = [po[i] for i in sorted(set(range(len(po))) - {p[0] for p in pairs})]
    only_ref = [pr[j] for j in sorted(set(range(len(pr))) - {p[1] for p in pairs})]
    res = {"n_out": len(ko), "n_ref": len(kr), "common": len(pairs), "one_sided": max(len(only_out), len(only_ref))}
    res["kp"] = (out["keypoints"][ia] - ref["keypoints"][ib]).abs().max().item() if pairs else 0.0
    res["score"] = (out["scores"][ia] - ref["scores"][ib]).abs().max().item() if pairs else 0.0
    res["desc"] = (out["descriptors"][ia] - ref["descriptors"][ib]).abs().max().item() if pairs else 0.0
    moved = [(i, j, float(ref["scores"][i]), float(ref["scores"][j])) for i, j in pairs if i != j and i < len(kr)]
    res["rows_out_of_place"] = len([1 for i, j in pairs if i != j])
    if label is not None:
        record(label, **res)
    if only_out or only_ref:
        near = near_decisions(K1h_ref)
        for x, y in only_out + only_ref:
            at_cut = cut is not None and key_ref is not None and abs(float(key_ref[y, x]) - cut) <= TIE_TOL
            assert bool(near[y, x]) or at_cut, ((x, y), float(K1h_ref[y, x]), res)
    assert res["one_sided"] <= max_one_sided and (max_one_sided > 0 or len(ko) == len(kr)), res
    assert bool((ref["scores"][1:] <= ref["scores"][:-1]).all()), "the reference rows are not score-descending"
    assert bool((out["scores"][1:] <= out["scores"][:-1]).all()), "the output rows are not score-descending"
    assert all(abs(a - b) <= TIE_TOL for _, _, a, b in moved), ("score-descending order differs beyond near ties", moved[:5], res)
    assert res["kp"] <= tol and res["score"] <= tol and res["desc"] <= tol, res
    return res


def _gold(name):
    g = np.load(GOLD / f"xfeat_{name}.npz")
    return {k: torch.from_numpy(g[k]) for k in g.files}


# ---- 1. goldens ---------------------------------------------------------------------------------------------------------------------------
def golden(lib, device, name):
    case = GOLDEN_CASES[name]
    img = image(case)
    gold = _gold(name)
    assert np.array_equal(gold["image"].numpy(), img.astype(np.uint8))
    H, W = img.shape[:2]
    _H, _W = H // 32 * 32, W // 32 * 32
    scale = (W / _W, H / _H)
    net = make_net(lib, device, (H, W), top_k=case["top_k"])
    out, sat = run(net, img, device)
    assert sat == 0, f"range guard fired ({sat})"
    assert out["keypoints"].shape == gold["keypoints"].shape and out["descriptors"].shape == (gold["keypoints"].shape[0], 64)
    ref = xfeat_ref.xfeat_forward(img, weights(), top_k=case["top_k"], taps=True)
    # (restatement == module bit for bit is asserted where the golden is made: torch's CPU kernels differ from host to host in the last bit)
    assert (ref["K1h"] - gold["K1h"]).abs().max().item() <= 1e-5 and (ref["H1"] - gold["H1"]).abs().max().item() <= 1e-5
    compare_xfeat(out, gold, gold["K1h"], scale, label=f"xfeat_{name}_{device}_golden")
    compare_xfeat(out, ref, ref["K1h"], scale)
    taps = net.debug_taps()
    assert taps["hw"] == (_H, _W)
    k_dev, h_dev = taps["K1h"][0].cpu(), taps["H1"][0].cpu()
    dk, dh = (k_dev - gold["K1h"]).abs().max().item(), (h_dev - gold["H1"]).abs().max().item()
    # keypoint heat map against fp64: at most twice the fp32 restatement's own error on the same input
    k64 = gold["K1h"].double() + gold["K1h_res64"].double()
    err_dev, err_ref = (k_dev.double() - k64).abs().max().item(), gold["K1h_res64"].double().abs().max().item()
    print(f"xfeat {name} {device}: K1h vs golden {dk:.3e}, H1 vs golden {dh:.3e}; K1h vs fp64: device {err_dev:.3e}, fp32 reference {err_ref:.3e}")
    record(f"xfeat_{name}_{device}_maps", K1h_vs_golden=dk, H1_vs_golden=dh, K1h_vs_fp64_device=err_dev, K1h_vs_fp64_fp32_reference=err_ref)
    assert dk <= 1e-5 and dh <= 1e-5, (dk, dh)
    assert err_dev <= 2.0 * err_ref, (err_dev, err_ref)
    # normalised image against fp64: the resize coordinates are fp32 in the reference too (1 ulp of a coordinate moves a 0..255 sample by ~2e-3),
    # so the yardstick is again the fp32 restatement's own distance from fp64
    n64 = xfeat_ref.xfeat_forward(img, weights(), top_k=case["top_k"], taps=True, dtype=torch.float64)["norm"]
    n_dev, n_ref = (taps["norm"][0].cpu().double() - n64).abs().max().item(), (ref["norm"].double() - n64).abs().max().item()
    record(f"xfeat_{name}_{device}_norm_vs_fp64", device=n_dev, fp32_restatement=n_ref)
    assert n_dev <= 2.0 * n_ref + 1e-6, (n_dev, n_ref)
    d_dense = (taps["M1"][0].cpu().permute(2, 0, 1) - ref["M1"]).abs().max().item()
    assert d_dense <= 1e-3, d_dense


# ---- 2. the photograph ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def photo_reference():
    return xfeat_ref.xfeat_forward(photo().astype(np.float32), weights(), top_k=4096, taps=True)


def ref_keys(ref):
    """(key map of the reference's candidates on its own maps, all candidate keys sorted descending)."""
    K1h, H1 = ref["K1h"][None, None], ref["H1"][None, None]
    mk, sc = xfeat_ref.select(K1h, H1, 1 << 30)
    keys = torch.zeros_like(ref["K1h"])
    ok = sc[0] > 0
    keys[mk[0, ok, 1], mk[0, ok, 0]] = sc[0, ok]
    return keys, sc[0, ok]


def photo_case(lib, device):
    img = photo().astype(np.float32)
    assert img.shape == (480, 640, 3)
    ref = photo_reference()
    keys, cand = ref_keys(ref)
    assert len(cand) > 4096, len(cand)
    cut = float(cand[4095])
    near_cut = int(((cand - cut).abs() <= TIE_TOL).sum())
    net = make_net(lib, device, (480, 640), top_k=4096)
    out, sat = run(net, img, device)
    assert sat == 0, f"range guard fired ({sat})"
    res = compare_xfeat(out, ref, ref["K1h"], (1.0, 1.0), label=f"xfeat_photo_{device}", max_one_sided=near_cut, key_ref=keys, cut=cut)
    record(f"xfeat_photo_{device}_ties", near_cut=near_cut, one_sided=res["one_sided"])


# ---- 3. batch and handle reuse ------------------------------------------------------------------------------------------------------------
def _raw(net, imgs, device):
    x = torch.stack([torch.from_numpy(i) for i in imgs]).contiguous().to(device)
    kp, sc, de, n = net.extract_batch(x)
    outs = []
    for b in range(len(imgs)):
        k = int(n[b].item())
        outs.append((kp[b, :k].cpu().clone(), sc[b, :k].cpu().clone(), de[b, :k].cpu().clone()))
    return outs


def _same(a, b):
    return all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


def batch_and_reuse(lib, device):
    rng = np.random.default_rng(7)
    a = rng.integers(0, 256, size=(100, 150, 3)).astype(np.float32)
    b = np.repeat(rng.integers(0, 256, size=(50, 75, 3)), 2, axis=0).repeat(2, axis=1).astype(np.float32)   # blockier: another count
    hw = (100, 150)
    two = _raw(make_net(lib, device, hw, top_k=600, max_batch=2), [a, b], device)
    one_a = _raw(make_net(lib, device, hw, top_k=600), [a], device)[0]
    one_b = _raw(make_net(lib, device, hw, top_k=600), [b], device)[0]
    assert len(one_a[0]) > 20 and len(one_b[0]) > 20 and len(one_a[0]) != len(one_b[0]), (len(one_a[0]), len(one_b[0]))
    assert _same(two[0], one_a) and _same(two[1], one_b), "a batch of 2 differs from the two single calls"
    small = a[:40, :70].copy()
    net = make_net(lib, device, hw, top_k=600)
    first, mid, again = _raw(net, [a], device)[0], _raw(net, [small], device)[0], _raw(net, [a], device)[0]
    fresh_small = _raw(make_net(lib, device, hw, top_k=600), [small], device)[0]
    assert _same(first, one_a) and _same(again, one_a) and _same(mid, fresh_small), "a reused handle differs from fresh handles"


# ---- 4. range guard -----------------------------------------------------------------------------------------------------------------------
def guard(lib, device):
    """One BasicLayer channel scaled out of the fp16x3 range and its consumer scaled back by the same power of two (tests/spopen_cases.py's guard):
    real arithmetic unchanged, the stored activation leaves +-4094; the guard fires and the guarded re-run equals the golden."""
    assert capi.get_arithmetic(lib) == 2
    case = GOLDEN_CASES["ragged"]
    img, gold = image(case), _gold("ragged")
    sd = {k: v.clone() for k, v in weights().items()}
    s = 2.0 ** 16
    # block3.1 channel 5: convolution row and running mean times s (the variance stays) -> relu((conv - mean) / sigma) times s, exactly
    sd["block3.1.layer.0.weight"][5] *= s
    sd["block3.1.layer.1.running_mean"][5] *= s
    sd["block3.2.layer.0.weight"][:, 5] /= s
    H, W = img.shape[:2]
    net = make_net(lib, device, (H, W), sd=sd)
    _, sat = run(net, img, device)
    assert sat > 0, "the range guard did not fire"
    out, _ = run(net, img, device, guarded=True)
    compare_xfeat(out, gold, gold["K1h"], (W / (W // 32 * 32), H / (H // 32 * 32)), label=f"xfeat_guard_{device}", max_one_sided=MAX_NEAR_TIES)


# ---- 5. operator-level selection ----------------------------------------------------------------------------------------------------------
def op_select(lib, device, K1h, H1, top_k, capacity=None):
    """dim_op_xfeat_select on [H][W] / [H/8][W/8] maps -> (positions [n,2] int64, keys [n])."""
    xf_mod.declare(lib)
    cap = capacity or top_k
    H, W = K1h.shape
    k1, h1 = K1h[None].contiguous().to(device), H1[None].contiguous().to(device)
    kp = torch.zeros(1, cap, 2, dtype=torch.float32, device=device); sc = torch.zeros(1, cap, dtype=torch.float32, device=device)
    n = torch.zeros(1, dtype=torch.int32, device=device)
    ws = torch.zeros(int(lib.dim_op_xfeat_select_workspace_bytes(1, H, W, top_k)) + 16, dtype=torch.uint8, device=device)
    capi.check(lib, lib.dim_op_xfeat_select(capi.ptr(k1), capi.ptr(h1), 1, H, W, ctypes.c_float(THRESHOLD), top_k, cap, capi.ptr(ws), capi.ptr(kp),
                                            capi.ptr(sc), capi.ptr(n), capi.stream_ptr(device)))
    if device != "cpu":
        torch.cuda.synchronize()
    k = int(n[0].item())
    return kp[0, :k].cpu().long(), sc[0, :k].cpu()


def _ref_select(K1h, H1, top_k):
    mk, sc = xfeat_ref.select(K1h[None, None].clone(), H1[None, None].clone(), top_k)
    ok = sc[0] > 0
    return mk[0][ok], sc[0][ok]


def _crafted(H, W):
    K = torch.full((H, W), 2.0 ** -7)              # below the threshold everywhere
    R = torch.full((H // 8, W // 8), 0.5)
    return K, R


def _check_select(lib, device, K, R, top_k, expect_n=None):
    pos, key = op_select(lib, device, K, R, top_k)
    rpos, rkey = _ref_select(K, R, top_k)
    if expect_n is not None:
        assert len(rpos) == expect_n, (len(rpos), expect_n)
    assert pos.shape == rpos.shape and torch.equal(pos, rpos), (pos.tolist()[:8], rpos.tolist()[:8])
    assert torch.equal(key, rkey), (key - rkey).abs().max().item()
    return pos, key


def select_cases(lib, device, hw):
    H, W = hw
    # dyadic heat values, pairwise different, at positions at least 5 apart; reliability values are powers of two, so the products of the bilinear
    # sample are exact and only the order of its three additions matters, which the kernel takes from the reference: keys are bit-equal
    vals = [0.5 + i * 2.0 ** -6 for i in range(12)]
    # a. a two-pixel plateau inside one window keeps both pixels
    K, R = _crafted(H, W)
    K[10, 10] = K[10, 12] = 0.75; K[20, 17] = 0.5
    pos, _ = _check_select(lib, device, K, R, 50, expect_n=3)
    assert {(10, 10), (12, 10)} <= {tuple(p) for p in pos.tolist()}
    # b. a maximum at (0, 0) is dropped; c. last row / column dropped, first row / column kept
    K, R = _crafted(H, W)
    K[0, 0] = 0.875
    K[H - 1, 9] = vals[1]; K[11, W - 1] = vals[2]; K[H - 1, W - 1] = vals[3]
    K[0, 14] = vals[4]; K[17, 0] = vals[5]; K[13, 13] = vals[6]
    pos, _ = _check_select(lib, device, K, R, 50, expect_n=3)
    assert {tuple(p) for p in pos.tolist()} == {(14, 0), (0, 17), (13, 13)}
    # d. everything below the threshold: n = 0
    K, R = _crafted(H, W)
    pos, _ = _check_select(lib, device, K, R, 50, expect_n=0)
    # e. more candidates than top_k: cut at the k-th key; f. sorted also when n < k
    K, R = _crafted(H, W)
    g = torch.Generator().manual_seed(5)
    spots = [(y, x) for y in range(3, H - 3, 6) for x in range(3, W - 3, 6)]
    order = torch.randperm(len(spots), generator=g).tolist()
    for rank, si in enumerate(order):
        K[spots[si]] = 0.25 + rank * 2.0 ** -9
    R = 2.0 ** -torch.randint(0, 3, R.shape, generator=g).float()   # powers of two: every tap's product is exact, whatever the sampler fuses
    k = len(spots) // 2
    pos, key = _check_select(lib, device, K, R, k, expect_n=k)
    assert bool((key[1:] <= key[:-1]).all())
    pos, key = _check_select(lib, device, K, R, 4 * len(spots), expect_n=len(spots))
    assert bool((key[1:] <= key[:-1]).all()) and not bool((pos[1:, 1] * W + pos[1:, 0] >= pos[:-1, 1] * W + pos[:-1, 0]).all())


# ---- 6. the matcher chain -----------------------------------------------------------------------------------------------------------------
def chain(lib, device):
    """Two crops of the photograph shifted by (16, 24) -> XFeatHIP (batch 2) -> NearestNeighborHIP(mnn): the share of matches at the true shift
    against the same chain through xfeat_ref + nn_ref."""
    a, b = photo()[100:292, 200:456].astype(np.float32), photo()[116:308, 224:480].astype(np.float32)
    net = make_net(lib, device, (192, 256), top_k=1024, max_batch=2)
    x = torch.stack([torch.from_numpy(a), torch.from_numpy(b)]).contiguous().to(device)
    kp, sc, de, n = net.extract_batch(x)
    n0, n1 = int(n[0].item()), int(n[1].item())
    assert n0 > 100 and n1 > 100
    matcher = nn_mod.NearestNeighborHIP("mnn", 0.0, dim=64, max_pairs=1, max_kpts=1024, device=device, lib=lib)
    m = matcher.match_batch_guarded(kp, de, n)
    got = m["matches"][0, : int(m["n_matches"][0].item())].cpu().numpy()
    k0, k1 = kp[0].cpu().numpy(), kp[1].cpu().numpy()
    shift = np.array([24.0, 16.0])
    share = float(np.mean(np.abs(k0[got[:, 0]] - k1[got[:, 1]] - shift).max(axis=1) < 0.5)) if len(got) else 0.0
    ra, rb = (xfeat_ref.xfeat_forward(i, weights(), top_k=1024, taps=True) for i in (a, b))
    d0, d1 = ra["descriptors"], rb["descriptors"]
    d2 = nn_ref.d2_fp64(d0, d1)
    must, may = nn_ref.classify_fp64(d0, d1, "mnn", 0.0, nn_ref.measured_tol(d0, d1, d2), d2)
    rk0, rk1 = ra["keypoints"].numpy(), rb["keypoints"].numpy()
    at = lambda prs: sum(1 for i, j in prs if np.abs(rk0[i] - rk1[j] - shift).max() < 0.5)  # noqa: E731
    must, may = [tuple(p) for p in must], [tuple(p) for p in may]
    ref_share = at(must + may) / max(1, len(must) + len(may))
    # the share attributable to the reference's near ties: matches the fp64 rule does not pin, and candidates at the top-k cut
    near = sum(int(((c - float(c[1023])).abs() <= TIE_TOL).sum()) - 1 for c in (ref_keys(r)[1] for r in (ra, rb)) if len(c) > 1024)
    slack = (len(may) + near) / max(1, len(must) + len(may))
    print(f"xfeat chain {device}: share at the true shift {share:.4f} ({len(got)} matches), reference {ref_share:.4f} ({len(must) + len(may)}), near-tie share {slack:.4f}")
    record(f"xfeat_chain_{device}", share=share, matches=int(len(got)), reference_share=ref_share, reference_matches=len(must) + len(may), near_tie_share=slack)
    assert len(got) > 50
    assert share >= ref_share - slack, (share, ref_share, slack)
