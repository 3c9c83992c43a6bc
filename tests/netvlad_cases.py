"""Shared by the emulator and the GPU tests of the NetVLAD extractor (tests/test_netvlad_emu.py, tests/test_netvlad_gpu.py).  Every case takes
(lib, device): the emulator build with "cpu", or the gfx950 library with "cuda".

Weights are seeded synthetic ones (weights.synthetic_netvlad_state: the trained .mat checkpoints are downloaded by the reference at run time and
not available offline), regenerated from the seed and never committed.  tests/golden/netvlad_<case>.npz hold, per seeded image, the REFERENCE
MODULE's fp32 descriptor and the fp64 evaluation of tests/netvlad_ref.py (scripts/make_netvlad_golden.py, which also asserts that the restatement
equals the module bit for bit in fp32).

Tolerance (the rule SuperGlue and LighterGlue use): the error of a unit-norm descriptor is its largest elementwise distance from the fp64
evaluation; the device's error may be at most twice the reference fp32 module's error on the same case, with the largest module error over all
cases as the floor.  The range guard must stay at 0 on every case."""
from __future__ import annotations

import functools
import importlib
import json
from pathlib import Path

import numpy as np
import torch

from tests import netvlad_ref

nv_mod = importlib.import_module("deep-image-matching_amd.netvlad_hip")
capi = importlib.import_module("deep-image-matching_amd.capi")
weights_mod = importlib.import_module("deep-image-matching_amd.weights")
pairs_mod = importlib.import_module("deep-image-matching_amd.pairs")

HERE = Path(__file__).parent
GOLD = HERE / "golden"
PARITY = HERE.parent / "profiles" / "netvlad_parity.json"
WEIGHT_SEED = 31

# uniform-noise images (integers 0..255, handed over as value / 255) and one crop of the photograph
GOLDEN_CASES = {
    "min": {"shape": (16, 16), "seed": 1, "K": 64, "whiten_out": None},          # one location
    "odd": {"shape": (50, 75), "seed": 2, "K": 64, "whiten_out": 4096},          # 25 x 37 -> 12 x 18 -> 6 x 9 -> 3 x 4: a floor at three levels
    "blocks": {"shape": (208, 272), "seed": 3, "K": 64, "whiten_out": 4096},     # 13 x 17 = 221 locations: two workgroups, the last sub-block ragged
    "smallk": {"shape": (48, 64), "seed": 4, "K": 8, "whiten_out": 256},         # small K and a small whitening
    "photo": {"shape": (112, 160), "crop": (300, 400), "K": 64, "whiten_out": 4096},   # tests/assets/config1/sacre_coeur_A.jpg[300:412, 400:560]
}
# 8 images: image 0 and four copies of it with growing noise (more positive neighbours than num_matched: the top-k cut decides), image 5 and one copy
# (fewer: the min_score cut decides), image 7 alone (no pair at all).  The whitening bias of this fixture centres the descriptors on the fixture's
# mean VLAD vector (stored in the golden file), as a trained PCA whitening does: unrelated images then have NEGATIVE similarities.
RETRIEVAL = {"n": 8, "shape": (64, 80), "seed": 2, "copies": ((0, 6.0), (0, 12.0), (0, 18.0), (0, 24.0), (5, 12.0)), "K": 8, "whiten_out": 256, "num_matched": 3,
             "min_score": 0.0}


@functools.lru_cache(maxsize=None)
def photo() -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.open(HERE / "assets" / "config1" / "sacre_coeur_A.jpg").convert("RGB"))


def image(case) -> np.ndarray:
    """[H,W,3] float32 in 0..1."""
    h, w = case["shape"]
    if "crop" in case:
        y, x = case["crop"]
        return (photo()[y:y + h, x:x + w].astype(np.float32) / np.float32(255.0))
    rng = np.random.default_rng(case["seed"])
    return rng.integers(0, 256, size=(h, w, 3)).astype(np.float32) / np.float32(255.0)


def retrieval_images():
    """RGB arrays 0..255, names "0" .. "7": three blocky seeded images (8 x 8 blocks of uniform noise) at 0, 5 and 7; 1 .. 4 are copies of 0 with
    Gaussian noise of sigma 6, 12, 18, 24; 6 is a copy of 5 with sigma 12."""
    r = RETRIEVAL
    rng = np.random.default_rng(r["seed"])
    h, w = r["shape"]
    blocky = lambda: np.kron(rng.integers(0, 256, size=(h // 8, w // 8, 3)), np.ones((8, 8, 1))).astype(np.float32)  # noqa: E731
    imgs = {0: blocky(), 5: blocky(), 7: blocky()}
    slots = [i for i in range(r["n"]) if i not in imgs]
    for slot, (src, sigma) in zip(slots, r["copies"]):
        imgs[slot] = np.clip(np.rint(imgs[src] + rng.normal(0.0, sigma, size=imgs[src].shape)), 0, 255).astype(np.float32)
    return [str(i) for i in range(r["n"])], [imgs[i] for i in range(r["n"])]


def pairs_from_descriptors(names, desc: np.ndarray, num_matched: int, min_score=0.0):
    """thirdparty/hloc/pairs_from_retrieval.py:49-70,108-112 (self matches and, as main() calls it, similarities below min_score = 0 masked; top
    num_matched per query, best first, masked entries never come out) followed by image_retrieval.py:34-42 (first occurrence of every unordered
    pair kept), in fp64 numpy.  Returns (pairs, similarity matrix with -inf on the diagonal)."""
    sim = desc.astype(np.float64) @ desc.astype(np.float64).T
    np.fill_diagonal(sim, -np.inf)
    masked = sim.copy()
    if min_score is not None:
        masked[sim < min_score] = -np.inf
    seen, out = set(), []
    for i in range(len(names)):
        for j in np.argsort(-masked[i], kind="stable")[:num_matched]:
            if not np.isfinite(masked[i, j]):
                continue
            key = tuple(sorted((names[i], names[int(j)])))
            if key not in seen:
                seen.add(key)
                out.append((names[i], names[int(j)]))
    return out, sim


def retrieval_state(whiten_bias=None):
    """The fixture's weights: the seeded state with the centring whitening bias (from the golden file unless given)."""
    sd = dict(weights(RETRIEVAL["K"], RETRIEVAL["whiten_out"]))
    sd["whiten.bias"] = torch.from_numpy(np.asarray(_gold("retrieval")["whiten_bias"] if whiten_bias is None else whiten_bias, dtype=np.float32).copy())
    return sd


@functools.lru_cache(maxsize=None)
def weights(K: int = 64, whiten_out=4096):
    return weights_mod.synthetic_netvlad_state(WEIGHT_SEED, K, whiten_out)


@functools.lru_cache(maxsize=None)
def _gold(name):
    with np.load(GOLD / f"netvlad_{name}.npz") as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def error_floor() -> float:
    """The largest error of the reference fp32 module over all golden cases."""
    return max(float(np.abs(_gold(n)["module"].astype(np.float64) - _gold(n)["fp64"]).max()) for n in GOLDEN_CASES)


def record(label, **res):
    """Measured figures behind an assertion: profiles/netvlad_parity.json, one entry per label (rewritten in place)."""
    try:
        data = json.loads(PARITY.read_text()) if PARITY.exists() else {}
        data[label] = {k: (v if isinstance(v, (int, float, str, bool)) else str(v)) for k, v in res.items()}
        PARITY.write_text(json.dumps(data, indent=1, sort_keys=True) + "\n")
    except OSError:
        pass


def make_net(lib, device, hw, K=64, whiten_out=4096, max_batch=1, **conf):
    return nv_mod.NetVLADHIP(weights(K, whiten_out), {"whiten": bool(whiten_out), **conf}, max_batch=max_batch, max_hw=hw, device=device, lib=lib)


def run(net, imgs, device):
    """[B,H,W,3] images through extract_batch with the range-guard counters read: (descriptors on the CPU, guard total)."""
    x = torch.from_numpy(np.ascontiguousarray(imgs)).contiguous().to(device)
    capi.check(net.lib, net.lib.dim_saturation_reset(net._stream()))
    d = net.extract_batch(x)
    total, _ = capi.saturation(net.lib, net._stream(), reset=True)
    return d.cpu(), total


def golden(lib, device, name):
    case, g = GOLDEN_CASES[name], _gold(name)
    net = make_net(lib, device, case["shape"], case["K"], case["whiten_out"])
    d, sat = run(net, image(case)[None], device)
    d = d[0].numpy()
    assert d.shape == g["fp64"].shape and np.isfinite(d).all()
    ref_err = float(np.abs(g["module"].astype(np.float64) - g["fp64"]).max())
    dev_err = float(np.abs(d.astype(np.float64) - g["fp64"]).max())
    bound = max(2 * ref_err, error_floor())
    print(f"netvlad {name} [{device}]: device error {dev_err:.3e}, module error {ref_err:.3e}, bound {bound:.3e}, guard {sat}")
    record(f"{name}:{device}", device_error=dev_err, module_error=ref_err, bound=bound, guard=sat, norm=float(np.linalg.norm(d.astype(np.float64))))
    assert sat == 0
    assert abs(np.linalg.norm(d.astype(np.float64)) - 1.0) < 1e-5
    assert dev_err <= bound, (dev_err, ref_err, bound)


# ---- the two operator entries against fp64 numpy -----------------------------------------------------------------------------------------
def _head_fp64(x, score_w, centers):
    """x [b,n,512], score_w (K,512), centers (512,K) in fp64 numpy: NV:138 and NV:28-39."""
    xh = x / np.maximum(np.linalg.norm(x, axis=2, keepdims=True), 1e-12)
    s = xh @ score_w.T
    s = np.exp(s - s.max(axis=2, keepdims=True))
    s /= s.sum(axis=2, keepdims=True)
    v = np.einsum("bnk,bnd->bdk", s, xh) - centers[None] * s.sum(axis=1)[:, None, :]
    v = v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-12)
    v = v.reshape(v.shape[0], -1)
    return v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-12)


def head_op(lib, device, n, batch, K=64):
    """dim_op_netvlad_head_f32 against fp64 numpy.  Bound: the fp32 torch restatement's own error on the same input, doubled, and never below
    2^-24 (half an ulp of a value in [0.5, 1): the rounding of the largest element a unit-norm vector can hold)."""
    g = torch.Generator().manual_seed(1000 * n + batch + K)
    x = torch.randn(batch, n, 512, generator=g) * 3.0
    sd = weights(K, None)
    sw, c = sd["netvlad.score_proj.weight"], sd["netvlad.centers"]
    got = nv_mod.netvlad_head(x.to(device), sw, c, lib=lib).cpu().numpy().astype(np.float64)
    ref64 = _head_fp64(x.double().numpy(), sw[:, :, 0].double().numpy(), c.double().numpy())
    ref32 = netvlad_ref.head(x.permute(0, 2, 1).contiguous(), sw, c).numpy().astype(np.float64)
    dev_err, ref_err = float(np.abs(got - ref64).max()), float(np.abs(ref32 - ref64).max())
    bound = max(2 * ref_err, 2.0 ** -24)
    print(f"netvlad head op [{device}] n={n} b={batch} K={K}: device {dev_err:.3e}, torch fp32 {ref_err:.3e}, bound {bound:.3e}")
    record(f"head_op:n{n}:b{batch}:K{K}:{device}", device_error=dev_err, torch_fp32_error=ref_err, bound=bound)
    assert dev_err <= bound, (dev_err, ref_err, bound)
    if batch > 1:   # an image's result does not depend on the batch around it
        one = nv_mod.netvlad_head(x[1:2].contiguous().to(device), sw, c, lib=lib).cpu().numpy().astype(np.float64)
        assert np.array_equal(one[0], got[1])


def whiten_op(lib, device, batch, n_in=4096 * 2, n_out=37):
    """dim_op_netvlad_whiten_f32 against fp64 numpy, same bound rule; out_dim 37 is no multiple of the 16 rows a workgroup owns nor of the 4 a wave owns."""
    g = torch.Generator().manual_seed(77 + batch)
    v = torch.nn.functional.normalize(torch.randn(batch, n_in, generator=g), dim=1)
    W = torch.randn(n_out, n_in, generator=g) / n_in ** 0.5
    b = 0.01 * torch.randn(n_out, generator=g)
    got = nv_mod.netvlad_whiten(v.to(device), W.to(device), b.to(device), lib=lib).cpu().numpy().astype(np.float64)
    y = v.double().numpy() @ W.double().numpy().T + b.double().numpy()
    ref64 = y / np.maximum(np.linalg.norm(y, axis=1, keepdims=True), 1e-12)
    ref32 = netvlad_ref.whiten(v, W, b).numpy().astype(np.float64)
    dev_err, ref_err = float(np.abs(got - ref64).max()), float(np.abs(ref32 - ref64).max())
    bound = max(2 * ref_err, 2.0 ** -24)
    print(f"netvlad whiten op [{device}] b={batch}: device {dev_err:.3e}, torch fp32 {ref_err:.3e}, bound {bound:.3e}")
    record(f"whiten_op:b{batch}:{device}", device_error=dev_err, torch_fp32_error=ref_err, bound=bound)
    assert dev_err <= bound, (dev_err, ref_err, bound)
    if batch > 1:   # the same bits for every batch size (1, 2, 4, 8 and 16 images per pass are separate instantiations)
        one = nv_mod.netvlad_whiten(v[1:2].contiguous().to(device), W.to(device), b.to(device), lib=lib).cpu().numpy().astype(np.float64)
        assert np.array_equal(one[0], got[1])


# ---- properties of the resident handle ------------------------------------------------------------------------------------------------------
def batch_and_reuse(lib, device):
    """Batch 3 equals three single calls bit for bit; a handle that has run a larger image gives a smaller one the bits of a fresh handle."""
    rng = np.random.default_rng(11)
    imgs = rng.integers(0, 256, size=(3, 34, 50, 3)).astype(np.float32) / np.float32(255.0)
    net = make_net(lib, device, (48, 64), 8, 256, max_batch=3)
    both, sat = run(net, imgs, device)
    assert sat == 0
    for i in range(3):
        one, _ = run(net, imgs[i:i + 1], device)
        assert torch.equal(one[0], both[i]), i
    fresh = make_net(lib, device, (34, 50), 8, 256)
    again, _ = run(fresh, imgs[2:3], device)
    assert torch.equal(again[0], both[2])


def no_whiten_equals_head(lib, device):
    """conf whiten False: the handle's output is the head operator's output on the handle's own conv5_3 map, bit for bit; and whitening it with the
    whitening operator gives the whitened handle's bits."""
    case = GOLDEN_CASES["smallk"]
    img = image(case)[None]
    sd = weights(8, 256)
    net = make_net(lib, device, case["shape"], 8, None)
    plain, _ = run(net, img, device)
    fmap = net.debug_map()
    assert fmap.shape == (1, 3, 4, 512)
    via_head = nv_mod.netvlad_head(fmap.reshape(1, 12, 512).to(device), sd["netvlad.score_proj.weight"], sd["netvlad.centers"], lib=lib).cpu()
    assert torch.equal(via_head, plain)
    white, _ = run(make_net(lib, device, case["shape"], 8, 256), img, device)
    assert plain.shape == (1, 512 * 8) and white.shape == (1, 256)
    via_op = nv_mod.netvlad_whiten(plain.to(device), sd["whiten.weight"].to(device), sd["whiten.bias"].to(device), lib=lib).cpu()
    assert torch.equal(via_op, white)
    # ... and the unwhitened vector is what the reference's NetVLAD layer makes of it: intra-normalised columns, unit norm
    v = plain[0].double().numpy().reshape(512, 8)
    assert abs(np.linalg.norm(v) - 1.0) < 1e-5 and np.allclose(np.linalg.norm(v, axis=0), 1.0 / np.sqrt(8.0), atol=1e-5)


def guard(lib, device, nan_pixel=False):
    """Convolution weights scaled up until conv1_1's activations leave |x| <= 4094: the plain call reports the site, the guarded call repeats in
    the bf16 split and returns a finite unit-norm descriptor and leaves the counters at zero.  nan_pixel: a NaN pixel trips the guard of an
    otherwise clean handle as well."""
    sd = dict(weights(8, None))
    sd["backbone.0.weight"] = sd["backbone.0.weight"] * 64.0
    net = nv_mod.NetVLADHIP(sd, {"whiten": False}, max_hw=(16, 16), device=device, lib=lib)
    img = image(GOLDEN_CASES["min"])[None]
    _, sat = run(net, img, device)
    assert sat > 0
    d = net.extract_batch_guarded(torch.from_numpy(img).to(device)).cpu()
    assert torch.isfinite(d).all() and abs(float(d.double().norm()) - 1.0) < 1e-5
    total, _ = capi.saturation(lib, net._stream(), reset=True)
    assert total == 0
    if nan_pixel:
        clean = make_net(lib, device, (16, 16), 8, None)
        bad = img.copy()
        bad[0, 3, 5, 1] = float("nan")
        _, sat = run(clean, bad, device)
        assert sat > 0


def selector(lib, device):
    """RetrievalPairSelector on the 8-image fixture: the pair list equals the one derived from the reference module's descriptors."""
    r = RETRIEVAL
    names, images = retrieval_images()
    g = _gold("retrieval")
    sel = pairs_mod.RetrievalPairSelector(retrieval_state(), device=device, lib=lib, max_batch=4)
    got = sel.select(names, images, num_matched=r["num_matched"])
    want = [(str(a), str(b)) for a, b in g["pairs"]]
    assert got == want, (got, want)
    per_query = {n: sum(1 for a, _ in want if a == n) for n in names}
    assert per_query["7"] == 0 and max(per_query.values()) == r["num_matched"]   # both cuts act in this fixture
    full = sel.describe(images)
    # mixed sizes are batched size by size and come back in list order: rows equal the same-sized call's rows bit for bit
    mixed = sel.describe([images[0], images[1][:48, :64], images[2], images[3][:48, :64], images[4]])
    assert torch.equal(mixed[[0, 2, 4]], full[[0, 2, 4]])
    assert torch.equal(mixed[[1, 3]], sel.describe([images[1][:48, :64], images[3][:48, :64]]))
    d = full.cpu().numpy().astype(np.float64)
    err = float(np.abs(d - g["fp64"]).max())
    print(f"netvlad retrieval fixture [{device}]: descriptor error {err:.3e}, smallest rank gap {float(g['min_gap']):.3e}")
    record(f"retrieval:{device}", descriptor_error=err, min_gap=float(g["min_gap"]), pairs=len(got))


def selector_resize(lib, device):
    """RetrievalPairSelector.preprocess: an image above resize_max is down-sampled to int(round(x * scale)) with the area kernel — at the exact
    factor 2 INTER_AREA is the mean of 2 x 2 blocks (OpenCV adds the four values, then scales) — and handed on in 0..1; smaller images are only
    divided by 255."""
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, size=(32, 2048, 3)).astype(np.float32)
    sel = pairs_mod.RetrievalPairSelector(weights(RETRIEVAL["K"], RETRIEVAL["whiten_out"]), device=device, lib=lib)
    out = sel.preprocess(img).cpu().numpy()
    assert out.shape == (16, 1024, 3)
    want = img.reshape(16, 2, 1024, 2, 3).astype(np.float64).sum(axis=(1, 3)) / 4.0 / 255.0
    assert np.abs(out - want).max() < 1e-6, np.abs(out - want).max()
    small = sel.preprocess(img[:, :1024]).cpu().numpy()
    assert small.shape == (32, 1024, 3) and np.abs(small - img[:, :1024] / 255.0).max() < 1e-7
    odd = sel.preprocess(np.zeros((37, 1500, 3), np.float32))
    assert tuple(odd.shape) == (int(round(37 * 1024 / 1500)), 1024, 3)


def describe_mixed(lib, device, n=5):
    """RetrievalPairSelector.describe on a list of mixed sizes: batched size by size through one staging buffer per size, rows back in list order and
    bit-equal to describing every image on its own; a non-finite pixel is refused on the host."""
    rng = np.random.default_rng(9)
    imgs = [rng.integers(0, 256, size=s).astype(np.float32) for s in ((16, 16, 3), (16, 32, 3), (16, 16, 3), (16, 32, 3), (16, 16, 3))][:n]
    sel = pairs_mod.RetrievalPairSelector(weights(RETRIEVAL["K"], RETRIEVAL["whiten_out"]), device=device, lib=lib, max_batch=2)
    table = sel.describe(imgs).cpu()
    assert table.shape == (n, RETRIEVAL["whiten_out"])
    for i, im in list(enumerate(imgs))[1:]:   # (16, 32) sits between two (16, 16): its row and the row behind it went through the gather
        assert torch.equal(sel.describe([im]).cpu()[0], table[i]), i
    bad = imgs[0].copy()
    bad[2, 3, 1] = np.inf
    try:
        sel.describe([bad])
    except ValueError as e:
        assert "non-finite" in str(e)
    else:
        raise AssertionError("a non-finite pixel was accepted")
