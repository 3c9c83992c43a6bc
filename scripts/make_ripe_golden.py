"""Regenerates tests/golden/ripe_<case>.npz from the REFERENCE's RIPE module (thirdparty/RIPE/ripe, built by model_zoo.vgg_hyper) and pins
tests/ripe_ref.py to it bit for bit.  Needs the reference tree (environment variable DIM_REFERENCE_ROOT = its checkout) and runs on the CPU only;
nothing of the reference's program text is copied: its files are imported by path.

Neither torchvision nor ripe_weights.pth is available offline, so
  * a stand-in ``torchvision`` is put into sys.modules whose ``models.vgg19_bn().features`` is the standard layer list (configuration E with
    BatchNorm: 64,64,M,128,128,M,256 x 4,M,512 x 4,M,512 x 4,M) and whose ``transforms.functional.resize`` (imported by ripe/utils, never called on
    this path) raises, and
  * the seeded synthetic state (weights.synthetic_ripe_state_dict) is written with torch.save and handed to vgg_hyper(model_path), which then loads it
    with load_state_dict(strict): the keys are the reference's own.  A path is always given, so the download branch is never reached.
The reference's detectAndCompute then runs unmodified, in fp32.

Per case the script asserts that the restatement equals the module bit for bit in fp32 (heat map, keypoints, descriptors, scores), evaluates the
restatement in fp64, and checks the conditions tests/ripe_cases.py relies on: 20 .. 200 keypoints, fewer near-tie pixels (tolerance = 4 x the
module's own heat-map error) than 2 % of the keypoints, and a top-k cut that no other candidate lies within the tolerance of.

    python scripts/make_ripe_golden.py
"""
from __future__ import annotations

import importlib
import importlib.util
import os
import sys
import tempfile
import types
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
REF_SRC = Path(os.environ["DIM_REFERENCE_ROOT"]) / "src"
PKG = "deep_image_matching"

from tests import ripe_cases as cases, ripe_ref  # noqa: E402


def _vgg19_bn_stand_in():
    from torch import nn

    class VGG(nn.Module):
        def __init__(self):
            super().__init__()
            layers, cin = [], 3
            for v in (64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512, 512, 512, 512, "M"):
                if v == "M":
                    layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
                else:
                    layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.BatchNorm2d(v), nn.ReLU(inplace=True)]
                    cin = v
            self.features = nn.Sequential(*layers)

    return lambda *a, **k: VGG()


def install_reference():
    def _unavailable(*a, **k):
        raise RuntimeError("torchvision is not installed: stand-in")

    tv, tvm, tvt, tvf = (types.ModuleType(n) for n in ("torchvision", "torchvision.models", "torchvision.transforms", "torchvision.transforms.functional"))
    tvm.vgg19_bn = _vgg19_bn_stand_in()
    tvf.resize = _unavailable
    tv.models, tv.transforms, tvt.functional = tvm, tvt, tvf
    for m in (tv, tvm, tvt, tvf):
        sys.modules[m.__name__] = m
    if importlib.util.find_spec("cv2") is None:   # ripe/utils/utils.py imports it for its image helpers; nothing on this path calls it
        cv2 = types.ModuleType("cv2")
        cv2.__getattr__ = lambda name: type(name, (), {})   # its names appear in annotations only (cv2.DMatch, cv2.KeyPoint)
        sys.modules["cv2"] = cv2
    for sub in ("", ".thirdparty", ".thirdparty.RIPE"):   # empty packages: no __init__ of the reference's upper levels runs
        mod = types.ModuleType(PKG + sub)
        mod.__path__ = [str(REF_SRC / PKG / sub.strip(".").replace(".", "/"))] if sub else [str(REF_SRC / PKG)]
        mod.__package__ = PKG + sub
        sys.modules[PKG + sub] = mod
    return importlib.import_module(PKG + ".thirdparty.RIPE.ripe")


@torch.no_grad()
def main():
    ripe = install_reference()
    out = ROOT / "tests" / "golden"
    sd = cases.weights()
    with tempfile.TemporaryDirectory() as tmp:
        path = Path(tmp) / "ripe_weights.pth"
        torch.save(sd, path)
        model = ripe.vgg_hyper(path).eval()
    assert set(model.state_dict()) == set(sd)
    for name, case in cases.GOLDEN_CASES.items():
        img = cases.image(case)
        t = cases.to_tensor(img)
        thr, top_k = case["threshold"], case["top_k"]
        kp, desc, sc, aux = model.detectAndCompute(t, threshold=thr, top_k=top_k, output_aux=True)
        heat = aux["heatmap"][0, 0]
        r32 = ripe_ref.ripe_forward(t, sd, torch.float32, thr, top_k)
        for k, v in (("heat", heat), ("keypoints", kp), ("descriptors", desc), ("scores", sc)):
            assert r32[k].shape == v.shape and torch.equal(r32[k], v), f"{name}: tests/ripe_ref.py differs from the reference module in {k}"
        heat64, feats64 = ripe_ref.heat_map(t, sd, torch.float64)
        H, W = heat64.shape
        xy = kp.long()
        desc64 = ripe_ref.describe(feats64, xy, H, W, {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()})
        sc64 = heat64[xy[:, 1], xy[:, 0]] / heat64.max()
        err = {"heat": float((heat.double() - heat64).abs().max()), "scores": float((sc.double() - sc64).abs().max()),
               "descriptors": float((desc.double() - desc64).abs().max())}
        tol = 4.0 * err["heat"]
        n = kp.shape[0]
        assert 20 <= n <= 200, f"{name}: {n} keypoints"
        near, cut, budget = cases.tie_budget(heat64, thr, top_k, tol)
        assert budget < cases.MAX_NEAR_TIE_SHARE * n, f"{name}: {budget} near-tie pixels against {n} keypoints"
        cand = cases.candidates(heat64, thr)
        if len(cand) > top_k:
            assert n == top_k and float(cand[top_k - 2] - cand[top_k - 1]) > tol and float(cand[top_k - 1] - cand[top_k]) > tol, f"{name}: the top-k cut is a near tie"
        r64 = ripe_ref.ripe_forward(t, sd, torch.float64, thr, top_k)
        assert torch.equal(r64["keypoints"].long(), xy), f"{name}: fp32 and fp64 select or order the keypoints differently"
        peaks = cases.candidates(heat64, 0.0)
        print(f"{name}: {n} keypoints of {len(cand)} candidates ({len(peaks)} maxima above 0), module fp32 error heat {err['heat']:.3e} scores {err['scores']:.3e} "
              f"descriptors {err['descriptors']:.3e}, near-tie pixels {budget}, max |heat| {float(heat64.abs().max()):.2f}")
        np.savez_compressed(out / f"ripe_{name}.npz", image=img, heat=heat.numpy(), heat_res64=(heat64 - heat.double()).float().numpy(),
                            keypoints=kp.numpy(), scores=sc.numpy(), descriptors=desc.numpy(), scores64=sc64.numpy(), descriptors64=desc64.numpy(),
                            err_heat=np.float64(err["heat"]), err_scores=np.float64(err["scores"]), err_descriptors=np.float64(err["descriptors"]))


if __name__ == "__main__":
    main()
