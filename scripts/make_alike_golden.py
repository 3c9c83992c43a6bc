"""Regenerates tests/golden/alike_<case>.npz from the REFERENCE's ALIKE modules (thirdparty/alike/{alnet,alike,soft_detect}.py) and pins
tests/alike_ref.py to them bit for bit.  Needs the reference tree (environment variable DIM_REFERENCE_ROOT = its checkout) and runs
on the CPU only; nothing of the reference's program text is copied: its three files are imported by path with two stand-ins
(torchvision.models.resnet.conv3x3 / conv1x1 -> bias-free nn.Conv2d factories, cv2 -> an empty module: it is only touched when
image_size_max forces a resize, which deep-image-matching never does).

    python scripts/make_alike_golden.py            # writes the four golden files, copies the four checkpoints (in parts) to tests/golden/alike/
"""
from __future__ import annotations

import importlib
import os
import sys
import types
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
REF = Path(os.environ["DIM_REFERENCE_ROOT"]) / "src/deep_image_matching/thirdparty/alike"   # the reference checkout

from tests import alike_cases, alike_ref  # noqa: E402


def reference_module():
    tv, models, resnet = types.ModuleType("torchvision"), types.ModuleType("torchvision.models"), types.ModuleType("torchvision.models.resnet")
    resnet.conv1x1 = lambda i, o, stride=1: torch.nn.Conv2d(i, o, 1, stride=stride, bias=False)
    resnet.conv3x3 = lambda i, o, stride=1, groups=1, dilation=1: torch.nn.Conv2d(i, o, 3, stride=stride, padding=dilation, bias=False)
    tv.models, models.resnet = models, resnet
    for n, m in {"torchvision": tv, "torchvision.models": models, "torchvision.models.resnet": resnet, "cv2": types.ModuleType("cv2")}.items():
        sys.modules[n] = m
    pkg = types.ModuleType("ref_alike")
    pkg.__path__ = [str(REF)]
    sys.modules["ref_alike"] = pkg
    return importlib.import_module("ref_alike.alike")


def main():
    mod = reference_module()
    dst = ROOT / "tests" / "golden" / "alike"
    dst.mkdir(parents=True, exist_ok=True)
    for m in ("t", "s", "n", "l"):   # byte copies, cut into parts of at most PART bytes (the repository's limit for one file is 1 MiB)
        data = (REF / "models" / f"alike-{m}.pth").read_bytes()
        for old in dst.glob(f"alike-{m}.pth*"):
            old.unlink()
        for i in range(0, len(data), alike_cases.PART):
            (dst / f"alike-{m}.pth.{i // alike_cases.PART}").write_bytes(data[i:i + alike_cases.PART])
    for name, case in alike_cases.GOLDEN_CASES.items():
        cfg = case["cfg"]
        crop = alike_cases.crop(case)
        conf = dict(mod.configs[cfg["model"]])
        net = mod.ALike(**conf, device="cpu", top_k=cfg["top_k"], scores_th=cfg["scores_th"], n_limit=cfg["n_limit"])
        assert not net.training
        got = net(crop, sub_pixel=True)
        sd = alike_cases.weights(cfg["model"])
        mine = alike_ref.alike_forward(crop, sd, cfg, taps=True)
        # restatement == reference module, bit for bit
        assert np.array_equal(got["keypoints"], mine["keypoints"].numpy()), name
        assert np.array_equal(got["scores"], mine["scores"].numpy()), name
        assert np.array_equal(got["descriptors"], mine["descriptors"].t().numpy()), name
        assert np.array_equal(got["scores_map"], mine["score_map"].numpy()), name
        np.savez_compressed(ROOT / "tests" / "golden" / f"alike_{name}.npz", image=crop, keypoints=got["keypoints"], scores=got["scores"],
                            descriptors=np.ascontiguousarray(got["descriptors"].T), score_map=got["scores_map"][0, 0])
        print(name, cfg["model"], crop.shape, "keypoints", got["keypoints"].shape[0], "restatement == reference: bit-identical")


if __name__ == "__main__":
    main()
