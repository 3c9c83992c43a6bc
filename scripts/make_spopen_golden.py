"""Regenerates tests/golden/spopen_<case>.npz from the REFERENCE's open SuperPoint module (thirdparty/SuperPoint_open/superpoint_pytorch.py).
Needs the reference tree (environment variable DIM_REFERENCE_ROOT = its checkout) and runs on the CPU only; nothing of the reference's program
text is copied: its one file is imported by path and fed the seeded synthetic weights and images of tests/spopen_cases.py.  The extractor hook's
zero padding to multiples of 8 (extractors/superpoint_open.py:131-135) is restated by spopen_cases.image.

Per case the file holds the inputs as seeds (+ the padded size and a sha1 of the state dict), the module's outputs, its intermediate maps
(conv1b's pooled stage at a sample of rows and columns, encoder, score map, un-normalised dense descriptors) and the module's fp64
evaluation of scores, descriptors and score map.  Asserted here, for every case: fp32 and fp64 give the same keypoints in the same order; no fp64
NMS maximum lies within MARGIN of the threshold, nor the k-th within MARGIN of the (k+1)-th; sorted outputs have distinct neighbours; the module's
NMS equals oracle.simple_nms bit for bit.

    DIM_REFERENCE_ROOT=... python scripts/make_spopen_golden.py
"""
from __future__ import annotations

import copy
import importlib.util
import os
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
REF = Path(os.environ["DIM_REFERENCE_ROOT"]) / "src/deep_image_matching/thirdparty/SuperPoint_open/superpoint_pytorch.py"

from oracle import superpoint_ref  # noqa: E402
from tests import spopen_cases as cases  # noqa: E402

MARGIN = 1e-4


def reference_module():
    spec = importlib.util.spec_from_file_location("ref_superpoint_open", str(REF))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    orig = mod.sample_descriptors
    # the module casts keypoints with .float(): in the fp64 evaluation grid_sample then refuses the mixed dtypes
    mod.sample_descriptors = lambda k, d, s=8: orig(k.to(d.dtype), d, s)
    return mod


def evaluate(mod, case, dtype):
    cfg = case["cfg"]
    k = cfg["max_keypoints"]
    net = mod.SuperPoint(detection_threshold=cfg["keypoint_threshold"], max_num_keypoints=None if k < 0 else k, nms_radius=cfg["nms_radius"],
                         remove_borders=cfg["remove_borders"], descriptor_dim=256).eval()
    net.load_state_dict({k_: v for k_, v in cases.weights(case).items()})
    net = copy.deepcopy(net).to(dtype)
    img = cases.image(case).to(dtype)
    with torch.no_grad():
        out = net({"image": img})
        b1 = net.backbone[0](img)
        c2a = net.backbone[1][0](b1)
        feat = net.backbone(img)
        dd = net.descriptor(feat)
        sc = torch.softmax(net.detector(feat), 1)[:, :-1]
        b, _, h, w = sc.shape
        smap = sc.permute(0, 2, 3, 1).reshape(b, h, w, 8, 8).permute(0, 1, 3, 2, 4).reshape(b, h * 8, w * 8)
        nms = mod.batched_nms(smap, cfg["nms_radius"])
    return {"keypoints": out["keypoints"][0], "scores": out["keypoint_scores"][0], "descriptors": out["descriptors"][0].t().contiguous(),
            "conv1b": b1, "conv2a": c2a, "encoder": feat, "dense_desc": dd, "score_map": smap[0], "nms_map": nms[0]}


def sample_index(n: int) -> np.ndarray:
    return np.unique(np.concatenate([np.arange(0, n, 3), [0, 1, n - 2, n - 1]])).astype(np.int32)


def main():
    mod = reference_module()
    for name, case in cases.CASES.items():
        cfg = case["cfg"]
        r32, r64 = evaluate(mod, case, torch.float32), evaluate(mod, case, torch.float64)
        n = r32["keypoints"].shape[0]
        assert torch.equal(r32["keypoints"].long(), r64["keypoints"].long()), f"{name}: fp32 and fp64 keypoints differ - pick another seed"
        assert torch.equal(superpoint_ref.simple_nms(r32["score_map"][None], cfg["nms_radius"])[0], r32["nms_map"]), name
        # decision margins in fp64: candidates = NMS maxima inside the border
        rb = cfg["remove_borders"]
        inner = r64["nms_map"][rb:-rb, rb:-rb] if rb else r64["nms_map"]
        maxima = inner[inner > 0]
        thr_gap = (maxima - cfg["keypoint_threshold"]).abs().min().item()
        assert thr_gap >= MARGIN, f"{name}: an fp64 score lies {thr_gap:.2e} from the threshold - pick another seed"
        cand = torch.sort(maxima[maxima > cfg["keypoint_threshold"]], descending=True).values
        k = cfg["max_keypoints"]
        if 0 < k < len(cand):
            assert n == k and (cand[k - 1] - cand[k]).item() >= MARGIN, f"{name}: k-th and (k+1)-th fp64 scores are {float(cand[k - 1] - cand[k]):.2e} apart"
            gaps = (r64["scores"][:-1] - r64["scores"][1:]).min().item()
            assert gaps >= 1e-5, f"{name}: sorted fp64 scores {gaps:.2e} apart: the order is not pinned"
        else:
            assert n == len(cand), (name, n, len(cand))
        rows, cols = sample_index(r32["conv1b"].shape[2]), sample_index(r32["conv1b"].shape[3])
        nhwc = lambda t: t[0].permute(1, 2, 0).contiguous().numpy()  # noqa: E731
        c2a = r32["conv2a"][0, cases.GUARD_CHANNEL]
        res = lambda x64, x32: (x64 - x32.double()).float().numpy()  # noqa: E731
        Hp, Wp = cases.padded(case["H"]), cases.padded(case["W"])
        np.savez_compressed(
            ROOT / "tests" / "golden" / f"spopen_{name}.npz",
            H=case["H"], W=case["W"], Hp=Hp, Wp=Wp, seed=case["seed"], state_dict_sha1=cases.state_dict_sha1(cases.weights(case)),
            keypoints=r32["keypoints"].numpy(), scores=r32["scores"].numpy(), descriptors=r32["descriptors"].numpy(),
            conv1b=nhwc(r32["conv1b"])[rows][:, cols], conv1b_rows=rows, conv1b_cols=cols, encoder=nhwc(r32["encoder"]),
            dense_desc=nhwc(r32["dense_desc"]), score_map=r32["score_map"].numpy(),
            # the fp64 evaluation as its float32 residual from the fp32 one (fp64 = fp32 + residual to ~1e-14: half the bytes)
            scores64_res=res(r64["scores"], r32["scores"]), descriptors64_res=res(r64["descriptors"], r32["descriptors"]),
            score_map64_res=res(r64["score_map"], r32["score_map"]),
            guard_min=float(c2a.min()), guard_max=float(r32["conv2a"].max()))
        size = (ROOT / "tests" / "golden" / f"spopen_{name}.npz").stat().st_size
        assert size < (1 << 20), (name, size)
        neg = float((r32["conv1b"] < 0).float().mean())
        print(f"{name}: {Hp}x{Wp} keypoints {n} candidates {len(cand)} threshold gap {thr_gap:.2e} score range [{float(r32['scores'].min()):.4f}, "
              f"{float(r32['scores'].max()):.4f}] negative conv1b share {neg:.2f} conv2a[guard channel] min {float(c2a.min()):.1f} file {size} B "
              f"score map fp32 vs fp64 {float((r32['score_map'].double() - r64['score_map']).abs().max()):.2e}")


if __name__ == "__main__":
    main()
