"""Regenerates tests/golden/xfeat_<case>.npz from the REFERENCE's XFeat modules (thirdparty/accelerated_features/modules/{xfeat,model,
interpolator}.py) and pins tests/xfeat_ref.py to them bit for bit.  Needs the reference tree (environment variable DIM_REFERENCE_ROOT = its
checkout) and runs on the CPU only; nothing of the reference's program text is copied: its files are imported by path (tqdm, which xfeat.py
imports and the sparse path never uses, is replaced by an empty module when it is not installed).

Per case the script asserts: (a) restatement == module, bit for bit; (b) the fp32 and fp64 evaluations select the same pixel set; (c) at most
MAX_NEAR_TIES fp64 decisions lie within TIE_TOL of the threshold or of a neighbour in the 5 x 5 window; (d) the case's structural property.
A case that fails (b)-(d) gets another seed in tests/xfeat_cases.py, not a looser bound.

    python scripts/make_xfeat_golden.py            # writes the golden files
    python scripts/make_xfeat_golden.py --time     # times the reference module on this machine's CPU cores at 1024 x 1024
"""
from __future__ import annotations

import importlib
import os
import sys
import time
import types
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
REF = Path(os.environ["DIM_REFERENCE_ROOT"]) / "src/deep_image_matching/thirdparty/accelerated_features"   # the reference checkout

from tests import xfeat_cases, xfeat_ref  # noqa: E402


def reference_module(sd):
    try:
        import tqdm  # noqa: F401
    except ImportError:
        sys.modules["tqdm"] = types.ModuleType("tqdm")
    sys.path.insert(0, str(REF))
    mod = importlib.import_module("modules.xfeat")
    net = mod.XFeat(weights=None)
    net.dev = torch.device("cpu")
    net.net = net.net.to("cpu").eval()
    missing, unexpected = net.net.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("fine_matcher.") for k in missing), (missing, unexpected)
    return net


@torch.no_grad()
def main():
    sd = xfeat_cases.weights()
    net = reference_module(sd)
    if "--time" in sys.argv:
        img = np.random.default_rng(0).integers(0, 256, size=(1024, 1024, 3)).astype(np.float32)
        net.detectAndCompute(img, top_k=4096)
        t0 = time.perf_counter()
        for _ in range(3):
            net.detectAndCompute(img, top_k=4096)
        print(f"reference XFeat, CPU, {torch.get_num_threads()} threads, 1024 x 1024, top_k 4096: {(time.perf_counter() - t0) / 3 * 1e3:.1f} ms per image")
        return
    for name, case in xfeat_cases.GOLDEN_CASES.items():
        img = xfeat_cases.image(case)
        got = net.detectAndCompute(img, top_k=case["top_k"])[0]
        mine = xfeat_ref.xfeat_forward(img, sd, top_k=case["top_k"], taps=True)
        x, _, _ = net.preprocess_tensor(img)
        M1, K1, H1 = net.net(x)
        K1h = net.get_kpts_heatmap(K1)
        for k in ("keypoints", "scores", "descriptors"):   # (a)
            assert got[k].shape == mine[k].shape and torch.equal(got[k], mine[k]), (name, k)
        assert torch.equal(K1h[0, 0], mine["K1h"]) and torch.equal(H1[0, 0], mine["H1"]), name
        m64 = xfeat_ref.xfeat_forward(img, sd, top_k=1 << 30, taps=True, dtype=torch.float64)
        all32 = xfeat_ref.xfeat_forward(img, sd, top_k=1 << 30, taps=True)
        s32, s64 = {tuple(p) for p in all32["pixels"].tolist()}, {tuple(p) for p in m64["pixels"].tolist()}
        assert s32 == s64, (name, "fp32 and fp64 select different pixels", s32 ^ s64)   # (b)
        near = int(xfeat_cases.near_decisions(m64["K1h"]).sum())
        assert near <= xfeat_cases.MAX_NEAR_TIES, (name, "near ties", near)   # (c)
        _H, _W = mine["hw"]
        n = got["keypoints"].shape[0]
        if name == "ragged":   # (d)
            pos = xfeat_ref.nms(K1h)[0]
            dropped = int(((pos[:, 0] == _W - 1) | (pos[:, 1] == _H - 1)).sum())
            kept = int(((all32["pixels"][:, 0] == 0) | (all32["pixels"][:, 1] == 0)).sum())
            assert dropped >= 1 and kept >= 1 and (_H, _W) == (96, 128), (dropped, kept)
            print("   ragged: dropped last-row / last-column maxima", dropped, "kept first-row / first-column keypoints", kept)
        if name == "topk":
            assert len(all32["pixels"]) > case["top_k"] and n == case["top_k"]
        if name == "min32":
            assert (_H, _W) == (32, 32) and n > 0
        if name == "gray":
            assert img.ndim == 2 and (_H, _W) == (32, 64) and n > 0
        np.savez_compressed(ROOT / "tests" / "golden" / f"xfeat_{name}.npz", image=img.astype(np.uint8), keypoints=got["keypoints"].numpy(),
                            scores=got["scores"].numpy(), descriptors=got["descriptors"].numpy(), K1h=K1h[0, 0].numpy(), H1=H1[0, 0].numpy(),
                            K1h_res64=(m64["K1h"] - K1h[0, 0].double()).float().numpy(), H1_res64=(m64["H1"] - H1[0, 0].double()).float().numpy())
        print(name, img.shape, "->", (_H, _W), "keypoints", n, "candidates", len(all32["pixels"]), "near ties", near, "restatement == reference: bit-identical")


if __name__ == "__main__":
    main()
