"""Device time of the XFeat extractor (dim_xfeat_extract) next to ALIKE alike-t and SuperPoint at the same shape and keypoint count.

    python scripts/bench_xfeat.py            # every step in this process, one JSON line at the end
    python scripts/bench_xfeat.py --quick    # a few calls per network only (the kernel-trace pass: rocprofv3 --kernel-trace --stats -- python ...)

Shape: 1024 x 1024 with batch 16 and batch 1, 4096 keypoints.  Times are HIP-event times of back-to-back extract_batch calls after a warm-up,
best of 3 alternating repeats of a window of at least 0.3 s, reported as milliseconds per IMAGE.  Weights are the seeded synthetic ones (the
arithmetic and the launch shapes do not depend on the values); the input is uniform noise in 0..255 for XFeat and 0..1 for the others.
Result: one line `XFEAT_BENCH {json}` and profiles/xfeat_bench.json.
"""
from __future__ import annotations

import argparse
import importlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
H, W = 1024, 1024
TOP_K = 4096


def timed(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "xfeat_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    weights = importlib.import_module("deep-image-matching_amd.weights")
    xf = importlib.import_module("deep-image-matching_amd.xfeat_hip")
    ak = importlib.import_module("deep-image-matching_amd.alike_hip")
    sp = importlib.import_module("deep-image-matching_amd.superpoint_hip")
    capi = importlib.import_module("deep-image-matching_amd.capi")
    lib = capi.load()
    results = []
    for B in (16, 1):
        rgb = torch.rand(B, H, W, 3, generator=torch.Generator().manual_seed(0)).cuda().contiguous()
        inputs = {"xfeat": (rgb * 255.0).contiguous(), "alike-t": rgb, "superpoint": rgb[..., 0].contiguous()}
        nets = {"xfeat": xf.XFeatHIP(weights.synthetic_xfeat_state_dict(21), {"top_k": TOP_K}, max_batch=B, max_hw=(H, W)),
                "alike-t": ak.AlikeHIP(weights.synthetic_alike_state_dict(11, "alike-t"), {"model": "alike-t", "top_k": TOP_K}, max_batch=B, max_hw=(H, W)),
                "superpoint": sp.SuperPointHIP(weights.synthetic_superpoint_state_dict(1234), {"nms_radius": 4, "keypoint_threshold": 0.005, "max_keypoints": TOP_K,
                                                                                                 "remove_borders": 4}, max_batch=B, max_hw=(H, W))}
        capi.check(lib, lib.dim_saturation_reset(capi.stream_ptr("cuda")))
        outs = {}
        for name, net in nets.items():      # warm-up: code objects, allocations of the outputs
            outs[name] = net.extract_batch(inputs[name])
            for _ in range(2):
                net.extract_batch(inputs[name], out=outs[name])
        torch.cuda.synchronize()
        run = {name: (lambda net=net, name=name: net.extract_batch(inputs[name], out=outs[name])) for name, net in nets.items()}
        iters = {name: 3 if args.quick else max(3, min(500, int(0.3e3 / max(timed(run[name], 3), 1e-3)))) for name in nets}
        ms = {name: [] for name in nets}
        for _ in range(1 if args.quick else 3):
            for name in nets:
                ms[name].append(timed(run[name], iters[name]))
        total, sites = capi.saturation(lib, None)
        row = {"H": H, "W": W, "batch": B, "top_k": TOP_K, "range_guard_total": total, "repeats_ms_per_call": ms,
               "ms_per_image": {name: min(ms[name]) / B for name in nets},
               "keypoints_per_image": {name: float(outs[name][3].float().mean()) for name in nets}}
        results.append(row)
        del nets, outs, run
        torch.cuda.empty_cache()
    doc = {"what": "warm HIP-event extract_batch time per image, best of 3 alternating repeats; synthetic weights, uniform-noise images",
           "device": torch.cuda.get_device_name(0), "shapes": results}
    print("XFEAT_BENCH " + json.dumps(doc), flush=True)
    if not args.quick:
        try:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")
        except OSError:
            pass
    return 0


if __name__ == "__main__":
    sys.exit(main())
