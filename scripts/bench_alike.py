"""Device time of the ALIKE extractor (dim_alike_extract) next to ALIKED (dim_aliked_extract) at the same shapes and keypoint count.

    python scripts/bench_alike.py            # every step in this process, one JSON line at the end
    python scripts/bench_alike.py --quick    # the 480 x 640 shape only

Shapes: 1024 x 1024 with batch 16, and 480 x 640 with batch 1; models alike-t / s / n / l and aliked-n16, all in top-k mode with the same k
(the selection then returns exactly k rows for every model, so the sparse heads do the same amount of work).  Times are HIP-event times of
back-to-back extract_batch calls after a warm-up, best of 3 repeats of a window of at least 0.3 s (device events, warm,
everything compared in one process), reported as milliseconds per IMAGE together with the shader clock the last window held.  Weights are the seeded synthetic ones (the arithmetic and the
launch shapes do not depend on the values); the input is uniform noise, whose score map has more NMS maxima than k.
Result: one line `ALIKE_BENCH {json}` and profiles/alike_bench.json.
"""
from __future__ import annotations

import argparse
import ctypes
import importlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
SHAPES = [(1024, 1024, 16), (480, 640, 1)]
TOP_K = 4000


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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "alike_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    weights = importlib.import_module("deep-image-matching_amd.weights")
    ak = importlib.import_module("deep-image-matching_amd.alike_hip")
    al = importlib.import_module("deep-image-matching_amd.aliked_hip")
    capi = importlib.import_module("deep-image-matching_amd.capi")
    lib = capi.load()
    results = []
    for H, W, B in (SHAPES[1:] if args.quick else SHAPES):
        x = torch.rand(B, H, W, 3, generator=torch.Generator().manual_seed(0)).cuda().contiguous()
        row = {"H": H, "W": W, "batch": B, "top_k": TOP_K, "ms_per_image": {}, "repeats_ms_per_call": {}}
        nets = {m: ak.AlikeHIP(weights.synthetic_alike_state_dict(11, m), {"model": m, "top_k": TOP_K}, max_batch=B, max_hw=(H, W)) for m in weights.ALIKE_CFGS}
        nets["aliked-n16"] = al.AlikedHIP(weights.synthetic_aliked_state_dict(7, "aliked-n16"),
                                          {"model_name": "aliked-n16", "max_num_keypoints": TOP_K, "detection_threshold": -1.0}, max_batch=B, max_hw=(H, W))
        outs = {}
        for name, net in nets.items():      # warm-up: code objects, allocations of the outputs
            outs[name] = net.extract_batch(x)
            for _ in range(2):
                net.extract_batch(x, out=outs[name])
        torch.cuda.synchronize()
        iters = {name: max(3, min(500, int(0.3e3 / max(timed(lambda: net.extract_batch(x, out=outs[name]), 3), 1e-3)))) for name, net in nets.items()}
        ms = {name: [] for name in nets}
        clk = torch.zeros(4, dtype=torch.int64, device="cuda")
        row["sustained_clock_mhz"] = {}
        for rep in range(3):
            for name, net in nets.items():
                # shader-clock probes around the window (dim_op_read_clocks: {shader cycles, 100 MHz ticks}), as bench.py does
                capi.check(lib, lib.dim_op_read_clocks(ctypes.c_void_p(clk.data_ptr()), capi.stream_ptr("cuda")))
                ms[name].append(timed(lambda: net.extract_batch(x, out=outs[name]), iters[name]))
                capi.check(lib, lib.dim_op_read_clocks(ctypes.c_void_p(clk.data_ptr() + 16), capi.stream_ptr("cuda")))
                ck = clk.cpu().tolist()
                row["sustained_clock_mhz"][name] = (ck[2] - ck[0]) / max(1, ck[3] - ck[1]) * 100.0
        total, sites = capi.saturation(lib, None)
        row["range_guard_total"] = total
        for name in nets:
            row["repeats_ms_per_call"][name] = ms[name]
            row["ms_per_image"][name] = min(ms[name]) / B
            row.setdefault("keypoints_per_image", {})[name] = float(outs[name][3].float().mean())
        results.append(row)
        del nets, outs
        torch.cuda.empty_cache()
    doc = {"what": "warm HIP-event extract_batch time per image, best of 3 alternating repeats; synthetic weights, uniform-noise images, top-k mode",
           "device": torch.cuda.get_device_name(0), "shapes": results}
    print("ALIKE_BENCH " + json.dumps(doc), flush=True)
    try:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")
    except OSError:
        pass
    return 0


if __name__ == "__main__":
    sys.exit(main())
