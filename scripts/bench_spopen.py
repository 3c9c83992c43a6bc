"""Device time of the open SuperPoint extractor (dim_spo_create: BatchNorm in the convolution epilogue) next to SuperPoint (dim_sp_create) at
the same shape, configuration and run.

    python scripts/bench_spopen.py

Shape: 1024 x 1024 with batch 16, the pipeline's configuration (nms 5, threshold 0.005, 4096 keypoints).  Times are HIP-event times of back-to-back
extract_batch calls after a warm-up, best of 3 ALTERNATING repeats of a window of at least 0.3 s (device events, warm, both handles in one
process), reported as milliseconds per call and per image with the shader clock each last window held.  Weights are the seeded synthetic ones
of both networks (the launch shapes do not depend on the values); the input is uniform noise.  The two networks differ by one fma per output
and, on the pooled layers, three v_min and a select, against 27 x Cin matrix-core terms: the ratio is expected near 1.
Result: one line `SPOPEN_BENCH {json}` and profiles/spopen_bench.json.
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
H, W, B = 1024, 1024, 16
CFG = {"nms_radius": 5, "keypoint_threshold": 0.005, "max_keypoints": 4096, "remove_borders": 4}


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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "spopen_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    weights = importlib.import_module("deep-image-matching_amd.weights")
    sp = importlib.import_module("deep-image-matching_amd.superpoint_hip")
    capi = importlib.import_module("deep-image-matching_amd.capi")
    lib = capi.load()
    x = torch.rand(B, H, W, generator=torch.Generator().manual_seed(0)).cuda().contiguous()
    nets = {"superpoint": sp.SuperPointHIP(weights.synthetic_superpoint_state_dict(1234), {**CFG, "fix_sampling": True}, max_batch=B, max_hw=(H, W)),
            "superpoint_open": sp.SuperPointOpenHIP(weights.synthetic_superpoint_open_state_dict(4321), CFG, max_batch=B, max_hw=(H, W))}
    outs = {}
    capi.check(lib, lib.dim_saturation_reset(capi.stream_ptr("cuda")))
    for name, net in nets.items():      # warm-up: code objects, allocations of the outputs
        outs[name] = net.extract_batch(x)
        for _ in range(2):
            net.extract_batch(x, out=outs[name])
    torch.cuda.synchronize()
    iters = {name: max(3, min(500, int(0.3e3 / max(timed(lambda: net.extract_batch(x, out=outs[name]), 3), 1e-3)))) for name, net in nets.items()}
    ms = {name: [] for name in nets}
    clk = torch.zeros(4, dtype=torch.int64, device="cuda")
    clocks = {}
    for rep in range(3):
        for name, net in nets.items():
            # shader-clock probes around the window (dim_op_read_clocks: {shader cycles, 100 MHz ticks}), as bench.py does
            capi.check(lib, lib.dim_op_read_clocks(ctypes.c_void_p(clk.data_ptr()), capi.stream_ptr("cuda")))
            ms[name].append(timed(lambda: net.extract_batch(x, out=outs[name]), iters[name]))
            capi.check(lib, lib.dim_op_read_clocks(ctypes.c_void_p(clk.data_ptr() + 16), capi.stream_ptr("cuda")))
            ck = clk.cpu().tolist()
            clocks[name] = (ck[2] - ck[0]) / max(1, ck[3] - ck[1]) * 100.0
    total, sites = capi.saturation(lib, None)
    best = {name: min(v) for name, v in ms.items()}
    doc = {"what": "warm HIP-event extract_batch time, best of 3 alternating repeats; synthetic weights, uniform-noise images",
           "device": torch.cuda.get_device_name(0), "H": H, "W": W, "batch": B, "config": CFG, "iterations_per_window": iters,
           "repeats_ms_per_call": ms, "ms_per_call": best, "ms_per_image": {k: v / B for k, v in best.items()},
           "ratio_open_over_superpoint": best["superpoint_open"] / best["superpoint"], "sustained_clock_mhz": clocks,
           "keypoints_per_image": {name: float(outs[name][3].float().mean()) for name in nets}, "range_guard_total": total, "range_guard_sites": sites}
    print("SPOPEN_BENCH " + json.dumps(doc), flush=True)
    try:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")
    except OSError:
        pass
    return 0


if __name__ == "__main__":
    sys.exit(main())
