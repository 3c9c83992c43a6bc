"""Device time of the RIPE extractor (dim_ripe_extract), split into its spans, and of the depthwise 5 x 5 kernel at scale 1.

    python scripts/bench_ripe.py            # one JSON line at the end, and profiles/ripe_bench.json
    python scripts/bench_ripe.py --quick    # a few calls only

Shape: 1024 x 1024, top_k 4096, threshold 0.5, batch 1 and 4.  Times are HIP-event times of back-to-back calls after a warm-up; the whole call is the
median of 5 repeats of a window of at least 0.3 s, reported as milliseconds per IMAGE.  The spans (encoder, the decoder's four scales, detection,
descriptors) are the library's own event pairs around them (dim_profile_start / dim_profile_stop, one span armed at a time), the median over the
calls of a window.  The depthwise kernel is timed through its operator entry on a 64-channel 1024 x 1024 map; its algorithmic traffic is one read
and one write of that map.  Weights are the seeded synthetic ones (the dense part's arithmetic and launch shapes do not depend on the values); the
input is uniform noise in 0..1, on which those weights find fewer keypoints than top_k (the count is recorded): the detection and descriptor spans
are those of that count.
"""
from __future__ import annotations

import argparse
import ctypes
import importlib
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
H, W = 1024, 1024
TOP_K = 4096
SPANS = ["encoder", "decoder_scale8", "decoder_scale4", "decoder_scale2", "decoder_scale1", "detection", "descriptors"]
PROF_FIRST = 18   # DIM_PROF_RIPE_ENCODER (include/dim_hip.h)


def timed(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def median_ms(fn, quick):
    for _ in range(2):
        fn()
    iters = 2 if quick else max(3, min(500, int(0.3e3 / max(timed(fn, 2), 1e-3))))
    return statistics.median(timed(fn, iters) for _ in range(1 if quick else 5))


def span_ms(lib, fn, site, calls):
    import torch
    torch.cuda.synchronize()
    lib.dim_profile_start(ctypes.c_ulonglong(1 << site))
    for _ in range(calls):
        fn()
    tot, n = ctypes.c_double(), ctypes.c_int()
    lib.dim_profile_stop(ctypes.byref(tot), ctypes.byref(n))
    assert n.value == calls, (n.value, calls)
    return tot.value / calls


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ripe_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    weights = importlib.import_module("deep-image-matching_amd.weights")
    rp = importlib.import_module("deep-image-matching_amd.ripe_hip")
    capi = importlib.import_module("deep-image-matching_amd.capi")
    lib = capi.load()
    rp.declare(lib)
    sd = weights.synthetic_ripe_state_dict()
    results = []
    for B in (1, 4):
        x = torch.rand(B, H, W, 3, generator=torch.Generator().manual_seed(0)).cuda().contiguous()
        net = rp.RipeHIP(sd, {"top_k": TOP_K, "threshold": 0.5}, max_batch=B, max_hw=(H, W))
        capi.check(lib, lib.dim_saturation_reset(capi.stream_ptr("cuda")))
        out = net.extract_batch(x)
        torch.cuda.synchronize()
        total, _ = capi.saturation(lib, None)
        call = lambda: net.extract_batch(x, out=out)  # noqa: E731
        t_all = median_ms(call, args.quick)
        calls = 2 if args.quick else 5
        spans = {name: statistics.median(span_ms(lib, call, PROF_FIRST + i, calls) for _ in range(1 if args.quick else 3)) / B for i, name in enumerate(SPANS)}
        results.append({"H": H, "W": W, "batch": B, "top_k": TOP_K, "keypoints": [int(v) for v in out[3].tolist()], "range_guard_total": total,
                        "ms_per_image": {"total": t_all / B, **spans, "sum_of_spans": sum(spans.values())}, "ms_per_call": t_all})
        del net, out
        torch.cuda.empty_cache()
    # the depthwise kernel at scale 1: one read and one write of the 64-channel map
    C = 64
    m = torch.rand(1, H, W, C, device="cuda")
    wk, bk, o = torch.randn(25, C, device="cuda") * 0.2, torch.randn(C, device="cuda") * 0.1, torch.empty(1, H, W, C, device="cuda")
    st = capi.stream_ptr("cuda")
    dw = lambda: capi.check(lib, lib.dim_op_ripe_dw5x5_f32(capi.ptr(m), capi.ptr(wk), capi.ptr(bk), capi.ptr(o), 1, H, W, C, st))  # noqa: E731
    t_dw = median_ms(dw, args.quick)
    algo = 2 * H * W * C * 4
    doc = {"what": "warm HIP-event time, median of 5 repeats; synthetic weights, uniform-noise images; spans from the library's own event pairs, one armed at a time",
           "device": torch.cuda.get_device_name(0), "shapes": results,
           "depthwise_scale1": {"H": H, "W": W, "C": C, "ms": t_dw, "algorithmic_bytes": algo, "tb_per_s": algo / (t_dw * 1e-3) / 1e12},
           "fused_depthwise_pointwise": "not measured (the unfused pair is what the library runs)"}
    print("RIPE_BENCH " + json.dumps(doc), flush=True)
    if not args.quick:
        try:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")
        except OSError:
            pass
    return 0


if __name__ == "__main__":
    sys.exit(main())
