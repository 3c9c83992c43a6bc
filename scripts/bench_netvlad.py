"""Device time of the NetVLAD global descriptor (dim_netvlad_extract) and of its two own kernels.

    python scripts/bench_netvlad.py            # one JSON line at the end, and profiles/netvlad_bench.json
    python scripts/bench_netvlad.py --quick    # a few calls only (the kernel-trace pass: rocprofv3 --kernel-trace --stats -- python ...)

Shape: 1024 x 768 (hloc's resize_max 1024 on a 4:3 photograph), K = 64, whitening 32768 -> 4096, batch 1 and 16.  Times are HIP-event times of
back-to-back calls after a warm-up, best of 3 repeats of a window of at least 0.3 s, reported as milliseconds per IMAGE.  The head and the
whitening are timed through their operator entries on the handle's own conv5_3 map (64 x 48 = 3072 locations) and VLAD vectors; the backbone's
share is the rest of the whole call.  tb_per_s_on_w = the 512 MiB of W over the whitening's time per call (W is read once per call).  Weights are
the seeded synthetic ones (the arithmetic and the launch shapes do not depend on the values); the input is uniform noise in 0..1.
"""
from __future__ import annotations

import argparse
import importlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
H, W = 768, 1024
K, WHITEN = 64, 4096


def timed(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def best(fn, quick):
    for _ in range(2):
        fn()
    iters = 3 if quick else max(3, min(500, int(0.3e3 / max(timed(fn, 3), 1e-3))))
    return min(timed(fn, iters) for _ in range(1 if quick else 3))


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "netvlad_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    weights = importlib.import_module("deep-image-matching_amd.weights")
    nv = importlib.import_module("deep-image-matching_amd.netvlad_hip")
    capi = importlib.import_module("deep-image-matching_amd.capi")
    lib = capi.load()
    sd = weights.synthetic_netvlad_state(31, K, WHITEN)
    ww, wb = sd["whiten.weight"].cuda(), sd["whiten.bias"].cuda()
    sw, sc = sd["netvlad.score_proj.weight"].cuda(), sd["netvlad.centers"].cuda()
    results = []
    for B in (1, 16):
        x = torch.rand(B, H, W, 3, generator=torch.Generator().manual_seed(0)).cuda().contiguous()
        net = nv.NetVLADHIP(sd, {"whiten": True}, max_batch=B, max_hw=(H, W))
        capi.check(lib, lib.dim_saturation_reset(capi.stream_ptr("cuda")))
        out = net.extract_batch(x)
        torch.cuda.synchronize()
        total, _ = capi.saturation(lib, None)
        fmap = net.debug_map().reshape(B, -1, 512).cuda().contiguous()
        vlad = nv.netvlad_head(fmap, sw, sc)
        # the operator entries themselves: operands in kernel layout, workspace and output allocated ONCE, outside the timed calls
        n = fmap.shape[1]
        sdk, ckd = sw.reshape(K, 512).t().contiguous(), sc.t().contiguous()
        hws = torch.empty(max(1, lib.dim_op_netvlad_head_workspace_bytes(B, n, K) // 4), dtype=torch.float32, device="cuda")
        wws = torch.empty(max(1, lib.dim_op_netvlad_whiten_workspace_bytes(B, 512 * K, WHITEN) // 4), dtype=torch.float32, device="cuda")
        hout, wout = torch.empty_like(vlad), torch.empty(B, WHITEN, dtype=torch.float32, device="cuda")
        st = capi.stream_ptr("cuda")
        head = lambda: capi.check(lib, lib.dim_op_netvlad_head_f32(capi.ptr(fmap), B, n, K, capi.ptr(sdk), capi.ptr(ckd), capi.ptr(hws), capi.ptr(hout), st))  # noqa: E731
        whiten = lambda: capi.check(lib, lib.dim_op_netvlad_whiten_f32(capi.ptr(vlad), B, 512 * K, capi.ptr(ww), capi.ptr(wb), WHITEN, capi.ptr(wws), capi.ptr(wout), st))  # noqa: E731
        head(), whiten()
        torch.cuda.synchronize()
        assert torch.equal(hout, vlad) and torch.equal(wout, out)
        t_all = best(lambda: net.extract_batch(x, out=out), args.quick)
        t_head = best(head, args.quick)
        t_wh = best(whiten, args.quick)
        results.append({"H": H, "W": W, "batch": B, "K": K, "whiten_out": WHITEN, "range_guard_total": total, "locations": fmap.shape[1],
                        "ms_per_image": {"total": t_all / B, "head": t_head / B, "whitening": t_wh / B, "backbone": (t_all - t_head - t_wh) / B},
                        "ms_per_call": {"total": t_all, "head": t_head, "whitening": t_wh},
                        "tb_per_s_on_w": WHITEN * 512 * K * 4 / (t_wh * 1e-3) / 1e12})
        del net, out, fmap, vlad
        torch.cuda.empty_cache()
    doc = {"what": "warm HIP-event time per image, best of 3 repeats; synthetic weights, uniform-noise images; head / whitening through their C operator "
                   "entries with operands, workspace and output prepared outside the timed calls, backbone = total - head - whitening",
           "device": torch.cuda.get_device_name(0), "shapes": results}
    print("NETVLAD_BENCH " + json.dumps(doc), flush=True)
    if not args.quick:
        try:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")
        except OSError:
            pass
    return 0


if __name__ == "__main__":
    sys.exit(main())
