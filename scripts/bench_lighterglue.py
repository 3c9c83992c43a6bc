"""Device time of the LighterGlue matcher (LighterGlueHIP: width 96, one head, 6 layers) next to LightGlueHIP (width 256, four heads, 9 layers) at the
same keypoint counts in the same run, and of the chain XFeatHIP -> LighterGlueHIP.

    python scripts/bench_lighterglue.py                  # every step as a process of its own, then profiles/lighterglue_bench.json
    python scripts/bench_lighterglue.py --step p16_k2048 # one step in this process: one JSON line `LGL_BENCH_STEP {json}`
    python scripts/bench_lighterglue.py --quick ...      # a few calls per network only (the kernel-trace pass)

Steps: 1 pair and 16 pairs per call at 2048 x 2048 and 4096 x 4096 keypoints, each in two modes — fixed work (no early stop, no pruning: depth and
width confidence -1) and each network's default (LighterGlue -1 / 0.95, LightGlue 0.95 / 0.99) — and the chain on two 1024 x 1024 images with 4096
keypoints each.  Every step runs under its own `timeout -k 10`; the steps are chained, so a failure stops the rest.  Times are HIP-event times of
back-to-back match_batch calls after a warm-up, best of 3 alternating repeats of a window of at least 0.3 s, reported as milliseconds per PAIR.
Weights are the seeded synthetic ones (fixed work does not depend on the values; the default modes' early stops and pruning do, and are reported
with the stop layers they produced); keypoints are uniform, descriptors random unit rows.
"""
from __future__ import annotations

import argparse
import importlib
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
STEPS = {"p1_k2048": (1, 2048), "p16_k2048": (16, 2048), "p1_k4096": (1, 4096), "p16_k4096": (16, 4096), "chain": None}
STEP_LIMIT_S = 240


def timed(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def best_of(run, quick):
    """{name: fn} -> {name: [ms per call, ...]}: alternating repeats."""
    import torch
    for fn in run.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    iters = {k: 3 if quick else max(3, min(500, int(0.3e3 / max(timed(fn, 3), 1e-3)))) for k, fn in run.items()}
    ms = {k: [] for k in run}
    for _ in range(1 if quick else 3):
        for k, fn in run.items():
            ms[k].append(timed(fn, iters[k]))
    return ms


def match_step(pairs, kpts, quick):
    import torch
    weights = importlib.import_module("deep-image-matching_amd.weights")
    lgl = importlib.import_module("deep-image-matching_amd.lighterglue_hip")
    lg = importlib.import_module("deep-image-matching_amd.lightglue_hip")
    capi = importlib.import_module("deep-image-matching_amd.capi")
    lib = capi.load()
    g = torch.Generator().manual_seed(0)
    kt = (torch.rand(2 * pairs, kpts, 2, generator=g) * 1024).cuda()
    nt = torch.full((2 * pairs,), kpts, dtype=torch.int32).cuda()
    st = torch.tensor([[1024.0, 1024.0]] * (2 * pairs)).cuda()
    desc = {D: torch.nn.functional.normalize(torch.randn(2 * pairs, kpts, D, generator=g), dim=-1).cuda().contiguous() for D in (64, 256)}
    sds = {"lighterglue": weights.synthetic_lighterglue_state_dict(3), "lightglue": weights.synthetic_lightglue_state_dict(0, 256, gain=2.0)}
    rows = []
    for mode in ("fixed", "default"):
        conf = {"depth_confidence": -1, "width_confidence": -1} if mode == "fixed" else {}
        nets = {"lighterglue": lgl.LighterGlueHIP(sds["lighterglue"], conf, max_pairs=pairs, max_kpts=kpts),
                "lightglue": lg.LightGlueHIP(sds["lightglue"], conf, max_pairs=pairs, max_kpts=kpts)}
        capi.check(lib, lib.dim_saturation_reset(capi.stream_ptr("cuda")))
        outs = {k: net.match_batch(kt, desc[net.input_dim], nt, st, n_pairs=pairs) for k, net in nets.items()}
        run = {k: (lambda net=net, k=k: net.match_batch(kt, desc[net.input_dim], nt, st, n_pairs=pairs, out=outs[k])) for k, net in nets.items()}
        ms = best_of(run, quick)
        total, _ = capi.saturation(lib, None)
        per_pair = {k: min(v) / pairs for k, v in ms.items()}
        rows.append({"pairs": pairs, "kpts": kpts, "mode": mode, "range_guard_total": total, "repeats_ms_per_call": ms, "ms_per_pair": per_pair,
                     "lighterglue_over_lightglue": per_pair["lighterglue"] / per_pair["lightglue"],
                     "stop_layers": {k: sorted(set(outs[k]["stop"].cpu().tolist())) for k in nets},
                     "matches_per_pair": {k: float(outs[k]["n_matches"].float().mean()) for k in nets}})
        del nets, outs, run
        torch.cuda.empty_cache()
    return rows


def chain_step(quick):
    import torch
    weights = importlib.import_module("deep-image-matching_amd.weights")
    lgl = importlib.import_module("deep-image-matching_amd.lighterglue_hip")
    xf = importlib.import_module("deep-image-matching_amd.xfeat_hip")
    H = W = 1024
    x = (torch.rand(2, H, W, 3, generator=torch.Generator().manual_seed(0)) * 255.0).cuda().contiguous()
    ex = xf.XFeatHIP(weights.synthetic_xfeat_state_dict(21), {"top_k": 4096}, max_batch=2, max_hw=(H, W))
    net = lgl.LighterGlueHIP(weights.synthetic_lighterglue_state_dict(3), None, max_pairs=1, max_kpts=4096)
    st = torch.tensor([[float(W), float(H)]] * 2).cuda()
    feats = ex.extract_batch(x)
    d64 = torch.zeros(2, 4096, 64, device="cuda")
    out = net.match_batch(feats[0][:, :4096].contiguous(), d64, feats[3], st, n_pairs=1)

    def both():
        kp, sc, de, n = ex.extract_batch(x, out=feats)
        d64.copy_(de[:, :4096, :64])
        net.match_batch(kp[:, :4096], d64, n, st, n_pairs=1, out=out)

    ms = best_of({"xfeat+lighterglue": both, "xfeat": lambda: ex.extract_batch(x, out=feats)}, quick)
    return [{"chain": "2 images 1024 x 1024 -> XFeatHIP (top_k 4096, batch 2) -> LighterGlueHIP (1 pair)", "keypoints": feats[3].cpu().tolist(),
             "repeats_ms_per_call": ms, "ms_per_pair": {k: min(v) for k, v in ms.items()}}]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=list(STEPS))
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "lighterglue_bench.json"))
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), "needs an MI355X"
        rows = chain_step(args.quick) if args.step == "chain" else match_step(*STEPS[args.step], args.quick)
        print("LGL_BENCH_STEP " + json.dumps({"device": torch.cuda.get_device_name(0), "rows": rows}), flush=True)
        return 0
    rows, device = [], None
    for step in STEPS:   # one process per step, each under its own time limit; the first failure ends the run
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, str(Path(__file__).resolve()), "--step", step] + (["--quick"] if args.quick else [])
        r = subprocess.run(cmd, capture_output=True, text=True)
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith("LGL_BENCH_STEP ")), None)
        if r.returncode != 0 or line is None:
            print(f"step {step} failed with exit status {r.returncode}: stopping\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", flush=True)
            return r.returncode or 1
        part = json.loads(line[len("LGL_BENCH_STEP "):])
        device = part["device"]
        rows += part["rows"]
        print(f"step {step} done", flush=True)
    doc = {"what": "warm HIP-event match_batch time per pair, best of 3 alternating repeats; synthetic weights, uniform keypoints, random unit descriptors",
           "device": device, "rows": rows}
    print("LGL_BENCH " + json.dumps(doc), flush=True)
    if not args.quick:
        try:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")
        except OSError:
            pass
    return 0


if __name__ == "__main__":
    sys.exit(main())
