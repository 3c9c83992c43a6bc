"""Device time of the SuperGlue matcher (SuperGlueHIP: 18 layers, Sinkhorn) at 2048 x 2048 keypoints, split by stage, next to a LightGlueHIP
fixed-work pair (9 layers, no early stop, no pruning) from the same run.

    python scripts/bench_superglue.py                # every step as a process of its own, then profiles/superglue_bench.json
    python scripts/bench_superglue.py --step p16     # one step in this process: one JSON line `SG_BENCH_STEP {json}`

Steps: 16 pairs per call and 1 pair per call, each at 20 and at 100 Sinkhorn iterations.  Every step runs under its own `timeout -k 10`; the steps
are chained, so a failure stops the rest.  Times are HIP-event times of back-to-back calls after a warm-up, best of 3 alternating repeats of a
window of at least 0.3 s, reported as milliseconds per PAIR.  The split comes from timing parts of the call through the library's own entry points:
  sinkhorn   dim_sg_sinkhorn alone on the score block the last match left (the two passes x iterations + the zeroing of u, v)
  selection  dim_sg_select alone
  head       a match with the graph network switched off (dim_sg_debug_layers 0) and 0 iterations, minus selection: the keypoint encoder,
             final_proj and the score product
  gnn        a match with 0 iterations minus that same call without the graph network
Sinkhorn's traffic figure is 2 passes x 4 bytes x m x n x iterations over its time.  Weights are the seeded synthetic ones; keypoints are
uniform, descriptors random unit rows (the work does not depend on the values).
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
STEPS = {"p16": 16, "p1": 1}
KPTS = 2048
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


def best_of(run):
    """{name: fn} -> {name: best ms per call}: alternating repeats."""
    import torch
    for fn in run.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    iters = {k: max(3, min(500, int(0.3e3 / max(timed(fn, 2), 1e-3)))) for k, fn in run.items()}
    ms = {k: [] for k in run}
    for _ in range(3):
        for k, fn in run.items():
            ms[k].append(timed(fn, iters[k]))
    return {k: min(v) for k, v in ms.items()}, ms


def step(pairs):
    import torch
    weights = importlib.import_module("deep-image-matching_amd.weights")
    sg = importlib.import_module("deep-image-matching_amd.superglue_hip")
    lg = importlib.import_module("deep-image-matching_amd.lightglue_hip")
    capi = importlib.import_module("deep-image-matching_amd.capi")
    lib = capi.load()
    g = torch.Generator().manual_seed(0)
    kt = (torch.rand(2 * pairs, KPTS, 2, generator=g) * 1024).cuda()
    sc = torch.rand(2 * pairs, KPTS, generator=g).cuda()
    nt = torch.full((2 * pairs,), KPTS, dtype=torch.int32).cuda()
    st = torch.tensor([[1024.0, 1024.0]] * (2 * pairs)).cuda()
    desc = torch.nn.functional.normalize(torch.randn(2 * pairs, KPTS, 256, generator=g), dim=-1).cuda().contiguous()
    net = sg.SuperGlueHIP(weights.synthetic_superglue_state_dict(3, final_gain=12.0), None, max_pairs=pairs, max_kpts=KPTS)
    lgn = lg.LightGlueHIP(weights.synthetic_lightglue_state_dict(0, 256, gain=2.0), {"depth_confidence": -1, "width_confidence": -1}, max_pairs=pairs, max_kpts=KPTS)
    capi.check(lib, lib.dim_saturation_reset(capi.stream_ptr("cuda")))
    out = net.match_batch(kt, desc, sc, nt, st, n_pairs=pairs, sinkhorn_iterations=20, match_threshold=0.2)
    lout = lgn.match_batch(kt, desc, nt, st, n_pairs=pairs)
    s = lambda: capi.stream_ptr("cuda")   # noqa: E731
    p = capi.ptr

    def match(iters, layers=-1):
        def fn():
            capi.check(lib, lib.dim_sg_debug_layers(net._h, layers))
            net.match_batch(kt, desc, sc, nt, st, n_pairs=pairs, sinkhorn_iterations=iters, match_threshold=0.2, out=out)
            capi.check(lib, lib.dim_sg_debug_layers(net._h, -1))
        return fn

    run = {"match_100": match(100), "match_20": match(20), "match_0": match(0), "head_0": match(0, 0),
           "sinkhorn_100": lambda: capi.check(lib, lib.dim_sg_sinkhorn(net._h, pairs, KPTS, 100, s())),
           "sinkhorn_20": lambda: capi.check(lib, lib.dim_sg_sinkhorn(net._h, pairs, KPTS, 20, s())),
           "selection": lambda: capi.check(lib, lib.dim_sg_select(net._h, pairs, KPTS, 0.2, p(out["matches"]), p(out["scores"]), p(out["n_matches"]),
                                                                  p(out["matches01"]), p(out["mscores01"]), s())),
           "lightglue_fixed": lambda: lgn.match_batch(kt, desc, nt, st, n_pairs=pairs, out=lout)}
    best, reps = best_of(run)
    net.match_batch(kt, desc, sc, nt, st, n_pairs=pairs, sinkhorn_iterations=20, match_threshold=0.2, out=out)
    total, _ = capi.saturation(lib, None)
    per = {k: v / pairs for k, v in best.items()}
    rows = []
    for iters in (20, 100):
        sink = per[f"sinkhorn_{iters}"]
        traffic = 2 * 4 * KPTS * KPTS * iters * pairs
        rows.append({"pairs": pairs, "kpts": KPTS, "sinkhorn_iterations": iters, "ms_per_pair": per[f"match_{iters}"],
                     "split_ms_per_pair": {"head (encoder, final_proj, scores)": per["head_0"] - per["selection"], "gnn": per["match_0"] - per["head_0"],
                                           "sinkhorn": sink, "selection": per["selection"]},
                     "sinkhorn_us_per_pass": 1e3 * best[f"sinkhorn_{iters}"] / (2 * iters),
                     "sinkhorn_bytes": traffic, "sinkhorn_TB_per_s": traffic / (best[f"sinkhorn_{iters}"] * 1e-3) / 1e12,
                     "lightglue_fixed_ms_per_pair": per["lightglue_fixed"], "range_guard_total": total,
                     "matches_per_pair": float(out["n_matches"].float().mean()), "repeats_ms_per_call": reps})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=list(STEPS))
    ap.add_argument("--out", default=str(ROOT / "profiles" / "superglue_bench.json"))
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), "needs an MI355X"
        print("SG_BENCH_STEP " + json.dumps({"device": torch.cuda.get_device_name(0), "rows": step(STEPS[args.step])}), flush=True)
        return 0
    rows, device = [], None
    for name in STEPS:   # one process per step, each under its own time limit; the first failure ends the run
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, str(Path(__file__).resolve()), "--step", name]
        r = subprocess.run(cmd, capture_output=True, text=True)
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith("SG_BENCH_STEP ")), None)
        if r.returncode != 0 or line is None:
            print(f"step {name} failed with exit status {r.returncode}: stopping\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", flush=True)
            return r.returncode or 1
        part = json.loads(line[len("SG_BENCH_STEP "):])
        device = part["device"]
        rows += part["rows"]
        print(f"step {name} done", flush=True)
    doc = {"what": "warm HIP-event time per pair at 2048 x 2048 keypoints, best of 3 alternating repeats; synthetic weights, uniform keypoints, random unit "
                   "descriptors; the split times parts of the call through dim_sg_sinkhorn / dim_sg_select / dim_sg_debug_layers", "device": device, "rows": rows}
    print("SG_BENCH " + json.dumps(doc), flush=True)
    try:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")
    except OSError:
        pass
    return 0


if __name__ == "__main__":
    sys.exit(main())
