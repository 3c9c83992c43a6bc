"""Device time of the geometric verification (dim_gv_fundamental): the streaming kernels for match tables wider than 4096 rows against
the LDS-resident kernels, and the two chunk layouts of the streaming phase A against each other.

    python scripts/bench_gv.py            # driver: one child process per step, each under its own `timeout`; stops at the first failure
    python scripts/bench_gv.py --step N   # one step (what the driver starts)

Steps (2048 hypotheses, Sampson error, threshold 2 px, synthetic two-view scenes with 60 % inliers):
  0  16 pairs x 4096 matches:  (lds)     an NK = 4096 table: the kernels that hold a pair's points in LDS;
                               (stream1) the SAME pairs in an NK = 4097 table: packed points, one staging buffer of 4096 points (DIM_GV_STREAM_LAYOUT=single);
                               (stream2) the same, two staging buffers of 2048 points (DIM_GV_STREAM_LAYOUT=double);
  1  16 pairs x 8192 matches:  (stream1), (stream2) in an NK = 8192 table;
  2  64 pairs x 4096 matches:  as step 0 with 512 workgroups in phase A — two per CU, where the 64 KB of staging and the registers decide.
Times are HIP-event times of back-to-back calls after a warm-up (device events, >= 0.3 s windows, the variants of a step in the same
process, alternating, best of 3).  Every variant's masks are compared with the first one's: the layouts must agree bit for bit.
Result: profiles/gv_bench.json; with --measured FILE one row per step is also appended to that JSON-lines file (the measurement log the
GPU tests append their figures to).
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
ITERS = 2048
STEPS = [(16, 4096, [("lds", 4096, None), ("stream1", 4097, "single"), ("stream2", 4097, "double")]),
         (16, 8192, [("stream1", 8192, "single"), ("stream2", 8192, "double")]),
         (64, 4096, [("lds", 4096, None), ("stream1", 4097, "single"), ("stream2", 4097, "double")])]
STEP_TIMEOUT_S = 240


def run_step(k: int) -> dict:
    import torch

    from oracle import geom_ref
    verify = importlib.import_module("deep-image-matching_amd.verify")
    assert torch.cuda.is_available(), "needs an MI355X"
    PAIRS, S, variants = STEPS[k]
    kt = torch.zeros(2 * PAIRS, S, 2)
    for p in range(PAIRS):
        ni = int(0.6 * S)
        x0, x1, _, _ = geom_ref.synthetic_two_view(ni, S - ni, seed=100 + p, noise_px=0.4)
        kt[2 * p], kt[2 * p + 1] = torch.from_numpy(x0), torch.from_numpy(x1)
    kt = kt.cuda()
    n = torch.full((PAIRS,), S, dtype=torch.int32, device="cuda")
    v = verify.DeviceVerifier(threshold=2.0, iters=ITERS, seed=3)
    tabs, outs = {}, {}
    for name, nk, _ in variants:
        mt = torch.zeros(PAIRS, nk, 2, dtype=torch.int64)
        mt[:, :S, 0] = mt[:, :S, 1] = torch.arange(S)
        tabs[name] = mt.cuda()

    def call(name, nk, layout):
        if layout is not None:
            os.environ["DIM_GV_STREAM_LAYOUT"] = layout      # read by the library at every call
        outs[name] = v.verify_batch(kt, tabs[name], n, out=outs.get(name))

    def timed(args, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            call(*args)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters

    for args in variants:
        for _ in range(2):
            call(*args)
    torch.cuda.synchronize()
    first = variants[0][0]
    same = {name: bool(torch.equal(outs[name]["mask"][:, :S], outs[first]["mask"][:, :S]) and torch.equal(outs[name]["n_inliers"], outs[first]["n_inliers"]))
            for name, _, _ in variants}
    iters = {a[0]: max(3, min(500, int(0.3e3 / max(timed(a, 2), 1e-3)))) for a in variants}
    ms = {a[0]: [] for a in variants}
    for _ in range(3):
        for a in variants:
            ms[a[0]].append(timed(a, iters[a[0]]))
    best = {name: min(t) for name, t in ms.items()}
    res = {"test": "verification", "pairs": PAIRS, "matches": S, "hypotheses": ITERS, "iters": iters, "ms_per_batch_repeats": ms,
           "ms_per_batch": best, "same_masks_as_" + first: same, "mean_inliers": float(outs[first]["n_inliers"].float().mean())}
    if "lds" in best:
        res["stream1_over_lds"] = best["stream1"] / best["lds"]
        res["stream2_over_lds"] = best["stream2"] / best["lds"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", type=int, default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "gv_bench.json"))
    ap.add_argument("--measured", default=None, help="JSON-lines measurement log to append one row per step to")
    args = ap.parse_args()
    if args.step is not None:
        print("GV_BENCH " + json.dumps(run_step(args.step)), flush=True)
        return 0
    results, failed = [], None
    for k in range(len(STEPS)):
        t0 = time.time()
        r = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, str(Path(__file__).resolve()), "--step", str(k)],
                           capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("GV_BENCH ")]
        if r.returncode != 0 or not line:
            failed = {"step": k, "returncode": r.returncode, "stderr_tail": r.stderr[-2000:]}
            print("step", k, "FAILED", r.returncode, r.stderr[-2000:], flush=True)
            break      # nothing more is started on the GPU after a failure
        results.append(json.loads(line[0][len("GV_BENCH "):]))
        print("step", k, "%.1f s" % (time.time() - t0), json.dumps(results[-1]["ms_per_batch"]), flush=True)
    doc = {"what": "dim_gv_fundamental, 2048 hypotheses: LDS-resident kernels vs the streaming kernels (one staging buffer of 4096 points / two of "
                   "2048); HIP-event ms per batch, best of 3 alternating repeats", "steps": results, "failed": failed}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")
    if args.measured:
        Path(args.measured).parent.mkdir(parents=True, exist_ok=True)
        with open(args.measured, "a") as f:
            for r in results:
                f.write(json.dumps(r) + "\n")
    return 0 if failed is None else 1


if __name__ == "__main__":
    sys.exit(main())
