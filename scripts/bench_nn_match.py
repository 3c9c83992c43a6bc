"""Device time of the nearest-neighbour matcher (dim_nn_match) against the composition a user of the library could build without it.

    python scripts/bench_nn_match.py            # driver: one child process per step, each under its own `timeout`; stops at the first failure
    python scripts/bench_nn_match.py --step N   # one step (what the driver starts)

Steps = (rows per side, descriptor width, batch): 2048 / 8000 x 256 and 1800 x 128, at batch 1 and 16.  Per step, on planted unit-norm sets:
  (a) fused      dim_nn_match in smnn (norms, tile kernel, merge, finalize), three MFMA terms (fp16x3) — no M x N buffer;
  (a1) fused, fp16-exact table: one MFMA term;
  (b) composed   dim_op_gemm_x6_nt_f32 into an M x N buffer per pair, then torch.topk(sim, 2) along both axes on the GPU (on unit-norm descriptors
                 the two largest similarities are the two nearest neighbours; the ratio tests / compaction of (a) are not even included).
Times are HIP-event times of back-to-back calls after a warm-up (measuring-on-mi355x: device events, >= 0.3 s windows, both variants in the same
process, alternating).  The share of the fp16 MFMA peak is 2 M N D x terms / time over 2.5 PFLOP/s (MI355X dense fp16) for the WHOLE fused call
(norms, merge and finalize included), a lower bound of the tile kernel's own share.  Result: profiles/nn_match_bench.json.
If (a) loses somewhere the JSON says so ("fused_not_slower": false); get the kernel breakdown of that step with
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_nn_match.py --step N
"""
from __future__ import annotations

import argparse
import importlib
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
STEPS = [(2048, 256, 1), (2048, 256, 16), (8000, 256, 1), (8000, 256, 16), (1800, 128, 1), (1800, 128, 16)]
PEAK_F16 = 2.5e15
STEP_TIMEOUT_S = 240


def _planted(n, dim, seed):
    import torch

    g = torch.Generator().manual_seed(seed)
    a = torch.nn.functional.normalize(torch.randn(n, dim, generator=g), dim=1)
    b = a[torch.randperm(n, generator=g)] + torch.rand(n, 1, generator=g) * 0.12 * torch.randn(n, dim, generator=g)
    return a, torch.nn.functional.normalize(b, dim=1)


def run_step(k: int) -> dict:
    import torch

    capi = importlib.import_module("deep-image-matching_amd.capi")
    nn = importlib.import_module("deep-image-matching_amd.nn_hip")
    assert torch.cuda.is_available(), "needs an MI355X"
    n, dim, batch = STEPS[k]
    lib = capi.load()
    tab = torch.zeros(2 * batch, n, dim)
    for p in range(batch):
        tab[2 * p], tab[2 * p + 1] = _planted(n, dim, p)
    tab = tab.cuda()
    tab16 = tab.half().float().contiguous()          # what features.h5 holds
    nt = torch.full((2 * batch,), n, dtype=torch.int32, device="cuda")
    net = nn.NearestNeighborHIP("smnn", 0.95, dim=dim, max_pairs=batch, max_kpts=n)
    out = net.match_batch(None, tab, nt, None, n_pairs=batch)
    sim = torch.empty(batch, n, n, device="cuda")
    stream = lambda: net._stream()      # noqa: E731

    def fused():
        net.match_batch(None, tab, nt, None, n_pairs=batch, out=out, f16_exact=False)

    def fused_one_term():
        net.match_batch(None, tab16, nt, None, n_pairs=batch, out=out, f16_exact=True)

    def composed():
        for p in range(batch):
            capi.check(lib, lib.dim_op_gemm_x6_nt_f32(capi.ptr(tab[2 * p]), dim, capi.ptr(tab[2 * p + 1]), dim, capi.ptr(sim[p]), n, n, n, dim, stream()))
        torch.topk(sim, 2, dim=2)
        torch.topk(sim, 2, dim=1)

    def timed(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters

    variants = {"fused": fused, "fused_f16_exact": fused_one_term, "composed": composed}
    for fn in variants.values():      # warm-up: code objects, torch's topk workspaces
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    iters = {name: max(3, min(2000, int(0.3e3 / max(timed(fn, 3), 1e-3)))) for name, fn in variants.items()}
    ms = {name: [] for name in variants}
    for _ in range(3):                # alternate the variants; keep every repeat
        for name, fn in variants.items():
            ms[name].append(timed(fn, iters[name]))
    total, sites = capi.saturation(lib, None)
    assert total == 0, sites
    best = {name: min(v) for name, v in ms.items()}
    flops = 2.0 * n * n * dim * batch
    res = {"rows": n, "dim": dim, "batch": batch, "iters": iters, "ms_per_call_repeats": ms,
           "fused_ms_per_pair": best["fused"] / batch, "fused_f16_exact_ms_per_pair": best["fused_f16_exact"] / batch,
           "composed_ms_per_pair": best["composed"] / batch, "fused_over_composed": best["fused"] / best["composed"],
           "fused_not_slower": best["fused"] <= best["composed"],
           "fused_share_of_fp16_mfma_peak": 3 * flops / (best["fused"] * 1e-3) / PEAK_F16,
           "fused_f16_exact_share_of_fp16_mfma_peak": flops / (best["fused_f16_exact"] * 1e-3) / PEAK_F16,
           "matches_per_pair": float(out["n_matches"].float().mean()), "fused_workspace_bytes": net.workspace_bytes(),
           "composed_mxn_bytes": int(sim.numel() * 4)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", type=int, default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "nn_match_bench.json"))
    args = ap.parse_args()
    if args.step is not None:
        print("NN_BENCH " + json.dumps(run_step(args.step)), flush=True)
        return 0
    results, failed = [], None
    for k in range(len(STEPS)):
        t0 = time.time()
        r = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, str(Path(__file__).resolve()), "--step", str(k)],
                           capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("NN_BENCH ")]
        if r.returncode != 0 or not line:
            failed = {"step": k, "shape": STEPS[k], "returncode": r.returncode, "stderr_tail": r.stderr[-2000:]}
            print("step", k, STEPS[k], "FAILED", r.returncode, r.stderr[-2000:], flush=True)
            break      # nothing more is started on the GPU after a failure
        results.append(json.loads(line[0][len("NN_BENCH "):]))
        print("step", k, STEPS[k], "%.1f s" % (time.time() - t0), {q: round(v, 4) for q, v in results[-1].items() if isinstance(v, float)}, flush=True)
    doc = {"what": "dim_nn_match (fused, no M x N buffer) vs dim_op_gemm_x6_nt_f32 + torch.topk along both axes; HIP-event ms, best of 3 alternating repeats",
           "peak_fp16_mfma_flops": PEAK_F16, "steps": results, "failed": failed,
           "fused_not_slower_everywhere": failed is None and all(r["fused_not_slower"] for r in results)}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")
    return 0 if failed is None else 1


if __name__ == "__main__":
    sys.exit(main())
