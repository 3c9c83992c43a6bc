"""Regenerates tests/golden/sg_<case>.npz for the SuperGlue matcher.  Needs the reference tree (environment variable DIM_REFERENCE_ROOT = its
checkout) and runs on the CPU only; nothing of the reference's program text is copied: its network file is imported by path.

superglue_{indoor,outdoor}.pth are not in the reference tree, so the module is built with torch.load patched to hand it the case's seeded synthetic
state dict (weights.synthetic_superglue_state_dict) where it would read the checkpoint.

Per case the script asserts: (a) tests/superglue_ref.py == the module on every integer output, matching scores within 1e-5; (b) the fp32 and fp64
evaluations of the oracle make identical decisions; (c) every decision margin in fp64 is at least 10 x TIE_TOL = 1e-3 — the top-2 gaps of the row
and of the column of every match, the distance of every mutual pair's score from the threshold (superglue_cases.decision_margin); (d) the case's
structural property.  A case that fails gets another seed in tests/superglue_cases.py, not a looser bound.  The GPU-only 1100 x 900 case is checked
for (b) and (c) as well (it has no module golden).

    python scripts/make_superglue_golden.py
"""
from __future__ import annotations

import importlib.util
import os
import sys
from pathlib import Path
from unittest import mock

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
SGN = Path(os.environ["DIM_REFERENCE_ROOT"]) / "src/deep_image_matching/thirdparty/SuperGluePretrainedNetwork/models/superglue.py"

from tests import superglue_cases as sc  # noqa: E402


def reference_module(sd, conf):
    spec = importlib.util.spec_from_file_location("ref_sgn", str(SGN))
    sgn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sgn)
    assert sgn.SuperGlue.default_config["sinkhorn_iterations"] == sc.NET["sinkhorn_iterations"]
    assert sgn.SuperGlue.default_config["match_threshold"] == sc.NET["match_threshold"]
    assert sgn.SuperGlue.default_config["GNN_layers"] == ["self", "cross"] * 9 and sgn.SuperGlue.default_config["keypoint_encoder"] == [32, 64, 128, 256]
    with mock.patch.object(torch, "load", lambda *a, **k: sd), mock.patch("builtins.print", lambda *a, **k: None):
        net = sgn.SuperGlue({"weights": "outdoor", **conf}).eval()   # keys omitted from conf: the network's own defaults (the wrapper quirk)
    return net


def module_data(f0, f1):
    img = lambda f: torch.empty(1, 1, int(f["size"][0]), int(f["size"][1]))   # noqa: E731  (the wrapper: np.empty((1, 1, *image_size)))
    d = sc.data_of(f0, f1)
    d["image0"], d["image1"] = img(f0), img(f1)
    return d


def check_bc(name, case, sd, f0, f1):
    conf = sc.conf_of(case)
    ref32, ref64 = sc.oracle(f0, f1, sd, conf), sc.oracle(f0, f1, sd, conf, torch.float64)
    for k in ("matches0", "matches1", "matches"):                                                    # (b)
        assert torch.equal(ref32[k], ref64[k]), (name, k, "fp32 and fp64 decide differently")
    worst = sc.decision_margin(ref64, conf["match_threshold"])                                       # (c)
    assert worst >= sc.MIN_MARGIN, (name, "decision margin", worst)
    return ref32, ref64, worst


@torch.no_grad()
def main():
    for name, case in sc.GOLDEN_CASES.items():
        sd, (f0, f1), conf = sc.case_weights(case), sc.case_inputs(case), sc.conf_of(case)
        net = reference_module(sd, case["conf"])
        assert net.config["sinkhorn_iterations"] == conf["sinkhorn_iterations"] and net.config["match_threshold"] == conf["match_threshold"]
        got = {k: v[0] for k, v in net(module_data(f0, f1)).items()}
        ref32, ref64, worst = check_bc(name, case, sd, f0, f1)
        for k in ("matches0", "matches1"):                                                           # (a)
            assert torch.equal(ref32[k], got[k].long()), (name, k, "oracle != module")
        for k in ("matching_scores0", "matching_scores1"):
            assert float((ref32[k] - got[k]).abs().max()) <= 1e-5, (name, k)
        m, n = case["m"], case["n"]
        m0 = got["matches0"].long()
        matches = torch.stack([torch.arange(m)[m0 > -1], m0[m0 > -1]], dim=1)
        S, mutual = int(matches.shape[0]), int((ref64["matching_scores0"] > 0).sum())
        res = sc.residuals(ref32, ref64)
        if name == "zoo":                                                                            # (d)
            assert (m, n) == (70, 130) and conf == {"sinkhorn_iterations": 100, "match_threshold": 0.3} and S >= 10 and mutual - S >= 3, (S, mutual)
        if name == "yaml":
            assert m % 32 and n % 32 and conf == {"sinkhorn_iterations": 20, "match_threshold": 0.3} and S >= 10
        if name == "odd":
            assert (m, n) == (33, 97) and case["conf"] == {} and conf == {"sinkhorn_iterations": 100, "match_threshold": 0.2} and S >= 10
            strict = sc.oracle(f0, f1, sd, {**conf, "match_threshold": 0.3}, torch.float64)
            assert strict["matches"].shape[0] < S, "a threshold of 0.3 must be told apart from the network's 0.2"
        if name == "wide":
            assert m > 256 and 9 <= (n + 31) // 32 <= 10 and 9 <= (m + 31) // 32 <= 10 and S >= 10
        if name == "dustbin":
            junk = int(round(case["junk"] * n))
            assert junk >= 0.4 * n and int((m0 == -1).sum()) >= 0.25 * m and int((got["matches1"] == -1).sum()) >= 0.25 * n
            # the dustbin column of exp(Z): what every row of image 0 sends there (rows of exp(Z) sum to 1 once the iteration has converged)
            dust = (sd["bin_score"].double() + ref64["u"][:m] + ref64["v"][n] - ref64["norm"]).exp()
            assert float(dust.sum()) >= 0.2 * m, float(dust.sum())
        np.savez_compressed(ROOT / "tests" / "golden" / f"sg_{name}.npz", matches0=got["matches0"].long().numpy(), matches1=got["matches1"].long().numpy(),
                            matching_scores0=got["matching_scores0"].numpy(), matching_scores1=got["matching_scores1"].numpy(),
                            matches=matches.numpy(), min_margin=np.float64(worst), **{k: np.float64(v) for k, v in res.items()})
        print(f"{name}: {m} x {n} -> {S} matches of {mutual} mutual pairs, smallest fp64 margin {worst:.4f}, fp32 - fp64: scores {res['score_res64']:.2e}, "
              f"u / v {res['uv_res64']:.2e}, descriptors {res['desc_res64']:.2e}, encoder {res['enc_res64']:.2e}; oracle == module")
    case = sc.BIG_CASE
    _, ref64, worst = check_bc("big", case, sc.case_weights(case), *sc.case_inputs(case))
    print(f"big: {case['m']} x {case['n']} -> {ref64['matches'].shape[0]} matches, smallest fp64 margin {worst:.4f} (GPU test, no module golden)")


if __name__ == "__main__":
    main()
