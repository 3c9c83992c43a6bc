"""Regenerates tests/golden/lgl_<case>.npz for the LighterGlue matcher.  Needs the reference tree (environment variable DIM_REFERENCE_ROOT = its
checkout) and runs on the CPU only; nothing of the reference's program text is copied: its files are read or imported by path.

The reference's LighterGlue (thirdparty/accelerated_features/modules/lighterglue.py) wraps kornia's LightGlue, and kornia is not installed here, so
that file cannot be imported.  kornia's class is a copy of the vendored thirdparty/LightGlue/lightglue/lightglue.py, which is what stands in:
built at the configuration that `default_conf_xfeat` sets — read out of the reference file with ast.literal_eval, and asserted equal to the constants
of this port — with the case's seeded synthetic state dict loaded (the trained xfeat-lighterglue.pt is not in the reference tree).

Per case the script asserts: (a) oracle/lightglue_ref.py == the module on every integer output, scores within 1e-5; (b) the fp32 and fp64 evaluations
of the oracle make identical decisions; (c) every decision margin in fp64 is at least 10 x tie_tol = 1e-3 — the top-2 row and column margins of every
reported match, the distance of its score from filter_threshold, and the distance of every matchability from the 0.05 pruning bar at every layer;
(d) the case's structural property.  A case that fails (b)-(d) gets another seed in tests/lighterglue_cases.py, not a looser bound.

    python scripts/make_lighterglue_golden.py
"""
from __future__ import annotations

import ast
import importlib
import importlib.util
import os
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
REF = Path(os.environ["DIM_REFERENCE_ROOT"]) / "src/deep_image_matching/thirdparty"   # the reference checkout

from tests import lighterglue_cases as lc  # noqa: E402
from tests.parity import compare_lightglue  # noqa: E402


def reference_conf() -> dict:
    tree = ast.parse((REF / "accelerated_features/modules/lighterglue.py").read_text())
    for cls in tree.body:
        if isinstance(cls, ast.ClassDef) and cls.name == "LighterGlue":
            for st in cls.body:
                if isinstance(st, ast.Assign) and st.targets[0].id == "default_conf_xfeat":
                    return ast.literal_eval(st.value)
    raise RuntimeError("default_conf_xfeat not found")


def check_constants(rc: dict):
    weights = importlib.import_module("deep-image-matching_amd.weights")
    plugins = importlib.import_module("deep-image-matching_amd.plugins")
    hip = lc.lgl_mod.LighterGlueHIP.default_conf
    for k in ("n_layers", "depth_confidence", "width_confidence", "filter_threshold"):
        assert hip[k] == rc[k] and lc.NET[k] == rc[k], (k, hip[k], rc[k])
    for k in ("n_layers", "depth_confidence", "width_confidence"):
        assert plugins.LighterGlueMatcher._network_conf[k] == rc[k], k
    for k in ("input_dim", "descriptor_dim", "num_heads", "n_layers"):
        assert weights.LIGHTERGLUE_SHAPE[k] == rc[k], k
    assert lc.NET["num_heads"] == rc["num_heads"] and rc["add_scale_ori"] is False and rc["add_laf"] is False


def reference_module(sd, rc, conf):
    spec = importlib.util.spec_from_file_location("ref_lgn", str(REF / "LightGlue/lightglue/lightglue.py"))
    lgn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lgn)
    net = lgn.LightGlue(features=None, input_dim=rc["input_dim"], descriptor_dim=rc["descriptor_dim"], n_layers=rc["n_layers"], num_heads=rc["num_heads"],
                        depth_confidence=conf["depth_confidence"], width_confidence=conf["width_confidence"], filter_threshold=conf["filter_threshold"]).eval()
    missing, unexpected = net.load_state_dict(sd, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    return net


def margins64(ref64, sd, conf):
    """The smallest decision margin of the fp64 evaluation (assertion (c))."""
    worst = float("inf")
    if "log_assignment" in ref64:
        la = ref64["log_assignment"][:-1, :-1]
        pos0 = {int(v): k for k, v in enumerate(ref64["ind0"].tolist())}
        pos1 = {int(v): k for k, v in enumerate(ref64["ind1"].tolist())}
        for (a, b), s in zip(ref64["matches"].tolist(), ref64["scores"].tolist()):
            i, j = pos0[a], pos1[b]
            for line in (la[i], la[:, j]):
                if line.numel() > 1:
                    top = torch.topk(line, 2).values
                    worst = min(worst, float(top[0] - top[1]))
            worst = min(worst, abs(s - conf["filter_threshold"]))
        # a non-match whose score sits at the threshold would be a decision too: every mutual pair's distance from it
        best0, best1 = la.max(1), la.max(0)
        for i in range(la.shape[0]):
            j = int(best0.indices[i])
            if int(best1.indices[j]) == i:
                worst = min(worst, abs(float(best0.values[i].exp()) - conf["filter_threshold"]))
    if conf["width_confidence"] > 0:
        sd64 = {k: v.double() for k, v in sd.items()}
        for i, (d0, d1, _, _) in enumerate(ref64["layers"][:-1]):   # (the last layer is not followed by pruning)
            w, b = sd64[f"log_assignment.{i}.matchability.weight"], sd64[f"log_assignment.{i}.matchability.bias"]
            for d in (d0, d1):
                if d.numel():
                    worst = min(worst, float((torch.sigmoid(d @ w.t() + b) - lc.PRUNE_BAR).abs().min()))
    return worst


@torch.no_grad()
def main():
    rc = reference_conf()
    check_constants(rc)
    for name, case in lc.GOLDEN_CASES.items():
        sd, (f0, f1), conf = lc.case_weights(case), lc.case_inputs(case), lc.conf_of(case)
        net = reference_module(sd, rc, conf)
        got = net(lc.data_of(f0, f1))
        got = {k: (v if isinstance(v, int) else v[0]) for k, v in got.items()}   # batch 1: lists (matches, scores) and tensors alike
        ref32 = lc.oracle(f0, f1, sd, conf)
        ref64 = lc.oracle(f0, f1, sd, conf, torch.float64)
        compare_lightglue(ref32, got, score_tol=1e-5, max_ties=0)                                   # (a)
        for k in ("matches0", "matches1", "prune0", "prune1", "matches"):                           # (b)
            assert torch.equal(ref32[k].long(), ref64[k].long()), (name, k, "fp32 and fp64 decide differently")
        assert ref32["stop"] == ref64["stop"], name
        if "layers" not in ref64:   # the empty exit returns no taps: the case must empty a side after layer 0, whose state is restated here
            assert ref64["stop"] == 2, (name, ref64["stop"])
            from oracle import lightglue_ref as lr
            sd64 = {k: v.double() for k, v in sd.items()}
            enc = [lr.positional_encoding(lr.normalize_keypoints(f["kpts"].double(), f["size"]), sd64["posenc.Wr.weight"]) for f in (f0, f1)]
            d = [lr.self_block(lr._lin(f["desc"].double(), sd64, "input_proj"), e, sd64, 0, rc["num_heads"]) for f, e in zip((f0, f1), enc)]
            d0, d1 = lr.cross_block(d[0], d[1], sd64, 0, rc["num_heads"])
            ref64 = {**ref64, "layers": [(d0, d1, None, None), None]}
        worst = margins64(ref64, sd, conf)                                                           # (c)
        assert worst >= lc.MIN_MARGIN, (name, "decision margin", worst)
        S = int(got["matches"].shape[0])
        dense_res = desc_res = 0.0
        if "log_assignment" in ref64:
            dense_res = float((ref64["log_assignment"][:-1, :-1] - ref32["log_assignment"][:-1, :-1].double()).abs().max())
            desc_res = max(float((a.double() - b).abs().max()) for a, b in zip(ref32["layers"][-1][:2], ref64["layers"][-1][:2]))
        p0, p1 = got["prune0"].long(), got["prune1"].long()
        live = (len(ref32.get("ind0", [])), len(ref32.get("ind1", [])))
        if name == "fixed":                                                                          # (d)
            assert conf["width_confidence"] < 0 and case["m"] % 32 and case["n"] % 32 and case["size0"][0] != case["size0"][1] and S >= 10
        if name == "prune":
            assert len(set(p0.tolist())) >= 3 and len(set(p1.tolist())) >= 3 and S >= 10, (set(p0.tolist()), set(p1.tolist()), S)
            assert live[0] < 0.8 * case["m"] and live[1] < 0.8 * case["n"], live
        if name == "odd":
            assert (case["m"], case["n"]) == (33, 97) and S >= 10
        if name == "prune_to_empty":
            assert got["stop"] < rc["n_layers"] and S == 0 and float(got["matching_scores0"].abs().max()) == 0.0
        if name == "wide":
            assert case["m"] > 256 and 9 <= (case["n"] + 31) // 32 <= 10 and 9 <= (case["m"] + 31) // 32 <= 10 and S >= 10
        np.savez_compressed(ROOT / "tests" / "golden" / f"lgl_{name}.npz", matches0=got["matches0"].numpy(), matches1=got["matches1"].numpy(),
                            matching_scores0=got["matching_scores0"].numpy(), matching_scores1=got["matching_scores1"].numpy(),
                            matches=got["matches"].numpy(), scores=got["scores"].numpy(), prune0=p0.numpy(), prune1=p1.numpy(), stop=np.int64(got["stop"]),
                            dense_res64=np.float64(dense_res), desc_res64=np.float64(desc_res), min_margin=np.float64(worst))
        print(f"{name}: {case['m']} x {case['n']} -> stop {got['stop']}, {S} matches, live {live}, prune values {sorted(set(p0.tolist()))} / {sorted(set(p1.tolist()))}, "
              f"smallest fp64 margin {worst:.4f}, fp32 - fp64 log-assignment {dense_res:.2e}, descriptors {desc_res:.2e}; oracle == module")


if __name__ == "__main__":
    main()
