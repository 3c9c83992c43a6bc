"""GPU (MI355X): adaptive LightGlue (reference-default depth / width confidences) at full size against the oracle — the flagship adaptive batch
and the plugin's handle reused across pair sizes.  The CPU twins (tests/test_lightglue_adaptive_emu.py) run the same sequences on the emulator,
where kernels run synchronously: the real concurrency between the host following the stop flags and lg_decide_kernel exists only here."""
import importlib

import numpy as np
import pytest
import torch

from oracle import lightglue_ref
from tests import adaptive_cases as ac

pytestmark = pytest.mark.gpu


def test_adaptive_workload_at_full_size_vs_oracle_full_and_ragged(hip_lib):
    """workloads.adaptive_lightglue_workload(14, 2048) — bench.py's adaptive batch: stop layers 3 .. 9 twice, ~25 % of every image prunable — as ONE
    match_batch on a 14-pair handle (which selects the large-batch kernels by itself), then a second, ragged call on the SAME handle (counts cut down
    to 1 .. 2047 keypoints on six of the pairs).  Per pair: stop layer, prune counters, matches0 / 1, the compact list, scores and the dense
    log-assignment against the oracle at compare_lightglue's defaults (1e-3; near-ties 1e-4 in the oracle's own pruned-space log-assignment)."""
    from tests.test_configs_gpu import _record
    lg = importlib.import_module("deep-image-matching_amd.lightglue_hip")
    capi = importlib.import_module("deep-image-matching_amd.capi")
    P, N = 14, 2048
    wl = ac.workload(P, N)
    sd, expect = wl[0], wl[4]
    assert expect.tolist() == list(ac.STOPS) * 2
    net = lg.LightGlueHIP(sd, ac.CONF, max_pairs=P, max_kpts=N)
    ragged = [(N, N)] * P
    for p, mn in zip((0, 2, 4, 8, 10, 13), ac.RAGGED_2048):
        ragged[p] = mn
    capi.saturation(hip_lib, None, reset=True)
    measured = {"test": "adaptive_workload_14x2048_vs_oracle", "calls": []}
    for name, counts in (("full", None), ("ragged", ragged)):
        call = ac.call_of(wl, range(P), N, counts)
        o = net.match_batch(*[t.cuda() for t in call], dense=True)
        torch.cuda.synchronize()
        total, sites = capi.saturation(hip_lib, None, reset=True)
        assert total == 0, sites
        o = {k: v.cpu() for k, v in o.items()}
        worst = {"call": name, "stops": o["stop"].tolist(), "max_score_diff": 0.0, "max_log_assignment_diff": 0.0, "explained_near_ties": 0, "matches": 0}
        for p in range(P):
            m, n = int(call[2][2 * p]), int(call[2][2 * p + 1])
            ref = ac.oracle_of(sd, call, 2 * p, 2 * p + 1)
            if counts is None:
                assert ref["stop"] == int(expect[p]), (p, ref["stop"])
                assert all(0.2 < float((ref[k] < ref[k].max()).float().mean()) < 0.3 for k in ("prune0", "prune1")), p
                assert ref["matches"].shape[0] > 1000, (p, ref["matches"].shape)
            res = ac.check_row(ac.row_of(o, p, m, n), ref)
            print(name, p, (m, n), "stop", ref["stop"], "S", ref["matches"].shape[0], res)
            worst["max_score_diff"] = max(worst["max_score_diff"], res["max_matching_scores0_diff"], res["max_matching_scores1_diff"])
            worst["max_log_assignment_diff"] = max(worst["max_log_assignment_diff"], res.get("max_log_assignment_diff", 0.0))
            worst["explained_near_ties"] += len(res.get("explained_near_ties", []))
            worst["matches"] += int(ref["matches"].shape[0])
        measured["calls"].append(worst)
    _record(measured)


def test_plugin_matcher_handle_across_pair_sizes_on_hardware(hip_lib, tmp_path):
    """LightGlueMatcher._match_pairs on the GPU (the staged path: page-locked staging, dim_lg_stage_features, the `_lean` device buffers) with ONE matcher
    for pairs of 2048 -> 300 -> 2100 (more than 2048 rows of the 4096-row handle) -> 61 -> 4100 (rebuilds the handle with 8192 rows and reallocates
    `_lean`) -> 1024 keypoints, designed to stop after 9 / 3 / 5 / 3 / 7 / 4 layers, the whole sequence twice.  float16 (D, N) features as features.h5
    holds them; every (S, 2) result equals the oracle's match list on the same fp16-rounded inputs; the range guard raises instead of falling back."""
    plugins = importlib.import_module("deep-image-matching_amd.plugins")
    sd = ac.workload(1, 61, stops=(3,))[0]
    torch.save(sd, tmp_path / "lg.pth")
    m = plugins.LightGlueMatcher({"general": {}, "matcher": {"name": "lightglue", "depth_confidence": 0.95, "width_confidence": 0.99, "filter_threshold": 0.1,
                                                             "pruning_min_kpts": -1, "weights_path": str(tmp_path / "lg.pth"), "on_saturation": "raise"}})
    assert m._conf["n_layers"] == 9 and m._conf["pruning_min_kpts"] == -1
    refs, rows = {}, []
    for rep in range(2):
        for n, drop, stop in ((2048, 0, 9), (300, 20, 3), (2100, 77, 5), (61, 4, 3), (4100, 0, 7), (1024, 1, 4)):
            sd_n, kp, de, sz, _ = ac.workload(1, n, stops=(stop,))
            f0, k0, d0 = ac.h5_features(kp[0], de[0], sz[0])
            f1, k1, d1 = ac.h5_features(kp[1, :n - drop], de[1, :n - drop], sz[1])
            assert f0["descriptors"].shape == (256, n) and f0["descriptors"].dtype == np.float16
            got = m._match_pairs(f0, f1)
            if n not in refs:
                assert all(torch.equal(sd_n[k], sd[k]) for k in sd)
                refs[n] = lightglue_ref.lightglue_forward(k0, d0, sz[0], k1, d1, sz[1], sd, ac.CONF)
            ref = refs[n]
            assert ref["stop"] == stop and ref["matches"].shape[0] > 0.5 * (n - drop), (n, ref["stop"], ref["matches"].shape)
            assert got.dtype == np.int64 and np.array_equal(got, ref["matches"].numpy()), (rep, n, got.shape, ref["matches"].shape)
            rows.append(m._net_n)
    assert rows == [4096, 4096, 4096, 4096, 8192, 8192] + [8192] * 6
