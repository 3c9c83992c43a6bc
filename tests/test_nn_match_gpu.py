"""GPU (MI355X): the nearest-neighbour descriptor matcher (csrc/nn_match.hip, KorniaMatcher) against the fp64 decision rule of tests/nn_ref.py.

Parity inputs (each with its may-set within 1 % of its must-set, asserted):
  * the trained-ALIKED real-photograph features of tests/golden/config1_features_f16.npz: 8 images -> 28 pairs, ~1200 - 2600 x 128, smnn at 0.95
    (the shipped pipelines' mode and threshold), through the per-pair hook and through match_batch;
  * planted unit-norm 256-d sets (nn_ref.planted, 10 % of image 1's rows replaced so the ratio test rejects some) at 2048 and 8000 per side, in
    smnn and mnn; a 16-pair batch at 2048.
``tol`` is measured per input from the reference's fp32 arithmetic (4 x its error against fp64) and printed; with DIM_NN_PARITY_OUT=<file> the figures are also written there
(profiles/nn_match_parity.json is such a record).
The fp64 distances are evaluated by differences with torch on the GPU (test-side reference code only).  Reads nothing outside the repository."""
import importlib
import itertools
import json
import os
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import golden_cases as gc
from tests import nn_ref
from tests.config1_real import golden_features

pytestmark = pytest.mark.gpu
TH = 0.95
NAMES = list(gc.SACRE_COEUR) + list(gc.PYTEST_IMAGES)
ALIKED_CKPT = Path(__file__).parent / "assets" / "aliked-n16rot.pth"


def _m(name):
    return importlib.import_module("deep-image-matching_amd." + name)


def _record(obj):
    print("nn_match parity:", json.dumps(obj))
    out = os.environ.get("DIM_NN_PARITY_OUT")
    if not out:
        return
    try:
        p = Path(out)
        p.parent.mkdir(parents=True, exist_ok=True)
        cur = json.loads(p.read_text()) if p.exists() else []
        p.write_text(json.dumps(cur + [obj], indent=1) + "\n")
    except OSError:
        pass


def _classify(a, b, modes, th=TH):
    """a, b: CPU fp32 (N, D).  {mode: (must, may)}, tol — fp64 distances on the GPU, the fp32 reference on the CPU; the reference itself passes."""
    d2 = nn_ref.d2_fp64(a, b, device="cuda")
    tol = nn_ref.measured_tol(a, b, d2)
    out = {}
    for mode in modes:
        must, may = nn_ref.classify_fp64(a, b, mode, th, tol, d2)
        nn_ref.check_rule(nn_ref.reference_fp32(a, b, mode, th)[0], must, may, f"fp32 reference {mode}")
        out[mode] = (must, may)
    return out, tol


def _table(sets):
    cap = max(max(a.shape[0], b.shape[0]) for a, b in sets)
    tab = torch.zeros(2 * len(sets), cap, sets[0][0].shape[1])
    nt = torch.zeros(2 * len(sets), dtype=torch.int32)
    for p, (a, b) in enumerate(sets):
        tab[2 * p, : a.shape[0]], tab[2 * p + 1, : b.shape[0]] = a, b
        nt[2 * p], nt[2 * p + 1] = a.shape[0], b.shape[0]
    return tab.cuda().contiguous(), nt.cuda()


def _lists(o, P):
    n = o["n_matches"].cpu().numpy()
    m = o["matches"].cpu().numpy()
    return [m[p, : int(n[p])].copy() for p in range(P)]


def _net(mode, D, max_pairs, max_kpts, th=TH, **k):
    return _m("nn_hip").NearestNeighborHIP(mode, th, dim=D, max_pairs=max_pairs, max_kpts=max_kpts, **k)


@pytest.fixture(scope="module")
def aliked():
    feats = {n: golden_features("aliked", n) for n in NAMES}
    pairs = list(itertools.combinations(range(len(NAMES)), 2))
    assert len(pairs) == 28
    desc = {n: torch.from_numpy(np.ascontiguousarray(f["descriptors"].T.astype(np.float32))) for n, f in feats.items()}
    rules, tols = {}, []
    for i, j in pairs:
        r, tol = _classify(desc[NAMES[i]], desc[NAMES[j]], ("smnn",))
        rules[(i, j)] = r["smnn"]
        tols.append(tol)
    n_must, n_may = sum(len(v[0]) for v in rules.values()), sum(len(v[1]) for v in rules.values())
    assert n_must > 4000 and n_may <= 0.01 * n_must, (n_must, n_may)
    _record({"input": "aliked config1, 28 pairs, smnn 0.95", "tol_max": max(tols), "tol_min": min(tols), "must": n_must, "may": n_may})
    return feats, desc, pairs, rules


def test_aliked_pairs_through_the_hook_and_through_match_batch(hip_lib, aliked):
    feats, desc, pairs, rules = aliked
    capi = _m("capi")
    mt = _m("plugins").KorniaMatcher({"general": {}, "matcher": {"name": "kornia_matcher", "match_mode": "smnn", "th": TH, "on_saturation": "raise"}})
    hook = {}
    for i, j in pairs:
        out = mt._match_pairs(feats[NAMES[i]], feats[NAMES[j]])          # float16 (D, N), as features.h5 holds them
        assert out.dtype == np.int64
        nn_ref.check_rule(out, *rules[(i, j)], f"hook {NAMES[i]} {NAMES[j]}")
        hook[(i, j)] = out
    assert sum(len(v) for v in hook.values()) > 4000
    # the batched path: one feature table of the 8 images, pairs through pair_idx, 16 per call
    cap = max(d.shape[0] for d in desc.values())
    tab = torch.zeros(len(NAMES), cap, 128)
    for k, n in enumerate(NAMES):
        tab[k, : desc[n].shape[0]] = desc[n]
    tab, nt = tab.cuda(), torch.tensor([desc[n].shape[0] for n in NAMES], dtype=torch.int32).cuda()
    net = mt._ensure_pairs(cap, 16)
    assert net.input_dim == 128
    for s in range(0, len(pairs), 16):
        chunk = pairs[s:s + 16]
        pidx = torch.tensor(chunk, dtype=torch.int32).cuda()
        three = net.match_batch_guarded(None, tab, nt, None, pair_idx=pidx, n_pairs=len(chunk), taps=True)
        lists = _lists(three, len(chunk))
        one = net.match_batch(None, tab, nt, None, pair_idx=pidx, n_pairs=len(chunk), taps=True, f16_exact=True)
        torch.cuda.synchronize()
        for p, ij in enumerate(chunk):
            assert np.array_equal(lists[p], hook[ij]), ij                    # hook == batched
        # the fp16-exact one-term path: bit-identical to the three-term path on float16-exact tables
        assert torch.equal(one["n_matches"], three["n_matches"])
        assert all(np.array_equal(x, y) for x, y in zip(_lists(one, len(chunk)), lists))
        assert torch.equal(one["row_stats"].view(torch.int32), three["row_stats"].view(torch.int32))
        assert torch.equal(one["col_stats"].view(torch.int32), three["col_stats"].view(torch.int32))
    assert capi.saturation(hip_lib, None)[0] == 0
    assert net.workspace_bytes() < net.max_pairs * net.nk * net.nk * 4 // 8


@pytest.fixture(scope="module")
def planted_sets():
    cache = {}

    def get(n, seed=0):
        if (n, seed) not in cache:
            a, b = nn_ref.planted(n, 256, seed=seed, replaced=0.1)
            rules, tol = _classify(a, b, ("smnn", "mnn"))
            for mode, (must, may) in rules.items():
                assert len(must) > 0.7 * n and len(may) <= 0.01 * len(must), (n, mode, len(must), len(may))
            if seed == 0:
                _record({"input": f"planted 256-d, {n} per side, 10 % replaced", "tol": tol, **{f"{m}_must": len(v[0]) for m, v in rules.items()},
                         **{f"{m}_may": len(v[1]) for m, v in rules.items()}})
            cache[(n, seed)] = (a, b, rules)
        return cache[(n, seed)]

    return get


@pytest.mark.parametrize("n", [2048, 8000])
def test_planted_sets_in_smnn_and_mnn(hip_lib, planted_sets, n):
    a, b, rules = planted_sets(n)
    tab, nt = _table([(a, b)])
    for mode in ("smnn", "mnn"):
        net = _net(mode, 256, 1, n)
        o = net.match_batch_guarded(None, tab, nt, None, n_pairs=1)
        (m,) = _lists(o, 1)
        nn_ref.check_rule(m, *rules[mode], f"planted {n} {mode}")
        assert len(m) < n                                                  # the replaced rows are rejected
        o2 = net.match_batch(None, tab, nt, None, n_pairs=1)               # two runs: bit-identical
        torch.cuda.synchronize()
        assert torch.equal(o2["n_matches"], o["n_matches"]) and np.array_equal(_lists(o2, 1)[0], m)
        assert torch.equal(o2["scores"][0, : len(m)].view(torch.int32), o["scores"][0, : len(m)].view(torch.int32))
        assert net.workspace_bytes() < n * n * 4 // 8                      # no M x N buffer


def test_sixteen_pair_batch_at_2048(hip_lib, planted_sets):
    sets = [planted_sets(2048, seed)[:2] for seed in range(16)]
    tab, nt = _table(sets)
    net = _net("smnn", 256, 16, 2048)
    lists = _lists(net.match_batch_guarded(None, tab, nt, None, n_pairs=16), 16)
    for seed in range(16):
        nn_ref.check_rule(lists[seed], *planted_sets(2048, seed)[2]["smnn"], f"batch pair {seed}")
    one = _net("smnn", 256, 1, 2048)
    for seed in (0, 7, 15):
        t1, n1 = _table([sets[seed]])
        assert np.array_equal(_lists(one.match_batch(None, t1, n1, None, n_pairs=1), 1)[0], lists[seed])


def test_range_guard_reruns_in_bf16x6_and_still_passes(hip_lib):
    capi = _m("capi")
    a, b = nn_ref.planted(700, 128, seed=3, replaced=0.1)
    a, b = (a * 50000.0)[:640].contiguous(), b * 50000.0                   # elements up to ~2e4: beyond the fp16x3 range of 4094
    rules, tol = _classify(a, b, ("smnn",))
    must, may = rules["smnn"]
    assert len(may) <= 0.01 * len(must)
    f0, f1 = {"descriptors": a.numpy().T}, {"descriptors": b.numpy().T}      # float32 (D, N) views of (N, D) arrays
    strict = _m("plugins").KorniaMatcher({"general": {}, "matcher": {"name": "kornia_matcher", "match_mode": "smnn", "th": TH, "on_saturation": "raise"}})
    with pytest.raises(capi.SaturationError):
        strict._match_pairs(f0, f1)
    mt = _m("plugins").KorniaMatcher({"general": {}, "matcher": {"name": "kornia_matcher", "match_mode": "smnn", "th": TH}})
    nn_ref.check_rule(mt._match_pairs(f0, f1), must, may, "guarded re-run")
    assert capi.saturation(hip_lib, None)[0] == 0


def test_pair_jobs_run_end_to_end_through_the_batched_image_matcher(hip_lib, tmp_path):
    """superpoint+kornia_matcher and ALIKED + kornia_matcher on the real photographs: extract_features -> features.h5 -> match_pairs -> raw_matches.h5 /
    matches.h5, equal to the per-pair hook on the stored features.  The SuperPoint weights are synthetic (a plumbing run: the rule is checked without
    the cap); ALIKED runs its trained checkpoint."""
    bm, export, plugins = _m("batched_matcher"), _m("export"), _m("plugins")
    assert ALIKED_CKPT.exists()
    paths = [gc.REAL_DIR / n for n in gc.SACRE_COEUR[:3]]
    pairs = [(paths[0].name, paths[1].name), (paths[0].name, paths[2].name), (paths[1].name, paths[2].name)]
    general = {"geom_verification": "NONE", "min_inliers_per_pair": 1, "min_inlier_ratio_per_pair": 0.0}
    jobs = (("superpoint", plugins.SuperPointExtractor({"general": general, "extractor": {"name": "superpoint", **gc.CONFIG1_SP, "allow_synthetic_weights": True}}), False),
            ("aliked", plugins.AlikedExtractor({"general": general, "extractor": {"name": "aliked", **gc.CONFIG1_AL, "weights_path": str(ALIKED_CKPT)}}), True))
    for tag, ex, capped in jobs:
        mt = plugins.KorniaMatcher({"general": general, "matcher": {"name": "kornia_matcher", "match_mode": "smnn", "th": TH}})
        shim = bm.BatchedImageMatcher(ex, mt, tmp_path / tag, image_batch=3, pair_batch=2, verify=False)
        fp = shim.extract_features(paths)
        mp = shim.match_pairs(fp, pairs)
        raw, ver = export.MatchStore.read_all(tmp_path / tag / "raw_matches.h5"), export.MatchStore.read_all(mp)
        total = 0
        for a, b in pairs:
            fa, fb = export.FeatureStore.read(fp, a), export.FeatureStore.read(fp, b)
            one = mt._match_pairs(fa, fb)
            assert np.array_equal(raw[(a, b)], one), (tag, a, b)
            r, _ = _classify(torch.from_numpy(fa["descriptors"].T.astype(np.float32).copy()), torch.from_numpy(fb["descriptors"].T.astype(np.float32).copy()), ("smnn",))
            must, may = r["smnn"]
            nn_ref.check_rule(one, must, may, f"{tag} {a} {b}")
            if len(one) >= 8:
                assert np.array_equal(ver[(a, b)], one)
            total += len(one)
            if capped:
                assert len(may) <= 0.01 * max(len(must), 1), (tag, a, b, len(must), len(may))
        assert total > (300 if capped else 0), (tag, total)
