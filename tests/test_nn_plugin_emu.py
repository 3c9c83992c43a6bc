"""CPU (emulator): the KorniaMatcher plugin (reference matchers/kornia_matcher.py) — the per-pair hook on the arrays features.h5 holds, under the
reference's real MatcherBase, and through the batched paths (BatchedImageMatcher, PairMatchingPipeline).

Parity inputs are the trained-ALIKED real-photograph features of tests/golden/config1_features_f16.npz (cut to a few hundred rows for the
emulator).  The SuperPoint features the extractor produces here come from SYNTHETIC weights and are degenerate for descriptor matching: they serve
as a shape / dtype plumbing input only — checked against the same must / may rule, without the 1 % cap on the may-set."""
import importlib
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import golden_cases as gc
from tests import nn_ref, refstubs
from tests.config1_real import golden_features

plugins = importlib.import_module("deep-image-matching_amd.plugins")
bm = importlib.import_module("deep-image-matching_amd.batched_matcher")
export = importlib.import_module("deep-image-matching_amd.export")
pipeline = importlib.import_module("deep-image-matching_amd.pipeline")
nn = importlib.import_module("deep-image-matching_amd.nn_hip")

CONF = {"general": {}, "matcher": {"name": "kornia_matcher", "match_mode": "smnn", "th": 0.95}}


def _aliked(name, rows):
    f = golden_features("aliked", name)
    return {"keypoints": f["keypoints"][:rows], "descriptors": np.ascontiguousarray(f["descriptors"][:, :rows]), "image_size": f["image_size"]}


def _rule(f0, f1, mode, th, cap=True):
    a, b = torch.from_numpy(np.asarray(f0["descriptors"]).T.astype(np.float32)), torch.from_numpy(np.asarray(f1["descriptors"]).T.astype(np.float32))
    d2 = nn_ref.d2_fp64(a, b)
    tol = nn_ref.measured_tol(a, b, d2)
    must, may = nn_ref.classify_fp64(a, b, mode, th, tol, d2)
    if cap:
        assert len(may) <= 0.01 * len(must), (len(must), len(may))
    nn_ref.check_rule(nn_ref.reference_fp32(a, b, mode, th)[0], must, may, "fp32 reference")
    return must, may


def test_hook_on_float16_dn_arrays_and_float32_nd_views_gives_the_same_list(emu_install):
    m = plugins.KorniaMatcher(CONF)
    assert m.min_matches == 20 and m.max_feat_no_tiling == 200000 and m.required_inputs == []
    assert m._default_conf == {"name": "kornia_matcher", "match_mode": "smnn", "th": 0.8}
    f0, f1 = _aliked(gc.SACRE_COEUR[0], 300), _aliked(gc.SACRE_COEUR[1], 420)
    assert f0["descriptors"].dtype == np.float16 and f0["descriptors"].shape == (128, 300)
    out = m._match_pairs(f0, f1)
    assert out.dtype == np.int64 and out.ndim == 2 and out.shape[1] == 2 and len(out) >= 20
    must, may = _rule(f0, f1, "smnn", 0.95)
    nn_ref.check_rule(out, must, may, "hook f16")

    def nd_view(f):   # what an extractor hook returns: the transposed view of an owned float32 (N, D) array
        return {**f, "descriptors": np.ascontiguousarray(f["descriptors"].T.astype(np.float32)).T}

    g0, g1 = nd_view(f0), nd_view(f1)
    assert g0["descriptors"].shape == (128, 300) and not g0["descriptors"].flags.c_contiguous
    assert np.array_equal(m._match_pairs(g0, g1), out)                       # three MFMA terms == the one-term fp16-exact path
    assert np.array_equal(m._match_pairs(f0, g1), out)                       # mixed dtypes / layouts
    h0 = {**f0, "descriptors": f0["descriptors"].astype(np.float32)}         # float32, C-contiguous (D, N)
    assert np.array_equal(m._match_pairs(h0, f1), out)
    # the other modes, and the default threshold
    for mode, th in (("nn", 0.8), ("mnn", 0.8), ("snn", 0.9)):
        mm = plugins.KorniaMatcher({"general": {}, "matcher": {"name": "kornia_matcher", "match_mode": mode, "th": th}})
        must, may = _rule(f0, f1, mode, th)
        nn_ref.check_rule(mm._match_pairs(f0, f1), must, may, mode)
    # an empty side
    e = {**f0, "descriptors": f0["descriptors"][:, :0], "keypoints": f0["keypoints"][:0]}
    assert m._match_pairs(e, f1).shape == (0, 2) and m._match_pairs(f0, e).shape == (0, 2)


def test_unsupported_modes_are_rejected_at_construction(emu_install):
    for mode in ("fginn", "adalam", "lightglue", "bogus"):
        with pytest.raises(ValueError, match="nn.*mnn.*snn.*smnn"):
            plugins.KorniaMatcher({"general": {}, "matcher": {"name": "kornia_matcher", "match_mode": mode}})
    with pytest.raises(ValueError):
        plugins.KorniaMatcher({"general": {}, "matcher": {"name": "kornia_matcher", "arithmetic": "fp8"}})


def _write_images(folder: Path, n=4):
    from PIL import Image

    rng = np.random.default_rng(0)
    base = (rng.random((100, 120)) * 255).astype(np.uint8)
    folder.mkdir(parents=True)
    paths = []
    for i, (dy, dx, hw) in enumerate([(0, 0, (56, 72)), (8, 8, (56, 72)), (16, 0, (56, 72)), (0, 16, (48, 64))][:n]):
        p = folder / f"im{i}.png"
        Image.fromarray(base[dy:dy + hw[0], dx:dx + hw[1]]).save(p)
        paths.append(p)
    return paths


def test_batched_image_matcher_writes_what_the_per_pair_hook_returns(emu_install, tmp_path):
    paths = _write_images(tmp_path / "images")
    general = {"geom_verification": "NONE", "min_inliers_per_pair": 1, "min_inlier_ratio_per_pair": 0.0}
    ex = plugins.SuperPointExtractor({"general": general, "extractor": {"name": "superpoint", "max_keypoints": 150, "nms_radius": 2, "keypoint_threshold": 0.001,
                                                                         "remove_borders": 2, "allow_synthetic_weights": True}})
    mt = plugins.KorniaMatcher({"general": general, "matcher": {"name": "kornia_matcher", "match_mode": "smnn", "th": 0.95}})
    shim = bm.BatchedImageMatcher(ex, mt, tmp_path / "out", image_batch=3, pair_batch=2)
    fp = shim.extract_features(paths)
    pairs = [(paths[0].name, paths[1].name), (paths[0].name, paths[2].name), (paths[1].name, paths[3].name)]
    mp = shim.match_pairs(fp, pairs)
    raw = export.MatchStore.read_all(tmp_path / "out" / "raw_matches.h5")
    ver = export.MatchStore.read_all(mp)
    n_tot = 0
    for a, b in pairs:
        fa, fb = export.FeatureStore.read(fp, a), export.FeatureStore.read(fp, b)
        one = mt._match_pairs(fa, fb)
        assert np.array_equal(raw[(a, b)], one)
        must, may = _rule(fa, fb, "smnn", 0.95, cap=False)       # synthetic-weight SuperPoint features: plumbing input, no cap (module docstring)
        nn_ref.check_rule(one, must, may, f"{a} {b}")
        if len(one) >= 8:
            assert np.array_equal(ver[(a, b)], one)
        else:
            assert (a, b) not in ver
        n_tot += len(one)
    assert n_tot > 0


def test_pair_matching_pipeline_runs_with_the_nearest_neighbour_matcher(emu_install):
    feats = [_aliked(n, r) for n, r in zip(gc.SACRE_COEUR[:3], (300, 420, 360))]
    cap, D = 420, 128
    de = torch.zeros(3, cap, D)
    n = torch.tensor([f["descriptors"].shape[1] for f in feats], dtype=torch.int32)
    for i, f in enumerate(feats):
        de[i, : int(n[i])] = torch.from_numpy(f["descriptors"].T.astype(np.float32))
    table = (torch.zeros(3, cap, 2), torch.zeros(3, cap), de, n, torch.zeros(3, 2))
    net = nn.NearestNeighborHIP("mnn", dim=D, max_pairs=2, max_kpts=cap, device="cpu", lib=emu_install)
    pairs = torch.tensor([[0, 1], [0, 2], [1, 2]], dtype=torch.int32)
    cnt, mt, ms = pipeline.PairMatchingPipeline(None, net).match_all(table, pairs)
    lists = pipeline.PairMatchingPipeline.to_match_lists(cnt, mt, ms)
    for (i, j), (m, _) in zip(pairs.tolist(), lists):
        must, may = _rule(feats[i], feats[j], "mnn", 0.8)
        nn_ref.check_rule(m.numpy(), must, may, f"pipeline {i} {j}")


@pytest.mark.skipif(not refstubs.available(), reason="the reference tree is not present")
def test_kornia_matcher_under_the_reference_matcher_base(emu_install, tmp_path):
    """Config -> SuperPointExtractor.extract -> features.h5 -> KorniaMatcher(config).match(...) -> raw_matches.h5 / matches.h5, with the reference's
    own MatcherBase driving the hook (tests/test_reference_base_classes.py's set-up)."""
    added = refstubs.install(find_fundamental=lambda p0, p1, *a: (np.eye(3), np.ones((len(p0), 1), np.uint8)))
    for k in [k for k in sys.modules if k.startswith("deep-image-matching_amd.plugins")]:
        del sys.modules[k]
    try:
        plg = importlib.import_module("deep-image-matching_amd.plugins")
        assert plg.HAVE_DIM
        config_mod = importlib.import_module("deep_image_matching.config")
        mb = importlib.import_module("deep_image_matching.matchers.matcher_base")
        h5 = importlib.import_module("deep_image_matching.io.h5")
        assert issubclass(plg.KorniaMatcher, mb.MatcherBase)
        mro = plg.KorniaMatcher.__mro__
        assert mro.index(importlib.import_module("deep-image-matching_amd.tile_matching").BatchedTileMatchingMixin) < mro.index(mb.MatcherBase)
        with pytest.raises(TypeError):
            plg.KorniaMatcher({"general": {}, "matcher": {}})
        imgs = _write_images(tmp_path / "images", n=2)
        import yaml
        weights = importlib.import_module("deep-image-matching_amd.weights")
        torch.save(weights.synthetic_superpoint_state_dict(1234), tmp_path / "sp.pth")
        yml = tmp_path / "user.yaml"
        yml.write_text(yaml.safe_dump({
            "general": {"geom_verification": "NONE", "min_inliers_per_pair": 1, "min_inlier_ratio_per_pair": 0.0},
            "extractor": {"name": "superpoint", "max_keypoints": 150, "nms_radius": 2, "keypoint_threshold": 0.001, "remove_borders": 2,
                          "weights_path": str(tmp_path / "sp.pth")},
            "matcher": {"name": "kornia_matcher", "match_mode": "smnn", "th": 0.95}}))
        cfg = config_mod.Config({"dir": str(tmp_path), "pipeline": "superpoint+kornia_matcher", "strategy": "bruteforce", "tiling": "none",
                                 "force": True, "config_file": str(yml), "outs": str(tmp_path / "out")})
        ex = plg.SuperPointExtractor(cfg)
        for p in imgs:
            fp = ex.extract(p)
        m = plg.KorniaMatcher(cfg)
        assert m._mode == "smnn" and m._th == 0.95
        matches_path = cfg.general["output_dir"] / "matches.h5"
        out = m.match(fp, matches_path, imgs[0], imgs[1])
        f0, f1 = h5.get_features(fp, imgs[0].name), h5.get_features(fp, imgs[1].name)
        assert out is not None and out.dtype == np.int64 and np.array_equal(out, m._match_pairs(f0, f1))
        must, may = _rule(f0, f1, "smnn", 0.95, cap=False)       # synthetic-weight SuperPoint features: plumbing input, no cap
        nn_ref.check_rule(out, must, may, "reference flow")
        raw = h5.get_matches(cfg.general["output_dir"] / "raw_matches.h5", imgs[0].name, imgs[1].name)
        assert np.array_equal(np.asarray(raw), out)
    finally:
        refstubs.uninstall(added)
        for k in [k for k in sys.modules if k.startswith("deep-image-matching_amd.plugins")]:
            del sys.modules[k]
        importlib.import_module("deep-image-matching_amd.plugins")
