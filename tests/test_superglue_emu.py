"""CPU: the HIP SuperGlue sources (sg_kernels.hip, sg_api.hip and the LightGlue launchers they compose) on the test emulator against the
reference module's goldens and the fp64 oracle (cases in tests/superglue_cases.py), the host-side weight preparation, the SuperGlueMatcher plugin
and the weight loader."""
import importlib
import types
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import superglue_cases as cases
from tests import superglue_ref as ref

weights = importlib.import_module("deep-image-matching_amd.weights")


# ---- 1 + 2. goldens and taps ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.GOLDEN_CASES))
def test_superglue_golden(emu_lib, name):
    cases.golden(emu_lib, "cpu", name)


def test_superglue_golden_in_bf16x6(emu_lib):
    """The exact arithmetic the range guard falls back to, on the case with more than one query block."""
    cases.golden(emu_lib, "cpu", "wide", arithmetic="bf16x6")


# ---- 2b + 3. Sinkhorn alone -----------------------------------------------------------------------------------------------------------------
def test_superglue_sinkhorn_potentials_and_marginals_against_fp64(emu_lib):
    cases.sinkhorn_alone(emu_lib, "cpu")


# ---- 4 - 6, 8 -------------------------------------------------------------------------------------------------------------------------------
def test_superglue_edge_counts(emu_lib):
    cases.edge_counts(emu_lib, "cpu")


def test_superglue_batch_equals_singles_and_handles_can_be_reused(emu_lib):
    cases.batch_equals_singles(emu_lib, "cpu")


def test_superglue_range_guard_fires_and_the_guarded_rerun_equals_the_golden(emu_lib):
    cases.guard(emu_lib, "cpu")


def test_superglue_abi(emu_lib):
    cases.abi(emu_lib, "cpu")


# ---- 7. head permutation and BatchNorm fold (host only) ---------------------------------------------------------------------------------
def test_prepared_weights_reproduce_the_unfolded_module_in_fp64(monkeypatch):
    """The permuted (head-major) and BatchNorm-folded weights, kept in fp64, against the oracle on the module's own layout (unfolded BatchNorm,
    channel c = d * 4 + h from view(b, 64, 4, n)) on random input: 1e-12 relative.  Assuming c = h * 64 + d — no permutation — misses by O(1)."""
    sd = weights.synthetic_superglue_state_dict(9, n_layers=4)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    g = torch.Generator().manual_seed(2)
    d0, d1 = torch.randn(37, 256, generator=g, dtype=torch.float64), torch.randn(53, 256, generator=g, dtype=torch.float64)
    x = torch.randn(41, 3, generator=g, dtype=torch.float64)
    want0, want1 = d0, d1
    for i in range(4):
        s0, s1 = (want1, want0) if i % 2 else (want0, want1)
        want0, want1 = want0 + ref.propagation(sd64, i, want0, s0), want1 + ref.propagation(sd64, i, want1, s1)
    enc_want = ref.keypoint_encoder(sd64, x[:, :2], x[:, 2])
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())   # noqa: E731

    perm = weights.superglue_head_permutation()
    assert perm.tolist()[:3] == [0, 4, 8] and perm.tolist()[64:66] == [1, 5] and sorted(perm.tolist()) == list(range(256))
    prep = weights.prepare_superglue_weights(sd, dtype=torch.float64)
    got0, got1 = cases.folded_forward(prep, 4, d0, d1)
    assert max(rel(got0, want0), rel(got1, want1)) <= 1e-12 and rel(cases.folded_encoder(prep, x), enc_want) <= 1e-12
    # what the library is handed is the fp32 rounding of exactly these tensors
    prep32 = weights.prepare_superglue_weights(sd)
    assert all(v.dtype == torch.float32 and torch.equal(v, prep[k].float()) for k, v in prep32.items())
    # ... and the other head layout is not the module's
    monkeypatch.setattr(weights, "superglue_head_permutation", lambda: torch.arange(256))
    bad0, _ = cases.folded_forward(weights.prepare_superglue_weights(sd, dtype=torch.float64), 4, d0, d1)
    assert rel(bad0, want0) > 1e-3


def test_superglue_loader_validates_and_reads_the_environment(tmp_path, monkeypatch):
    sd = weights.synthetic_superglue_state_dict(3, n_layers=2)
    assert weights.validate_superglue_state_dict(sd) == 2 and weights.superglue_n_layers(weights.synthetic_superglue_state_dict(3)) == 18
    assert set(weights.superglue_state_dict_shapes(2)) <= set(sd)
    path = tmp_path / "superglue_outdoor.pth"
    torch.save(sd, path)
    got = weights.load_superglue_state_dict(str(path))
    assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    monkeypatch.setenv("DIM_SUPERGLUE_WEIGHTS", str(path))
    assert set(weights.load_superglue_state_dict(None)) == set(sd)
    monkeypatch.delenv("DIM_SUPERGLUE_WEIGHTS")
    with pytest.raises(weights.MissingWeightsError):
        weights.load_superglue_state_dict(None)
    bad = dict(sd)
    bad["gnn.layers.1.mlp.0.weight"] = torch.zeros(512, 256, 1)
    torch.save(bad, path)
    with pytest.raises(ValueError, match="mlp.0.weight"):
        weights.load_superglue_state_dict(str(path))
    odd = {k: v for k, v in sd.items() if not k.startswith("gnn.layers.1.")}
    torch.save(odd, path)
    with pytest.raises(ValueError, match="multiple of 2"):
        weights.load_superglue_state_dict(str(path))


# ---- 9. the plugin ------------------------------------------------------------------------------------------------------------------------
def _feats(f, dtype=np.float32, dn=True, **extra):
    """A feature dict as features.h5 holds it: descriptors (256, N), image_size (H, W), plus keys the matcher must ignore."""
    d = f["desc"].numpy().astype(dtype)
    return {"keypoints": f["kpts"].numpy().astype(dtype), "descriptors": np.ascontiguousarray(d.T) if dn else d, "scores": f["scores"].numpy().astype(dtype),
            "image_size": np.array([int(f["size"][0]), int(f["size"][1])]), "tile_idx": np.zeros(f["kpts"].shape[0], np.int32), "feature_path": "x.h5",
            "im_path": "x.jpg", **extra}


def test_superglue_plugin(emu_install, monkeypatch):
    plugins = importlib.import_module("deep-image-matching_amd.plugins")
    M = plugins.SuperGlueMatcher
    assert M.default_config == {"name": "superglue", "weights": "outdoor", "sinkhorn_iterations": 20, "match_threshold": 0.3} and M._default_conf == {}
    assert M.min_matches == 20 and M.max_feat_no_tiling == 50000 and M.required_inputs == []
    with pytest.raises(weights.MissingWeightsError):
        M({"general": {}, "matcher": {"name": "superglue"}})
    with pytest.raises(ValueError, match="indoor"):
        M({"general": {}, "matcher": {"name": "superglue", "weights": "aerial", "allow_synthetic_weights": True}})
    case = {"seed": 31, "m": 90, "n": 75, "size0": (300.0, 640.0), "size1": (640.0, 300.0)}   # non-square: (H, W) and (W, H) differ
    f0, f1 = cases.case_inputs(case)
    seen, call = [], cases.sg_mod.SuperGlueHIP.match_batch

    def spy(self, *a, **k):
        seen.append((a[4].detach().cpu().clone(), k.get("sinkhorn_iterations"), k.get("match_threshold")))
        return call(self, *a, **k)
    monkeypatch.setattr(cases.sg_mod.SuperGlueHIP, "match_batch", spy)
    mt = M({"general": {}, "matcher": {"name": "superglue", "allow_synthetic_weights": True}})
    sd = mt._sd
    got = mt._match_pairs(_feats(f0), _feats(f1))
    # keys omitted: the network's 100 / 0.2, not the class's 20 / 0.3; the library is handed (width, height)
    assert seen[-1][1:] == (100, 0.2) and seen[-1][0].tolist() == [[640.0, 300.0], [300.0, 640.0]]
    want = cases.oracle(f0, f1, sd, cases.NET)
    assert got.dtype == np.int64 and got.shape[1] == 2 and got.shape[0] > 10 and np.array_equal(got, want["matches"].numpy())
    # SuperGlue has no rotary: the encoder sees absolute positions, so (W, H) in place of (H, W) is another result
    swapped = cases.oracle({**f0, "size": f0["size"].flip(0)}, {**f1, "size": f1["size"].flip(0)}, sd, cases.NET)
    sw = mt._match_pairs(_feats({**f0, "size": f0["size"].flip(0)}), _feats({**f1, "size": f1["size"].flip(0)}))
    assert np.array_equal(sw, swapped["matches"].numpy())
    assert not torch.equal(swapped["matching_scores0"], want["matching_scores0"])
    # both values are read at every call
    mt.config["matcher"]["sinkhorn_iterations"], mt.config["matcher"]["match_threshold"] = 20, 0.3
    again = mt._match_pairs(_feats(f0), _feats(f1))
    assert seen[-1][1:] == (20, 0.3)
    want20 = cases.oracle(f0, f1, sd, {"sinkhorn_iterations": 20, "match_threshold": 0.3})
    assert np.array_equal(again, want20["matches"].numpy())
    mt.config["matcher"]["match_threshold"] = 0.999999
    assert mt._match_pairs(_feats(f0), _feats(f1)).shape == (0, 2)
    del mt.config["matcher"]["sinkhorn_iterations"], mt.config["matcher"]["match_threshold"]
    # float16 arrays, (N, D) descriptors
    h0, h1 = _feats(f0, np.float16), _feats(f1, np.float16, dn=False)
    g = lambda h, f: {"kpts": torch.from_numpy(h["keypoints"].astype(np.float32)), "scores": torch.from_numpy(h["scores"].astype(np.float32)),   # noqa: E731
                      "desc": torch.from_numpy((h["descriptors"].T if h["descriptors"].shape[0] == 256 else h["descriptors"]).astype(np.float32)), "size": f["size"]}
    half = mt._match_pairs(h0, h1)
    assert half.dtype == np.int64 and np.array_equal(half, cases.oracle(g(h0, f0), g(h1, f1), sd, cases.NET)["matches"].numpy())
    for key in ("scores", "image_size"):
        bad = _feats(f0)
        del bad[key]
        with pytest.raises(ValueError, match=key):
            mt._match_pairs(bad, _feats(f1))
    empty = mt._match_pairs({"keypoints": np.zeros((0, 2), np.float32), "descriptors": np.zeros((256, 0), np.float32), "scores": np.zeros(0, np.float32),
                             "image_size": np.array([300, 640])}, _feats(f1))
    assert empty.shape == (0, 2) and empty.dtype == np.int64


def test_superpoint_feeds_superglue_from_the_shipped_yaml(emu_install, tmp_path, monkeypatch):
    """config/superpoint+superglue.yaml (the committed byte copy), unmodified: both plugins are built from its sections and one 96 x 128 image
    goes through SuperPoint -> SuperGlue on the emulator: the matches are the oracle's on the extractor's features, and matching an image with
    itself pairs keypoints with themselves."""
    import yaml
    plugins = importlib.import_module("deep-image-matching_amd.plugins")
    raw = yaml.safe_load((Path(__file__).parent / "golden" / "reference_config" / "superpoint+superglue.yaml").read_text())
    assert raw["matcher"] == {"name": "superglue", "weights": "outdoor", "sinkhorn_iterations": 20, "match_threshold": 0.3}
    cfg = types.SimpleNamespace(**{k: dict(raw.get(k) or {}) for k in ("general", "extractor", "matcher")})
    torch.save(weights.synthetic_superpoint_state_dict(1234), tmp_path / "sp.pth")
    torch.save(weights.synthetic_superglue_state_dict(3, n_layers=4, final_gain=40.0), tmp_path / "sg.pth")   # (sharp: the seeded SuperPoint's descriptors are all alike)
    monkeypatch.setenv("DIM_SUPERPOINT_WEIGHTS", str(tmp_path / "sp.pth"))
    monkeypatch.setenv("DIM_SUPERGLUE_WEIGHTS", str(tmp_path / "sg.pth"))
    ex, mt = plugins.SuperPointExtractor(cfg), plugins.SuperGlueMatcher(cfg)
    img = (np.random.default_rng(3).random((96, 128)) * 255).astype(np.float32)
    feats = ex._extract(img)
    n = feats["keypoints"].shape[0]
    assert n > 20 and feats["descriptors"].shape == (256, n) and feats["scores"].shape == (n,)
    f = {**feats, "image_size": np.array([96, 128], np.int32)}
    out = mt._match_pairs(f, f)
    g = {"kpts": torch.from_numpy(feats["keypoints"]).float(), "desc": torch.from_numpy(feats["descriptors"]).float().T.contiguous(),
         "scores": torch.from_numpy(feats["scores"]).float(), "size": torch.tensor([96.0, 128.0])}
    want = cases.oracle(g, g, mt._sd, {"sinkhorn_iterations": 20, "match_threshold": 0.3})
    assert out.dtype == np.int64 and out.ndim == 2 and out.shape[1] == 2 and np.array_equal(out, want["matches"].numpy())
    assert out.shape[0] > 0.25 * n and np.array_equal(out[:, 0], out[:, 1]) and mt._net.n_layers == 4
