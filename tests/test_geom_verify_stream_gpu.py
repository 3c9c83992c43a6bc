"""GPU (MI355X): dim_gv_fundamental beyond 4096 matches per pair (the streaming kernels of csrc/geom_verify.hip) against the numpy
oracle at the chunk edges and against the LDS-resident kernels; the batched pipeline shim at 4200 keypoints per image; per-tile
verification of the device tile matcher."""
import importlib

import numpy as np
import pytest
import torch

from oracle import geom_ref
from tests import gv_stream_cases as gc

pytestmark = pytest.mark.gpu


def _verifier(err):
    verify = importlib.import_module("deep-image-matching_amd.verify")
    return verify.DeviceVerifier(threshold=gc.THRESHOLD, iters=gc.ITERS, error_type=err, seed=gc.SEED)


def test_streaming_path_equals_the_oracle_at_chunk_edges_gpu(hip_lib):
    """The six-pair call of tests/test_geom_verify_stream_emu.py on hardware (NK = 8193), with the allowance of
    tests/test_geom_verify_gpu.py: at most 2 mask places and 2 in the count per pair, whatever n is."""
    kt, mt, n = gc.tables(gc.six_pair_cases(), nk=8193)
    kt, mt, n = kt.cuda(), mt.cuda(), n.cuda()
    for err in ("sampson", "symmetric_epipolar"):
        out = _verifier(err).verify_batch(kt, mt, n)
        gc.check_against_oracle(out, err, mask_places=2, count_places=2)


def test_result_does_not_depend_on_the_table_width_gpu(hip_lib):
    cases = [gc.scene(0), gc.scene(3)]
    for err in ("sampson", "symmetric_epipolar"):
        v = _verifier(err)
        lds = v.verify_batch(*(t.cuda() for t in gc.tables(cases, nk=4096)))
        stream = v.verify_batch(*(t.cuda() for t in gc.tables(cases, nk=4352)))
        assert torch.equal(lds["mask"], stream["mask"][:, :4096]) and not stream["mask"][:, 4096:].any()
        assert torch.equal(lds["n_inliers"], stream["n_inliers"])
        for p, i in enumerate((0, 3)):
            F_oracle = gc.oracle(i, err, p)[0]
            d_paths = gc.f_distance(lds["F"][p].cpu().numpy(), stream["F"][p].cpu().numpy())
            d_oracle = gc.f_distance(lds["F"][p].cpu().numpy(), F_oracle)
            print(f"pair {p} ({err}): F streaming vs LDS {d_paths:.3e}, LDS vs oracle {d_oracle:.3e}")
            assert d_paths <= d_oracle


def _three_views(n_true, n_rand, seed, size=(1024, 1024), noise_px=0.3):
    """Three pinhole views of the same random 3-D points plus, per view, uniformly placed points that correspond to nothing
    (geom_ref.synthetic_two_view's camera model with a third camera).  -> three (n_true + n_rand, 2) float32 arrays, row i of every view
    being the same scene point (or the same non-point)."""
    rng = np.random.default_rng(seed)
    W, H = size
    K = np.array([[0.9 * W, 0, W / 2], [0, 0.9 * W, H / 2], [0, 0, 1.0]])

    def rot(a):
        cx, sx, cy, sy, cz, sz = np.cos(a[0]), np.sin(a[0]), np.cos(a[1]), np.sin(a[1]), np.cos(a[2]), np.sin(a[2])
        return np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])

    cams = [(np.eye(3), np.zeros(3)), (rot(rng.normal(0, 0.08, 3)), np.array([0.5, 0.05, 0.1])), (rot(rng.normal(0, 0.08, 3)), np.array([-0.4, 0.3, 0.05]))]
    views = [[], [], []]
    while len(views[0]) < n_true:
        X = np.array([rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(3, 9)])
        uv = [(K @ (R @ X + t)) for R, t in cams]
        uv = [u[:2] / u[2] for u in uv]
        if all(0 <= u[0] < W and 0 <= u[1] < H for u in uv):
            for v, u in zip(views, uv):
                v.append(u + rng.normal(0, noise_px, 2))
    return [np.concatenate([np.asarray(v), rng.uniform(0, [W, H], (n_rand, 2))]).astype(np.float32) for v in views]


def test_batched_shim_verifies_4200_keypoints_per_image(hip_lib, tmp_path):
    """BatchedImageMatcher.match_pairs with the nearest-neighbour matcher on a three-image feature store of 4200 keypoints each: the matcher
    handle has 8192 slots, so the verifier takes the streaming kernels (this raised ValueError before).  matches.h5 must hold
    apply_reference_filters of the oracle's masks on the raw match lists, within 2 rows per pair."""
    import types
    plugins = importlib.import_module("deep-image-matching_amd.plugins")
    bm = importlib.import_module("deep-image-matching_amd.batched_matcher")
    export = importlib.import_module("deep-image-matching_amd.export")
    verify = importlib.import_module("deep-image-matching_amd.verify")
    N, D, ITERS = 4200, 64, 256
    rng = np.random.default_rng(5)
    base = rng.normal(size=(N, D))
    base = (base / np.linalg.norm(base, axis=1, keepdims=True)).astype(np.float16)      # what features.h5 holds
    views = _three_views(2600, N - 2600, seed=41)
    names = ["a.jpg", "b.jpg", "c.jpg"]
    ids = [rng.permutation(N) for _ in names]                                            # keypoint j of image k shows scene row ids[k][j]
    fp = tmp_path / "features.h5"
    store = export.FeatureStore(fp)
    for name, v, idk in zip(names, views, ids):
        store.add(name, {"keypoints": v[idk], "descriptors": np.ascontiguousarray(base[idk].T.astype(np.float32)), "scores": np.ones(N, np.float32),
                         "tile_idx": np.zeros(N, np.float32), "image_size": np.array((1024, 1024))})
    store.close()
    general = {"geom_verification": "MAGSAC", "gv_threshold": 1.5, "quality": "HIGH", "min_inliers_per_pair": 15, "min_inlier_ratio_per_pair": 0.25}
    mt = plugins.KorniaMatcher({"general": general, "matcher": {"name": "kornia_matcher", "match_mode": "mnn", "th": 0.8}})
    shim = bm.BatchedImageMatcher(types.SimpleNamespace(_device="cuda", _lib=hip_lib), mt, tmp_path, pair_batch=2, gv_iters=ITERS)
    pairs = [("a.jpg", "b.jpg"), ("a.jpg", "c.jpg"), ("b.jpg", "c.jpg")]
    mp = shim.match_pairs(fp, pairs)
    assert mt._net_b.nk > 4096
    raw, ver = export.MatchStore.read_all(tmp_path / "raw_matches.h5"), export.MatchStore.read_all(mp)
    for k, (a, b) in enumerate(pairs):
        ia, ib = ids[names.index(a)], ids[names.index(b)]
        inv_b = np.argsort(ib)
        assert np.array_equal(raw[(a, b)], np.stack([np.arange(N), inv_b[ia]], 1))        # every keypoint finds its copy: 4200 raw matches
        fa, fb = export.FeatureStore.read(fp, a), export.FeatureStore.read(fp, b)
        r = raw[(a, b)]
        _, mask, cnt, _ = geom_ref.fundamental_ransac(fa["keypoints"][r[:, 0]], fb["keypoints"][r[:, 1]], 1.5, iters=ITERS, seed=0, pair=k % 2)
        want = verify.apply_reference_filters(r, mask, 15, 0.25)
        assert want is not None and len(want) >= 2500
        got = ver[(a, b)]
        diff = set(map(tuple, got)) ^ set(map(tuple, want))
        print(f"{a} {b}: raw {len(r)} oracle inliers {cnt} written {len(got)} differing rows {len(diff)}")
        assert len(diff) <= 2 and abs(len(got) - len(want)) <= 2


def test_per_tile_verification_on_device_tables(hip_lib):
    """tile_matching.match_tile_pairs_batched_device with a verifier, on the case of tests/test_tile_verify_emu.py: the scene's tile pair keeps
    its inliers, the 10-match and the random tile pairs contribute nothing; without a verifier every match comes back."""
    from tests import tile_verify_cases as tc
    plugins = importlib.import_module("deep-image-matching_amd.plugins")
    tm = importlib.import_module("deep-image-matching_amd.tile_matching")
    verify = importlib.import_module("deep-image-matching_amd.verify")
    f0, f1, expected, unverified = tc.case()
    m = plugins.KorniaMatcher({"general": {"tile_size": (64, 64), "tile_overlap": 0}, "matcher": {"name": "kornia_matcher", "match_mode": "mnn", "th": 0.8}})
    v = verify.DeviceVerifier(threshold=tc.THRESHOLD, iters=tc.ITERS, error_type="sampson", seed=tc.SEED)
    d0, d1 = tc.device_features(f0, "cuda"), tc.device_features(f1, "cuda")
    got = tm.match_tile_pairs_batched_device(m._ensure_pairs, d0, d1, tc.TILE_PAIRS, verifier=v)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), expected)
    assert np.array_equal(tm.match_tile_pairs_batched_device(m._ensure_pairs, d0, d1, tc.TILE_PAIRS).cpu().numpy(), unverified)
