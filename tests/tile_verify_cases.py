"""Shared inputs of the per-tile verification tests (CPU emulator and GPU): two tiled feature sets whose tile-pair match lists are known
(one-hot descriptors, permuted, matched by the nearest-neighbour matcher in mnn mode), and the expected result from the numpy oracle."""
import functools

import numpy as np

from oracle import geom_ref

D = 64
THRESHOLD, ITERS, SEED, MIN_INLIERS = 4.0, 2048, 0, 15
TILE_PAIRS = [(0, 0), (1, 1), (2, 2)]
HW = (64, 192)          # three 64 x 64 tiles in a row: the GRID selection is TILE_PAIRS


def _correspondences():
    rng = np.random.default_rng(7)
    a0, a1, _, _ = geom_ref.synthetic_two_view(40, 20, seed=31, noise_px=0.3)                       # tile pair 0: 40 inliers + 20 random outliers
    b0, b1, _, _ = geom_ref.synthetic_two_view(10, 0, seed=32, noise_px=0.0)                        # tile pair 1: 10 perfect inliers
    c0, c1 = (rng.uniform(0, 1024, (30, 2)).astype(np.float32) for _ in range(2))                   # tile pair 2: 30 random correspondences
    return [(a0, a1), (b0, b1), (c0, c1)]


@functools.lru_cache(maxsize=None)
def case():
    """-> (features0, features1, expected rows with per-tile verification, expected rows without).  Keypoint i of tile t in image 0 matches keypoint perm_t[i] of tile t in image 1; the merged
    tables interleave the tiles, so the tile-local index differs from the index in the image's table."""
    rng = np.random.default_rng(3)
    corr = _correspondences()
    n_tot = sum(len(c[0]) for c in corr)
    order0, order1 = rng.permutation(n_tot), rng.permutation(n_tot)        # position in the merged table of each (tile, local) keypoint
    k0, k1 = np.zeros((n_tot, 2), np.float32), np.zeros((n_tot, 2), np.float32)
    d0, d1 = np.zeros((D, n_tot), np.float32), np.zeros((D, n_tot), np.float32)
    t0, t1 = np.zeros(n_tot, np.float32), np.zeros(n_tot, np.float32)
    expected, raw, base = [], [], 0
    for t, (x0, x1) in enumerate(corr):
        n = len(x0)
        assert n <= D
        # get_features_by_tile keeps the table order: local index = rank of the table position among the tile's keypoints
        pos0, pos1 = np.sort(order0[base:base + n]), np.sort(order1[base:base + n])
        perm = rng.permutation(n)
        for i in range(n):
            k0[pos0[i]], t0[pos0[i]], d0[i, pos0[i]] = x0[i], t, 1.0
            k1[pos1[perm[i]]], t1[pos1[perm[i]]], d1[i, pos1[perm[i]]] = x1[i], t, 1.0
        # the matcher lists a tile pair's matches by ascending local index of image 0: (i, perm[i]), i.e. the order of x0 / x1
        _, mask, _, _ = geom_ref.fundamental_ransac(x0, x1, THRESHOLD, iters=ITERS, seed=SEED, pair=t)
        if len(x0) < 8:
            mask = np.ones(len(x0), bool)
        raw.append(np.stack([pos0, pos1[perm]], 1))
        if mask.sum() >= MIN_INLIERS:
            expected.append(np.stack([pos0[np.arange(n)[mask]], pos1[perm[mask]]], 1))
        base += n
    assert len(expected) == 1 and len(expected[0]) >= 36        # the scene keeps its inliers, the other two tile pairs contribute nothing
    exp = np.unique(np.vstack(expected).astype(np.int64), axis=0)
    f0 = {"keypoints": k0, "descriptors": d0, "scores": np.ones(n_tot, np.float32), "tile_idx": t0, "image_size": np.array(HW, np.int32)}
    f1 = {"keypoints": k1, "descriptors": d1, "scores": np.ones(n_tot, np.float32), "tile_idx": t1, "image_size": np.array(HW, np.int32)}
    return f0, f1, exp, np.unique(np.vstack(raw).astype(np.int64), axis=0)


def device_features(f, device):
    import torch
    return {"keypoints": torch.from_numpy(f["keypoints"]).to(device).contiguous(),
            "descriptors_nd": torch.from_numpy(np.ascontiguousarray(f["descriptors"].T)).to(device),
            "tile_idx": torch.from_numpy(f["tile_idx"]).to(device).contiguous(), "image_size": f["image_size"]}
