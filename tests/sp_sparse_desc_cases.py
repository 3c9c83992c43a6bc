"""Shared by the emulator and the GPU tests of SuperPoint's sparse descriptor head (tests/test_sp_sparse_desc_emu.py, tests/test_sp_sparse_desc_gpu.py).
Every case takes (lib, device): the emulator build with "cpu", or the gfx950 library with "cuda".

dim_tune_set key 20 selects the head: 0 = convDa / convDb on the whole map, 2 = on the cells that the keypoints sample, 1 = the rule of
sp_api.hip (sparse when min(4 capacity, h w) <= 0.8 h w and max_keypoints > 0).  Per cell the sparse kernels run the dense kernels' arithmetic, so
every case asserts that keypoints, scores, descriptors and counts of the forced-sparse run are BIT-IDENTICAL to the forced-dense run of the same
handle, that the fp16x3 range-guard counters agree, and that the device's row count equals the number of distinct in-map corner cells of the
returned keypoints (computed here in numpy with the samplers' formulas of oracle/superpoint_ref.py), and that the dense descriptor tap of
dim_sp_debug_buffers is the same map after either run.  Descriptors of dim_sp_create handles are also
held to the oracle through tests.parity.compare_superpoint: its default descriptor tolerance (1e-3) is the one tests/test_superpoint_gpu.py uses.
The open network has no oracle under oracle/: its dense path is pinned to the reference's goldens by tests/spopen_cases.py, and the sparse path
to the dense one here.
"""
from __future__ import annotations

import importlib

import numpy as np
import torch

from oracle import superpoint_ref
from tests.parity import compare_superpoint

sp_mod = importlib.import_module("deep-image-matching_amd.superpoint_hip")
capi = importlib.import_module("deep-image-matching_amd.capi")
weights_mod = importlib.import_module("deep-image-matching_amd.weights")

DENSE, AUTO, SPARSE = 0, 1, 2


def run(net, x, mode):
    """One extract_batch under dim_tune_set(20, mode): (kpts, scores, desc, n) on the CPU, net.desc_rows(), the range-guard total and sites."""
    lib = net.lib
    x = x.contiguous().to(net.device)
    try:
        capi.check(lib, lib.dim_tune_set(20, mode))
        capi.check(lib, lib.dim_saturation_reset(net._stream()))
        out = [t.cpu().clone() for t in net.extract_batch(x)]
        rows = net.desc_rows(x.shape[0])
        total, sites = capi.saturation(lib, net._stream(), reset=True)
    finally:
        lib.dim_tune_set(20, AUTO)
    return out, rows, total, sites


def corner_cells(kpts: np.ndarray, h: int, w: int, fix_sampling: bool) -> set:
    """Distinct cells inside the [h][w] map among the four bilinear corners of every keypoint (float32 arithmetic, the samplers' formulas)."""
    f = np.float32
    kx, ky = kpts[:, 0].astype(f), kpts[:, 1].astype(f)
    if fix_sampling:   # (k + 0.5) / (8 w), align_corners=False
        gx, gy = (kx + f(0.5)) / (f(w) * f(8)), (ky + f(0.5)) / (f(h) * f(8))
        gx, gy = gx * f(2) - f(1), gy * f(2) - f(1)
        ix, iy = ((gx + f(1)) * f(w) - f(1)) / f(2), ((gy + f(1)) * f(h) - f(1)) / f(2)
    else:              # (k - 4 + 0.5) / (8 w - 4 - 0.5), align_corners=True
        gx, gy = (kx - f(4) + f(0.5)) / (f(w * 8) - f(4) - f(0.5)), (ky - f(4) + f(0.5)) / (f(h * 8) - f(4) - f(0.5))
        gx, gy = gx * f(2) - f(1), gy * f(2) - f(1)
        ix, iy = ((gx + f(1)) / f(2)) * f(w - 1), ((gy + f(1)) / f(2)) * f(h - 1)
    x0, y0 = np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)
    cells, outside = set(), 0
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        cx, cy = x0 + dx, y0 + dy
        ok = (cx >= 0) & (cx < w) & (cy >= 0) & (cy < h)
        outside += int((~ok).sum())
        cells.update((cy[ok] * w + cx[ok]).tolist())
    return cells, outside


def check_pair(net, x, fix_sampling, label, expect_auto=None):
    """Forced dense vs forced sparse on one handle and one batch; returns the dense outputs, the sparse row counts and the corners outside the map."""
    B, H, W = x.shape
    h, w = H // 8, W // 8
    (kd, sd, dd, nd), rows_d, sat_d, sites_d = run(net, x, DENSE)
    map_d = net.debug_taps(B)["dense_desc"]
    (ks, ss, ds, ns), rows_s, sat_s, sites_s = run(net, x, SPARSE)
    map_s = net.debug_taps(B)["dense_desc"]     # the sparse head stored rows only: dim_sp_debug_buffers rebuilds the map
    assert map_d.shape == (B, h, w, 256) and torch.equal(map_d, map_s), (label, "the dense descriptor tap after a sparse extract")
    assert rows_d is None, "key 20 = 0 did not run the dense head"
    assert rows_s is not None, "key 20 = 2 did not run the sparse head"
    slots, n_rows = rows_s
    assert slots == min(4 * net.capacity, h * w)
    assert torch.equal(nd, ns), (label, nd, ns)
    assert (sat_d, sites_d) == (sat_s, sites_s), (label, sites_d, sites_s)
    outside = 0
    for b in range(B):
        k = int(nd[b])
        assert torch.equal(kd[b, :k], ks[b, :k]) and torch.equal(sd[b, :k], ss[b, :k]), (label, b)
        diff = (dd[b, :k] - ds[b, :k]).abs().max().item() if k else 0.0
        print(f"sparse desc {label} image {b}: {k} keypoints, {int(n_rows[b])} of {h * w} cells, max |dense - sparse| descriptor difference {diff:.3e}")
        assert torch.equal(dd[b, :k], ds[b, :k]), (label, b, diff)
        cells, out_b = corner_cells(kd[b, :k].numpy(), h, w, fix_sampling)
        outside += out_b
        assert int(n_rows[b]) == len(cells), (label, b, int(n_rows[b]), len(cells))
    if expect_auto is not None:
        (ka, sa, da, na), rows_a, _, _ = run(net, x, AUTO)
        assert (rows_a is not None) == expect_auto, (label, "the selection rule", rows_a)
        assert torch.equal(na, nd) and all(torch.equal(da[b, : int(nd[b])], dd[b, : int(nd[b])]) for b in range(B))
    return (kd, sd, dd, nd), n_rows, outside


def against_oracle(out, x, sd, cfg, fix_sampling):
    kd, sc, dd, nd = out
    for b in range(x.shape[0]):
        k = int(nd[b])
        ref = superpoint_ref.superpoint_forward(x[b][None, None], sd, {**cfg, "fix_sampling": fix_sampling})
        compare_superpoint({"keypoints": kd[b, :k], "scores": sc[b, :k], "descriptors": dd[b, :k].t()}, ref)


# ---- 1. batch 3 of 72 x 88 (9 x 11 cells), capacity 32, remove_borders 0, one image without keypoints ---------------------------------------
def ragged_images() -> torch.Tensor:
    """[3, 72, 88]: noise confined to the first and last 8 pixel rows (black between them), noise everywhere, black.  On the seeded weights the
    detector scores the black image below 0.017, the strongest 32 maxima of the banded image above 0.046 with some of them in its first and last four
    pixel rows (the convolutions' zero padding keeps the edge ROWS of a full noise image out of its strongest 32), and full noise above 0.15 with
    maxima in the first and last four pixel columns: the threshold 0.03 leaves the black image without keypoints and gives both axes keypoints whose
    corners fall outside the map (asserted by ragged_batch)."""
    x = torch.zeros(3, 72, 88)
    band = torch.rand(72, 88, generator=torch.Generator().manual_seed(3))
    x[0, :8], x[0, 64:] = band[:8], band[64:]
    x[1] = torch.rand(3, 72, 88, generator=torch.Generator().manual_seed(0))[1]
    return x


def ragged_batch(lib, device, fix_sampling):
    sd = weights_mod.synthetic_superpoint_state_dict(1234)
    cfg = {"nms_radius": 1, "keypoint_threshold": 0.03, "max_keypoints": 32, "remove_borders": 0, "fix_sampling": bool(fix_sampling)}
    x = ragged_images()
    net = sp_mod.SuperPointHIP(sd, cfg, max_batch=3, max_hw=(72, 88), capacity=32, device=device, lib=lib)
    out, n_rows, outside = check_pair(net, x, bool(fix_sampling), f"72x88 fix_sampling={fix_sampling} {device}")
    kd, _, _, nd = out
    assert int(nd[2]) == 0 and int(n_rows[2]) == 0, "the black image has keypoints: no workgroup-exits-at-once case"
    assert int(nd[0]) > 0 and int(nd[1]) > 0
    k = torch.cat([kd[b, : int(nd[b])] for b in range(2)])
    assert bool((k[:, 0] < 4).any()) and bool((k[:, 0] >= 84).any()) and bool((k[:, 1] < 4).any()) and bool((k[:, 1] >= 68).any()), "no keypoints at the image edges"
    assert outside > 0, "no corner fell outside the map"
    against_oracle(out, x, sd, cfg, bool(fix_sampling))


# ---- 2. batch 2 of 128 x 160 (16 x 20 cells): capacity 64 -> the rule picks sparse (256 <= 0.8 x 320), capacity 512 -> dense (320 slots) --------
def selection_rule(lib, device, open_net, capacity):
    g = torch.Generator().manual_seed(3)
    x = torch.rand(2, 128, 160, generator=g)
    cfg = {"nms_radius": 2, "keypoint_threshold": 0.0005, "max_keypoints": capacity, "remove_borders": 4}
    if open_net:
        sd = weights_mod.synthetic_superpoint_open_state_dict(4321)
        net = sp_mod.SuperPointOpenHIP(sd, cfg, max_batch=2, max_hw=(128, 160), capacity=capacity, device=device, lib=lib)
    else:
        sd = weights_mod.synthetic_superpoint_state_dict(1234)
        net = sp_mod.SuperPointHIP(sd, cfg, max_batch=2, max_hw=(128, 160), capacity=capacity, device=device, lib=lib)
    out, n_rows, _ = check_pair(net, x, bool(net.cfg["fix_sampling"]), f"128x160 open={open_net} capacity={capacity} {device}", expect_auto=capacity == 64)
    assert int(out[3].min()) > 16
    if not open_net:
        against_oracle(out, x, sd, cfg, False)


# ---- 3. one 256 x 256 image, every keypoint inside a 24 x 24 pixel window (three cells across): many keypoints per cell ---------------------------
def cluster(lib, device):
    sd = weights_mod.synthetic_superpoint_state_dict(1234)
    cfg = {"nms_radius": 1, "keypoint_threshold": 0.0, "max_keypoints": 64, "remove_borders": 116}   # candidates: 116 <= x, y < 140
    x = torch.rand(1, 256, 256, generator=torch.Generator().manual_seed(7))
    net = sp_mod.SuperPointHIP(sd, cfg, max_batch=1, max_hw=(256, 256), capacity=64, device=device, lib=lib)
    out, n_rows, _ = check_pair(net, x, False, f"256x256 cluster {device}")
    n = int(out[3][0])
    assert n == 64 and int(n_rows[0]) <= 25, (n, int(n_rows[0]))    # 4 n = 256 corners on at most 5 x 5 cells
    against_oracle(out, x, sd, cfg, False)
