"""Functional restatement of the reference's XFeat sparse path in plain torch: XFeat.detectAndCompute (thirdparty/accelerated_features/modules/
xfeat.py:50-103 = XFM) over XFeatModel.forward (modules/model.py:123-154 = XFN) and InterpolateSparse2d (modules/interpolator.py:17-33 = XFI),
as driven by extractors/xfeat.py.  Takes a plain state dict; scripts/make_xfeat_golden.py asserts that it equals the reference modules bit for
bit where the goldens are made.  ``dtype=torch.float64`` evaluates the same graph in double precision (the yardstick of the error bounds).
"""
from __future__ import annotations

import importlib

import numpy as np
import torch
import torch.nn.functional as F

weights_mod = importlib.import_module("deep-image-matching_amd.weights")
STRIDE = {p: s for p, _, _, _, s in weights_mod.XFEAT_BASIC}
KERNEL = {p: k for p, _, _, k, _ in weights_mod.XFEAT_BASIC}


def _basic(x, sd, p):
    """BasicLayer (XFN:12-25): bias-free convolution, BatchNorm2d(affine=False) in eval mode, ReLU."""
    x = F.conv2d(x, sd[p + ".layer.0.weight"], None, stride=STRIDE[p], padding=KERNEL[p] // 2)
    x = F.batch_norm(x, sd[p + ".layer.1.running_mean"], sd[p + ".layer.1.running_var"], None, None, False, 0.1, 1e-5)
    return F.relu(x)


def _chain(x, sd, block, n):
    for i in range(n):
        x = _basic(x, sd, f"{block}.{i}")
    return x


def preprocess(image, dtype=torch.float32):
    """XFM:219-240: (H, W) / (H, W, C) array -> [1][C][_H][_W] resized to multiples of 32, and the scale factors (rh, rw) as Python floats."""
    x = torch.as_tensor(np.asarray(image))
    x = (x[..., None] if x.dim() == 2 else x).permute(2, 0, 1)[None].float().to(dtype)
    H, W = x.shape[-2:]
    _H, _W = (H // 32) * 32, (W // 32) * 32
    return F.interpolate(x, (_H, _W), mode="bilinear", align_corners=False), H / _H, W / _W


def network(x, sd):
    """XFN:123-154 on the resized frame: (feats [B,64,H/8,W/8], keypoint logits [B,65,H/8,W/8], reliability [B,1,H/8,W/8], normalised image)."""
    x = x.mean(dim=1, keepdim=True)
    x = F.instance_norm(x, eps=1e-5)
    x1 = _chain(x, sd, "block1", 4)
    skip = F.conv2d(F.avg_pool2d(x, 4, stride=4), sd["skip1.1.weight"], sd["skip1.1.bias"])
    x2 = _chain(x1 + skip, sd, "block2", 2)
    x3 = _chain(x2, sd, "block3", 3)
    x4 = _chain(x3, sd, "block4", 3)
    x5 = _chain(x4, sd, "block5", 4)
    x4 = F.interpolate(x4, x3.shape[-2:], mode="bilinear")
    x5 = F.interpolate(x5, x3.shape[-2:], mode="bilinear")
    f = _chain(x3 + x4 + x5, sd, "block_fusion", 2)
    feats = F.conv2d(f, sd["block_fusion.2.weight"], sd["block_fusion.2.bias"])
    h = _chain(feats, sd, "heatmap_head", 2)
    heat = torch.sigmoid(F.conv2d(h, sd["heatmap_head.2.weight"], sd["heatmap_head.2.bias"]))
    B, C, H, W = x.shape
    u = x.unfold(2, 8, 8).unfold(3, 8, 8).reshape(B, C, H // 8, W // 8, 64).permute(0, 1, 4, 2, 3).reshape(B, -1, H // 8, W // 8)   # XFN:113-120
    k = _chain(u, sd, "keypoint_head", 3)
    logits = F.conv2d(k, sd["keypoint_head.3.weight"], sd["keypoint_head.3.bias"])
    return feats, logits, heat, x


def kpts_heatmap(logits):
    """XFM:242-247: softmax over the 65 channels, dustbin dropped, cell-major depth-to-space."""
    s = F.softmax(logits * 1.0, 1)[:, :64]
    B, _, H, W = s.shape
    return s.permute(0, 2, 3, 1).reshape(B, H, W, 8, 8).permute(0, 1, 3, 2, 4).reshape(B, 1, H * 8, W * 8)


def nms(x, threshold=0.05, kernel_size=5):
    """XFM:249-263: ONE max-pool pass; row-major (x, y) positions padded with (0, 0) rows to the batch's longest list."""
    B = x.shape[0]
    local_max = F.max_pool2d(x, kernel_size=kernel_size, stride=1, padding=kernel_size // 2)
    pos = (x == local_max) & (x > threshold)
    lists = [k.nonzero()[..., 1:].flip(-1) for k in pos]
    out = torch.zeros((B, max(len(p) for p in lists), 2), dtype=torch.long)
    for b, p in enumerate(lists):
        out[b, :len(p)] = p
    return out


def sample(x, pos, H, W, mode):
    """XFI:17-33: grid = 2 * pos / (W - 1, H - 1) - 1 with the FULL-resolution sizes, grid_sample(align_corners=False), zero padding."""
    grid = (2.0 * (pos / torch.tensor([W - 1, H - 1], dtype=pos.dtype)) - 1.0).unsqueeze(-2).to(x.dtype)
    return F.grid_sample(x, grid, mode=mode, align_corners=False).permute(0, 2, 3, 1).squeeze(-2)


def select(K1h, H1, top_k, threshold=0.05):
    """XFM:74-87 on given maps K1h [B,1,H,W], H1 [B,1,H/8,W/8]: (positions [B,n,2] long, scores [B,n]), sorted, cut at top_k, padding rows included."""
    _H, _W = K1h.shape[-2:]
    mk = nms(K1h, threshold=threshold, kernel_size=5)
    posf = mk.to(torch.float32)   # (integer positions divided by a float tensor are float32 in the reference: XFI:19)
    scores = (sample(K1h, posf, _H, _W, "nearest") * sample(H1, posf, _H, _W, "bilinear")).squeeze(-1)
    scores[torch.all(mk == 0, dim=-1)] = -1
    idxs = torch.argsort(-scores)
    mk = torch.stack([torch.gather(mk[..., 0], -1, idxs)[:, :top_k], torch.gather(mk[..., 1], -1, idxs)[:, :top_k]], dim=-1)
    return mk, torch.gather(scores, -1, idxs)[:, :top_k]


@torch.no_grad()
def xfeat_forward(image, sd, top_k=4096, threshold=0.05, taps=False, dtype=torch.float32):
    """detectAndCompute on one image (H x W or H x W x C array, any scale).  Returns keypoints [n,2], scores [n], descriptors [n,64] (rows: XFM
    hands them out untransposed) and, with taps, K1h / H1 / M1 / the normalised image / the candidate positions before the cut."""
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    x, rh, rw = preprocess(image, dtype)
    _H, _W = x.shape[-2:]
    M1, K1, H1, xn = network(x, sd)
    M1 = F.normalize(M1, dim=1)
    K1h = kpts_heatmap(K1)
    mk, scores = select(K1h, H1, top_k, threshold)
    feats = F.normalize(sample(M1, mk.to(torch.float32), _H, _W, "bicubic"), dim=-1)
    kp = mk * torch.tensor([rw, rh]).view(1, 1, -1)
    valid = scores > 0
    out = {"keypoints": kp[0][valid[0]], "scores": scores[0][valid[0]], "descriptors": feats[0][valid[0]]}
    if taps:
        out.update(K1h=K1h[0, 0], H1=H1[0, 0], M1=M1[0], norm=xn[0, 0], pixels=mk[0][valid[0]], hw=(_H, _W))
    return out
