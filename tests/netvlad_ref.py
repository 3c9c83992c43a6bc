"""Functional restatement of the reference's NetVLAD (thirdparty/hloc/extractors/netvlad.py = NV) on a state dict, in any dtype.

scripts/make_netvlad_golden.py asserts that this equals the reference MODULE bit for bit in fp32; the tests use the fp64 evaluation as the
yardstick every fp32 result (the module's and the device's) is measured against.  Torch on the CPU, nothing native."""
from __future__ import annotations

import importlib

import torch
import torch.nn.functional as F

weights_mod = importlib.import_module("deep-image-matching_amd.weights")

POOL_AFTER = (2, 7, 14, 21)   # features[4], [9], [16], [23] of torchvision's VGG16; features[:-2] drops the last ReLU and pool (NV:66-68)


def backbone(image: torch.Tensor, sd, dtype) -> torch.Tensor:
    """image [B,3,H,W] in 0..1 -> the conv5_3 map [B,512,h,w] (NV:126-133)."""
    mean = sd["preprocess.mean"].to(dtype)[None, :, None, None]
    unit_std = torch.ones(1, 3, 1, 1, dtype=dtype)
    t = (image.to(dtype) * 255).clamp(min=0.0, max=255.0)        # NV:126: the 0..255 range the network was trained on
    t = (t - mean) / unit_std                                     # NV:129-130: per-channel mean, std 1 (the division is kept: it is an fp operation)
    convs = weights_mod.NETVLAD_CONVS
    for pos, (i, _co, _ci) in enumerate(convs):
        t = F.conv2d(t, sd[f"backbone.{i}.weight"].to(dtype), sd[f"backbone.{i}.bias"].to(dtype), padding=1)
        if pos + 1 < len(convs):
            t = t.relu()
        if i in POOL_AFTER:
            t = F.max_pool2d(t, 2, 2)                             # floor semantics
    return t


def _unit(t: torch.Tensor, dim: int) -> torch.Tensor:
    """t / max(||t||_2, 1e-12) along dim: F.normalize's definition (and its kernel, so that fp32 agrees with the module bit for bit)."""
    return F.normalize(t, p=2.0, dim=dim, eps=1e-12)


def head(fmap_bdn: torch.Tensor, score_w: torch.Tensor, centers: torch.Tensor) -> torch.Tensor:
    """[B,512,n] -> [B,512 K]: per-location normalisation (NV:138), then the NetVLAD layer (NV:28-39): soft assignment = softmax over the K scores of
    a location (NV:30-31); residual of every location to every centre, weighted by the assignment and summed over the locations (NV:32-33);
    every cluster's 512-vector normalised (NV:36); flattened with the cluster index fastest and normalised as a whole (NV:37-38)."""
    xhat = _unit(fmap_bdn, 1)                                      # [B, D, n]
    assign = F.conv1d(xhat, score_w).softmax(dim=1)                # [B, K, n]
    residual = xhat[:, :, None, :] - centers[None, :, :, None]     # [B, D, K, n]
    vlad = (assign[:, None, :, :] * residual).sum(dim=3)           # [B, D, K]
    vlad = _unit(vlad, 1)
    return _unit(vlad.reshape(vlad.shape[0], -1), 1)


def whiten(v: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    return _unit(F.linear(v, weight, bias), 1)                     # NV:143-144


@torch.no_grad()
def netvlad_forward(image: torch.Tensor, sd, dtype=torch.float32) -> torch.Tensor:
    """image [B,3,H,W] in 0..1 -> the global descriptor [B, whiten_out or 512 K] (NV:122-146)."""
    fmap = backbone(image, sd, dtype)
    v = head(fmap.flatten(2), sd["netvlad.score_proj.weight"].to(dtype), sd["netvlad.centers"].to(dtype))
    if "whiten.weight" in sd:
        v = whiten(v, sd["whiten.weight"].to(dtype), sd["whiten.bias"].to(dtype))
    return v
