"""Pure-torch restatement of RIPE's inference path (vgg_hyper(): RIPE(VGG(mode="dect", InstanceNorm), HyperColumnFeatures, Conv1d(960, 256))) on a
state dict with the reference's own keys, in any dtype.  scripts/make_ripe_golden.py asserts that it equals the reference module bit for bit in
fp32; the tests evaluate it in fp64 as the yardstick.  Test-only: the package never imports it."""
from __future__ import annotations

import torch
import torch.nn.functional as F

ENCODER_CONVS = (0, 3, 7, 10, 14, 17, 20, 23, 27, 30, 33, 36)   # vgg19_bn().features: BatchNorm at + 1, ReLU at + 2
ENCODER_POOLS = (6, 13, 26, 39)
SCALES = ("8", "4", "2", "1")
EPS = 1e-5


def _bn(x, sd, p):
    return F.batch_norm(x, sd[f"{p}.running_mean"], sd[f"{p}.running_var"], sd[f"{p}.weight"], sd[f"{p}.bias"], False, 0.1, EPS)


def _cast(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def encoder(x, sd):
    """features[:40] of vgg19_bn: the maps in front of the four pools."""
    feats = []
    for i in range(40):
        if i in ENCODER_POOLS:
            feats.append(x)
            if i == 39:
                break   # the fourth pool's output is never used
            x = F.max_pool2d(x, 2, 2)
        elif i in ENCODER_CONVS:
            p = "net.encoder.layers"
            x = F.relu(_bn(F.conv2d(x, sd[f"{p}.{i}.weight"], sd[f"{p}.{i}.bias"], padding=1), sd, f"{p}.{i + 1}"))
    return feats


def refiner(x, sd, scale):
    p = f"net.decoder.layers.{scale}"
    x0 = F.relu(_bn(F.conv2d(x, sd[f"{p}.block1.0.weight"], sd[f"{p}.block1.0.bias"]), sd, f"{p}.block1.1"))
    x0 = F.conv2d(x0, sd[f"{p}.block1.3.weight"], sd[f"{p}.block1.3.bias"])
    x = x0
    for j in range(8):
        q = f"{p}.hidden_blocks.{j}"
        w = sd[f"{q}.0.weight"]
        x = F.relu(_bn(F.conv2d(x, w, sd[f"{q}.0.bias"], padding=2, groups=w.shape[0]), sd, f"{q}.1"))
        x = F.conv2d(x, sd[f"{q}.3.weight"], sd[f"{q}.3.bias"])
    x = (x + x0) / 1.4
    return F.conv2d(x, sd[f"{p}.out_conv.weight"], sd[f"{p}.out_conv.bias"])


def heat_map(img, sd, dtype=torch.float32):
    """img [1, 3, H, W] (or [1, 1, H, W]) in 0..1 -> (heat [H, W], the four encoder maps [1, C, h, w]) in ``dtype``."""
    sd = _cast(sd, dtype)
    x = img.to(dtype)
    if x.shape[1] == 1:
        x = x.repeat(1, 3, 1, 1)
    x = F.instance_norm(x, eps=EPS)
    feats = encoder(x, sd)
    output, context = 0, None
    for idx, (f, scale) in enumerate(zip(reversed(feats), SCALES)):
        stuff = refiner(f if context is None else torch.cat((f, context), dim=1), sd, scale)
        output = output + stuff[:, :1]
        context = stuff[:, 1:]
        if idx < 3:
            size = feats[-(idx + 2)].shape[-2:]
            output = F.interpolate(output, size=size, mode="bilinear", align_corners=False)
            context = F.interpolate(context, size=size, mode="bilinear", align_corners=False)
    return output[0, 0], feats


def nms(heat, threshold):
    """(x, y) int64 rows of the pixels that equal their 3 x 3 maximum and exceed the threshold, in row-major order."""
    x = heat[None]
    local_max = F.max_pool2d(x, kernel_size=3, stride=1, padding=1)
    pos = (x == local_max) & (x > threshold)
    return pos.nonzero()[..., 1:].flip(-1)


def hypercolumns(feats, kpts, H, W):
    """kpts [N, 2] int64 (x, y) -> [N, 960]."""
    dtype = feats[0].dtype   # (the module divides int64 by int64: a float32 true division, the same values as this in fp32)
    grid = (2.0 * (kpts[None].to(dtype) / torch.tensor([W - 1, H - 1], dtype=dtype)) - 1.0).unsqueeze(-2)
    rows = [F.grid_sample(f, grid, mode="bilinear", align_corners=True).permute(0, 2, 3, 1).squeeze(-2) for f in feats]
    return torch.cat(rows, dim=-1)[0]


def describe(feats, kpts, H, W, sd):
    rows = hypercolumns(feats, kpts, H, W)
    d = F.conv1d(rows.t()[None], sd["conv_dim_reduction_coarse_desc.weight"].to(rows.dtype), sd["conv_dim_reduction_coarse_desc.bias"].to(rows.dtype))
    return F.normalize(d.permute(0, 2, 1), dim=2)[0]


def ripe_forward(img, sd, dtype=torch.float32, threshold=0.5, top_k=2048):
    """detectAndCompute: {"heat" [H, W], "features", "keypoints" [N, 2] float (x, y), "descriptors" [N, 256], "scores" [N]} in score-descending order."""
    heat, feats = heat_map(img, sd, dtype)
    H, W = heat.shape
    xy = nms(heat, threshold)
    scores = heat[xy[:, 1], xy[:, 0]]
    xy = xy[torch.argsort(-scores)[:top_k]]
    if xy.shape[0] == 0:
        raise RuntimeError("No keypoints detected")
    descs = describe(feats, xy, H, W, sd)
    scores = heat[xy[:, 1], xy[:, 0]]
    scores = scores / heat.max()
    order = torch.argsort(-scores)
    return {"heat": heat, "features": feats, "keypoints": xy[order].to(dtype), "descriptors": descs[order], "scores": scores[order]}
