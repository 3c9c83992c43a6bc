"""Weights for the SuperPoint / LightGlue hot path.

The official checkpoints (``superpoint_v1.pth``, ``superpoint_lightglue.pth``) are
downloaded by the reference at run time (SPN:110,147-150; LGN:327-328,381-396) and
are not available offline, so this module provides

* ``load_superpoint_state_dict`` / ``load_lightglue_state_dict`` — accept the official
  files unchanged when a path is given (incl. LightGlue's legacy key rename,
  LGN:389-396), and
* seeded synthetic state dicts in exactly the official key/shape layout
   for tests, smoke and the synthetic benchmark.  They are
  drawn from ``torch.Generator`` streams so that the same seed gives the same
  tensors here, in the golden-vector generator and on the GPU box.
"""
from __future__ import annotations

import math
from pathlib import Path
from typing import Dict, Optional

import torch

SP_LAYERS = [
    # name, cout, cin, k
    ("conv1a", 64, 1, 3), ("conv1b", 64, 64, 3),
    ("conv2a", 64, 64, 3), ("conv2b", 64, 64, 3),
    ("conv3a", 128, 64, 3), ("conv3b", 128, 128, 3),
    ("conv4a", 128, 128, 3), ("conv4b", 128, 128, 3),
    ("convPa", 256, 128, 3), ("convPb", 65, 256, 1),
    ("convDa", 256, 128, 3), ("convDb", 256, 256, 1),
]


def synthetic_superpoint_state_dict(seed: int = 1234) -> Dict[str, torch.Tensor]:
    """He-normal conv weights, small biases."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, co, ci, k in SP_LAYERS:
        fan_in = ci * k * k
        sd[f"{name}.weight"] = torch.randn(co, ci, k, k, generator=g) * math.sqrt(2.0 / fan_in)
        sd[f"{name}.bias"] = torch.randn(co, generator=g) * 0.01
    return sd


class MissingWeightsError(RuntimeError):
    """No checkpoint was given.  The reference downloads the official files (SPN:149, LGN:383); this container and the
    GPU boxes have no network, so a path is required — seeded synthetic weights are an explicit opt-in for tests and
    benchmarks (``allow_synthetic_weights``), never a silent default: features from random weights are garbage."""


def _no_weights(what: str, env: str, allow_synthetic: bool) -> None:
    if not allow_synthetic:
        raise MissingWeightsError(
            f"{what}: no checkpoint given - set '<section>.weights_path' (or the {env} environment variable) to the official file; "
            "pass 'allow_synthetic_weights: True' only for tests / synthetic benchmarks")


def load_superpoint_state_dict(path: str | None = None, seed: int = 1234, allow_synthetic: bool = False) -> Dict[str, torch.Tensor]:
    if path is None:
        _no_weights("SuperPoint (superpoint_v1.pth, SPN:149)", "DIM_SUPERPOINT_WEIGHTS", allow_synthetic)
        return synthetic_superpoint_state_dict(seed)
    sd = torch.load(str(Path(path)), map_location="cpu")
    missing = [f"{n}.{s}" for n, *_ in SP_LAYERS for s in ("weight", "bias") if f"{n}.{s}" not in sd]
    if missing:
        raise KeyError(f"SuperPoint checkpoint {path} lacks keys {missing}")
    return {k: v.float().contiguous() for k, v in sd.items()}


def lightglue_confidence_thresholds(n_layers: int = 9) -> torch.Tensor:
    """LGN:581-584: 0.8 + 0.1*exp(-4 i / L), clipped to [0, 1], stored as float32."""
    import numpy as np

    return torch.Tensor([float(np.clip(0.8 + 0.1 * np.exp(-4.0 * i / n_layers), 0, 1)) for i in range(n_layers)])


def synthetic_lightglue_state_dict(seed: int = 0, input_dim: int = 256, n_layers: int = 9, dim: int = 256,
                                   gain: float = 1.0, num_heads: int = 4) -> Dict[str, torch.Tensor]:
    """nn.Linear-style uniform init in the official key layout (LGN:361-378).

    ``gain`` > 1 sharpens the synthetic network (larger logits) so that softmaxes are
    not uniform and the mutual-NN stage has something to decide in tests."""
    g = torch.Generator().manual_seed(seed)

    def lin(out_f, in_f, bias=True, prefix=""):
        bound = gain / math.sqrt(in_f)
        d = {prefix + "weight": (torch.rand(out_f, in_f, generator=g) * 2 - 1) * bound}
        if bias:
            d[prefix + "bias"] = (torch.rand(out_f, generator=g) * 2 - 1) * bound
        return d

    sd: Dict[str, torch.Tensor] = {}
    sd["confidence_thresholds"] = lightglue_confidence_thresholds(n_layers)
    if input_dim != dim:
        sd.update(lin(dim, input_dim, prefix="input_proj."))
    sd["posenc.Wr.weight"] = torch.randn(dim // num_heads // 2, 2, generator=g)  # head_dim//2 x 2, std gamma^-2 = 1 (LGN:62-63)
    for i in range(n_layers):
        t = f"transformers.{i}."
        sd.update(lin(3 * dim, dim, prefix=t + "self_attn.Wqkv."))
        sd.update(lin(dim, dim, prefix=t + "self_attn.out_proj."))
        for blk in ("self_attn", "cross_attn"):
            sd.update(lin(2 * dim, 2 * dim, prefix=t + blk + ".ffn.0."))
            sd[t + blk + ".ffn.1.weight"] = 1.0 + 0.1 * torch.randn(2 * dim, generator=g)
            sd[t + blk + ".ffn.1.bias"] = 0.1 * torch.randn(2 * dim, generator=g)
            sd.update(lin(dim, 2 * dim, prefix=t + blk + ".ffn.3."))
        for nm in ("to_qk", "to_v", "to_out"):
            sd.update(lin(dim, dim, prefix=t + "cross_attn." + nm + "."))
        sd.update(lin(1, dim, prefix=f"log_assignment.{i}.matchability."))
        sd.update(lin(dim, dim, prefix=f"log_assignment.{i}.final_proj."))
        if i < n_layers - 1:
            sd.update(lin(1, dim, prefix=f"token_confidence.{i}.token.0."))
    return sd


def synthetic_lightglue_matching_state_dict(seed: int = 0, input_dim: int = 256, n_layers: int = 9, dim: int = 256,
                                            residual: float = 0.003, sharpness: float = 220.0, matchability_bias: float = 5.0,
                                            center: Optional[torch.Tensor] = None, whiten: Optional[torch.Tensor] = None,
                                            num_heads: int = 4) -> Dict[str, torch.Tensor]:
    """Seeded synthetic LightGlue weights (official key layout) that MATCH: the transformer blocks are near-identity (`ffn.3`
    scaled by ``residual``, so a keypoint's state stays close to its input descriptor), every `final_proj` is
    ``sharpness`` x (identity - ``center``) (an orthogonal map: the similarity is sharpness^2 / 16 x the inner product of the CENTRED
    descriptors, which a random `final_proj` does not preserve; ``center`` = the mean descriptor of the workload, passed as
    `final_proj.bias` = -sharpness x center — the seeded SuperPoint's descriptors have a pairwise cosine of 0.98, so without centring
    the logits would have to be ~6000 to separate them and the REFERENCE's own fp32 evaluation of the matching scores would carry
    1e-3 of noise) and the matchability heads say "matchable".  On two views that share keypoints with equal
    descriptors (workloads.shifted_crops) the mutual-NN assignment then returns the true correspondences — several hundred
    matches per pair with scores above the reference's default threshold 0.1 — so that verification, the match writers and the
    multi-GPU match gather of the benchmarks carry real work.  Same arithmetic, same FLOPs as any other weights.
    ``whiten`` ([dim, dim], symmetric; ``descriptor_whitening``): `final_proj` = sharpness x whiten x (x - center) instead of the scaled identity.
    DIFFERENT photographs share no equal descriptors, and in the plain centred dot product a few long descriptors are everyone's nearest
    neighbour (20 - 41 mutual nearest neighbours among 2000 x 2000 keypoints of the DSC photographs under the seeded SuperPoint); after whitening
    the similarity is a Mahalanobis one and 216 - 406 are mutual (sharpness 2: 132 - 180 matches above 0.1, logits <= 220)."""
    sd = synthetic_lightglue_state_dict(seed, input_dim, n_layers, dim, gain=1.0, num_heads=num_heads)
    for k in list(sd):
        if ".ffn.3." in k:
            sd[k] = sd[k] * residual
        elif k.endswith("final_proj.weight"):
            sd[k] = torch.eye(dim) * sharpness if whiten is None else (sharpness * whiten.detach().float().cpu()).contiguous()
        elif k.endswith("final_proj.bias"):
            c = None if center is None else center.detach().float().cpu().reshape(-1)
            sd[k] = torch.zeros_like(sd[k]) if c is None else (-sharpness * (c if whiten is None else whiten.detach().float().cpu() @ c)).contiguous()
        elif k.endswith("matchability.weight"):
            sd[k] = sd[k] * 0.1
        elif k.endswith("matchability.bias"):
            sd[k] = torch.full_like(sd[k], matchability_bias)
    return sd


def descriptor_whitening(desc_nd: torch.Tensor, eps: float = 1e-5):
    """(center [D], whiten [D, D] float32) of a descriptor sample [N, D]: the mean and the symmetric inverse square root of the covariance
    (+ eps), computed in float64 — the arguments of synthetic_lightglue_matching_state_dict(center=, whiten=)."""
    x = desc_nd.detach().double().cpu()
    c = x.mean(0)
    xc = x - c
    ev, u = torch.linalg.eigh(xc.t() @ xc / x.shape[0])
    return c.float(), (u @ torch.diag(1.0 / torch.sqrt(ev.clamp_min(0.0) + eps)) @ u.t()).float().contiguous()


def load_lightglue_state_dict(path: str | None = None, seed: int = 0, input_dim: int = 256, n_layers: int = 9,
                              gain: float = 1.0, allow_synthetic: bool = False) -> Dict[str, torch.Tensor]:
    if path is None:
        _no_weights("LightGlue (<features>_lightglue.pth, LGN:383)", "DIM_LIGHTGLUE_WEIGHTS", allow_synthetic)
        return synthetic_lightglue_state_dict(seed, input_dim, n_layers, gain=gain)
    sd = torch.load(str(Path(path)), map_location="cpu")
    for i in range(n_layers):  # legacy names (LGN:389-396)
        sd = {k.replace(f"self_attn.{i}", f"transformers.{i}.self_attn"): v for k, v in sd.items()}
        sd = {k.replace(f"cross_attn.{i}", f"transformers.{i}.cross_attn"): v for k, v in sd.items()}
    if "confidence_thresholds" not in sd:
        sd["confidence_thresholds"] = lightglue_confidence_thresholds(n_layers)
    return {k: v.float().contiguous() for k, v in sd.items()}


LIGHTERGLUE_SHAPE = {"input_dim": 64, "descriptor_dim": 96, "num_heads": 1, "n_layers": 6}   # modules/lighterglue.py:12-27


def lighterglue_state_dict_shapes(input_dim: int = 64, dim: int = 96, n_layers: int = 6, num_heads: int = 1) -> Dict[str, tuple]:
    """Every tensor LighterGlueHIP reads, by its official (renamed) key."""
    sh = {"input_proj.weight": (dim, input_dim), "input_proj.bias": (dim,), "posenc.Wr.weight": (dim // num_heads // 2, 2)}
    for i in range(n_layers):
        t = f"transformers.{i}."
        sh.update({t + "self_attn.Wqkv.weight": (3 * dim, dim), t + "self_attn.Wqkv.bias": (3 * dim,),
                   t + "self_attn.out_proj.weight": (dim, dim), t + "self_attn.out_proj.bias": (dim,)})
        for blk in ("self_attn", "cross_attn"):
            sh.update({t + blk + ".ffn.0.weight": (2 * dim, 2 * dim), t + blk + ".ffn.0.bias": (2 * dim,), t + blk + ".ffn.1.weight": (2 * dim,),
                       t + blk + ".ffn.1.bias": (2 * dim,), t + blk + ".ffn.3.weight": (dim, 2 * dim), t + blk + ".ffn.3.bias": (dim,)})
        for nm in ("to_qk", "to_v", "to_out"):
            sh.update({t + f"cross_attn.{nm}.weight": (dim, dim), t + f"cross_attn.{nm}.bias": (dim,)})
        sh.update({f"log_assignment.{i}.matchability.weight": (1, dim), f"log_assignment.{i}.matchability.bias": (1,),
                   f"log_assignment.{i}.final_proj.weight": (dim, dim), f"log_assignment.{i}.final_proj.bias": (dim,)})
        if i < n_layers - 1:
            sh.update({f"token_confidence.{i}.token.0.weight": (1, dim), f"token_confidence.{i}.token.0.bias": (1,)})
    return sh


def validate_lighterglue_state_dict(sd: Dict[str, torch.Tensor]) -> None:
    for k, shape in lighterglue_state_dict_shapes().items():
        if k not in sd:
            raise KeyError(f"LighterGlue checkpoint lacks '{k}'")
        if tuple(sd[k].shape) != shape:
            raise ValueError(f"LighterGlue checkpoint: '{k}' has shape {tuple(sd[k].shape)}, expected {shape}")


def synthetic_lighterglue_state_dict(seed: int = 0, matching: bool = True, **kw) -> Dict[str, torch.Tensor]:
    """Seeded synthetic weights at LighterGlue's shape (64 -> 96, one head, 6 layers): the matching kind by default."""
    shape = dict(input_dim=64, n_layers=6, dim=96, num_heads=1)
    if matching:
        return synthetic_lightglue_matching_state_dict(seed, **shape, **kw)
    return synthetic_lightglue_state_dict(seed, **shape, **kw)


def load_lighterglue_state_dict(path: str | None = None, seed: int = 0, allow_synthetic: bool = False) -> Dict[str, torch.Tensor]:
    """xfeat-lighterglue.pt with the reference's key renames (modules/lighterglue.py:41-46: `matcher.` stripped, self_attn.{i} / cross_attn.{i}
    -> transformers.{i}.*), shapes validated.  ``path`` None: the DIM_LIGHTERGLUE_WEIGHTS environment variable, else (opt-in) synthetic weights."""
    import os

    path = path or os.environ.get("DIM_LIGHTERGLUE_WEIGHTS") or None
    if path is None:
        _no_weights("LighterGlue (xfeat-lighterglue.pt, modules/lighterglue.py:33-37)", "DIM_LIGHTERGLUE_WEIGHTS", allow_synthetic)
        return synthetic_lighterglue_state_dict(seed)
    sd = torch.load(str(Path(path)), map_location="cpu")
    for i in range(LIGHTERGLUE_SHAPE["n_layers"]):
        sd = {k.replace(f"self_attn.{i}", f"transformers.{i}.self_attn"): v for k, v in sd.items()}
        sd = {k.replace(f"cross_attn.{i}", f"transformers.{i}.cross_attn"): v for k, v in sd.items()}
        sd = {k.replace("matcher.", ""): v for k, v in sd.items()}
    if "confidence_thresholds" not in sd:
        sd["confidence_thresholds"] = lightglue_confidence_thresholds(LIGHTERGLUE_SHAPE["n_layers"])
    sd = {k: v.float().contiguous() for k, v in sd.items()}
    validate_lighterglue_state_dict(sd)
    return sd


ALIKED_CFGS = {  # ALN:573-579  c1, c2, c3, c4, dim, K, M
    "aliked-t16": (8, 16, 32, 64, 64, 3, 16),
    "aliked-n16": (16, 32, 64, 128, 128, 3, 16),
    "aliked-n16rot": (16, 32, 64, 128, 128, 3, 16),
    "aliked-n32": (16, 32, 64, 128, 128, 3, 32),
}


def synthetic_aliked_state_dict(seed: int = 7, model_name: str = "aliked-n16rot") -> Dict[str, torch.Tensor]:
    """Seeded synthetic ALIKED weights in the official key layout (the real
    aliked-*.pth files live in the reference tree under thirdparty/ALIKED/models and load unchanged
    through load_aliked_state_dict).  BN running stats are included for layout fidelity only: the
    plugin runs BatchNorm in training mode (Q7) and never reads them."""
    c1, c2, c3, c4, dim, K, M = ALIKED_CFGS[model_name]
    g = torch.Generator().manual_seed(seed)
    sd: Dict[str, torch.Tensor] = {}

    def conv(name, co, ci, k, bias=False, gain=1.0):
        sd[name + ".weight"] = torch.randn(co, ci, k, k, generator=g) * (gain * math.sqrt(2.0 / (ci * k * k)))
        if bias:
            sd[name + ".bias"] = torch.randn(co, generator=g) * 0.05

    def bn(name, c):
        sd[name + ".weight"] = 1.0 + 0.1 * torch.randn(c, generator=g)
        sd[name + ".bias"] = 0.1 * torch.randn(c, generator=g)
        sd[name + ".running_mean"] = torch.zeros(c)
        sd[name + ".running_var"] = torch.ones(c)
        sd[name + ".num_batches_tracked"] = torch.tensor(0)

    conv("block1.conv1", c1, 3, 3); bn("block1.bn1", c1); conv("block1.conv2", c1, c1, 3); bn("block1.bn2", c1)
    conv("block2.conv1", c2, c1, 3); bn("block2.bn1", c2); conv("block2.conv2", c2, c2, 3); bn("block2.bn2", c2)
    conv("block2.downsample", c2, c1, 1, bias=True)
    for blk, ci, co in (("block3", c2, c3), ("block4", c3, c4)):
        conv(blk + ".conv1.offset_conv", 2 * K * K, ci, 3, bias=True, gain=0.7)
        conv(blk + ".conv1.regular_conv", co, ci, 3)
        bn(blk + ".bn1", co)
        conv(blk + ".conv2.offset_conv", 2 * K * K, co, 3, bias=True, gain=0.7)
        conv(blk + ".conv2.regular_conv", co, co, 3)
        bn(blk + ".bn2", co)
        conv(blk + ".downsample", co, ci, 1, bias=True)
    conv("conv1", dim // 4, c1, 1); conv("conv2", dim // 4, c2, 1); conv("conv3", dim // 4, c3, 1); conv("conv4", dim // 4, dim, 1)
    conv("score_head.0", 8, dim, 1); conv("score_head.2", 4, 8, 3); conv("score_head.4", 4, 4, 3); conv("score_head.6", 1, 4, 3, gain=2.0)
    sd["desc_head.agg_weights"] = torch.rand(M, dim, dim, generator=g) * (2.0 / math.sqrt(M * dim)) - (1.0 / math.sqrt(M * dim))
    conv("desc_head.offset_conv.0", 2 * M, dim, K, bias=True)
    conv("desc_head.offset_conv.2", 2 * M, 2 * M, 1, bias=True, gain=2.0)
    conv("desc_head.sf_conv", dim, dim, 1)
    return sd


def load_aliked_state_dict(path: str | None = None, seed: int = 7, model_name: str = "aliked-n16rot",
                           allow_synthetic: bool = False) -> Dict[str, torch.Tensor]:
    if path is None:
        _no_weights("ALIKED (thirdparty/ALIKED/models/aliked-*.pth in the reference tree)", "DIM_ALIKED_WEIGHTS", allow_synthetic)
        return synthetic_aliked_state_dict(seed, model_name)
    sd = torch.load(str(Path(path)), map_location="cpu")
    return {k: (v.float().contiguous() if v.is_floating_point() else v) for k, v in sd.items()}


ALIKE_CFGS = {  # thirdparty/alike/alike.py:15-56  c1, c2, c3, c4, dim, single_head, radius
    "alike-t": (8, 16, 32, 64, 64, 1, 2),
    "alike-s": (8, 16, 48, 96, 96, 1, 2),
    "alike-n": (16, 32, 64, 128, 128, 1, 2),
    "alike-l": (32, 64, 128, 128, 128, 0, 2),
}
ALIKE_BN = ["block1.bn1", "block1.bn2", "block2.bn1", "block2.bn2", "block3.bn1", "block3.bn2", "block4.bn1", "block4.bn2"]


def alike_state_dict_shapes(model: str) -> Dict[str, tuple]:
    """Every tensor of an ALIKE checkpoint and its shape, derived from the model's geometry row (alnet.py:104-153)."""
    if model not in ALIKE_CFGS:
        raise ValueError(f"unknown ALIKE model {model!r}; expected one of {sorted(ALIKE_CFGS)}")
    c1, c2, c3, c4, dim, single_head, _ = ALIKE_CFGS[model]
    t: Dict[str, tuple] = {}
    for blk, ci, co in (("block1", 3, c1), ("block2", c1, c2), ("block3", c2, c3), ("block4", c3, c4)):
        t[blk + ".conv1.weight"] = (co, ci, 3, 3)
        t[blk + ".conv2.weight"] = (co, co, 3, 3)
        for bn in ("bn1", "bn2"):
            for leaf in ("weight", "bias", "running_mean", "running_var"):
                t[f"{blk}.{bn}.{leaf}"] = (co,)
            t[f"{blk}.{bn}.num_batches_tracked"] = ()
        if blk != "block1":
            t[blk + ".downsample.weight"] = (co, ci, 1, 1)
            t[blk + ".downsample.bias"] = (co,)
    # conv4 is declared conv1x1(dim, dim // 4) (alnet.py:135) and applied to block4's c4 channels: every shipped row has c4 == dim
    for name, ci in (("conv1", c1), ("conv2", c2), ("conv3", c3), ("conv4", dim)):
        t[name + ".weight"] = (dim // 4, ci, 1, 1)
    if not single_head:
        t["convhead1.weight"] = (dim, dim, 1, 1)
    t["convhead2.weight"] = (dim + 1, dim, 1, 1)
    return t


def validate_alike_state_dict(sd: Dict[str, torch.Tensor], model: str) -> None:
    """KeyError for a missing / unexpected tensor, ValueError for a wrong shape — each naming the tensor — before anything native is called."""
    table = alike_state_dict_shapes(model)
    for k, shape in table.items():
        if k not in sd:
            if k.endswith("num_batches_tracked"):
                continue
            raise KeyError(f"ALIKE {model}: state dict has no tensor {k!r}")
        if tuple(sd[k].shape) != tuple(shape):
            raise ValueError(f"ALIKE {model}: tensor {k!r} has shape {tuple(sd[k].shape)}, expected {tuple(shape)}")
    for k in sd:
        if k not in table:
            raise KeyError(f"ALIKE {model}: unexpected tensor {k!r} in the state dict")


def synthetic_alike_state_dict(seed: int = 11, model: str = "alike-n") -> Dict[str, torch.Tensor]:
    """Seeded synthetic ALIKE weights in the checkpoint layout (running statistics included: BatchNorm runs in eval mode)."""
    g = torch.Generator().manual_seed(seed)
    sd: Dict[str, torch.Tensor] = {}
    for k, shape in alike_state_dict_shapes(model).items():
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(0)
        elif k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(shape, generator=g)
        elif k.endswith("running_mean") or k.endswith(".bias"):
            sd[k] = 0.1 * torch.randn(shape, generator=g)
        elif len(shape) == 1:
            sd[k] = 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:
            sd[k] = torch.randn(shape, generator=g) * math.sqrt(2.0 / (shape[1] * shape[2] * shape[3]))
    return sd


def load_alike_state_dict(path: str | None = None, model: str = "alike-s", seed: int = 11, allow_synthetic: bool = False) -> Dict[str, torch.Tensor]:
    """thirdparty/alike/models/alike-{t,s,n,l}.pth (a plain state dict; alike.py:90-92), validated against the model's geometry.
    ``path``: a file name, or an open binary file holding the same bytes (the tests join the checkpoint from slices in memory)."""
    if model not in ALIKE_CFGS:
        raise ValueError(f"unknown ALIKE model {model!r}; expected one of {sorted(ALIKE_CFGS)}")
    if path is None:
        _no_weights("ALIKE (thirdparty/alike/models/alike-*.pth in the reference tree)", "DIM_ALIKE_WEIGHTS", allow_synthetic)
        return synthetic_alike_state_dict(seed, model)
    sd = torch.load(path if hasattr(path, "read") else str(Path(path)), map_location="cpu")   # (a path or an open binary file)
    sd = {k: (v.float().contiguous() if v.is_floating_point() else v) for k, v in sd.items()}
    validate_alike_state_dict(sd, model)
    return sd


# ---- the open SuperPoint (thirdparty/SuperPoint_open/superpoint_pytorch.py; checkpoint superpoint_v6_from_tf.pth) ----------------------------
# block prefix per layer, in SP_LAYERS order: backbone.{stage}.{0,1} = conv{stage+1}{a,b}, detector.{0,1} = convPa / convPb, descriptor.{0,1} = convDa / convDb
SPO_BLOCKS = [f"backbone.{i}.{j}" for i in range(4) for j in range(2)] + ["detector.0", "detector.1", "descriptor.0", "descriptor.1"]
SPO_BN_EPS = 1e-3  # VGGBlock: nn.BatchNorm2d(c_out, eps=0.001)


def superpoint_open_state_dict_shapes() -> Dict[str, tuple]:
    """Every tensor of the open SuperPoint's checkpoint and its shape: per block conv.{weight, bias} and bn.{weight, bias, running_mean, running_var}
    (+ the optional scalar bn.num_batches_tracked), with the layer geometry of SP_LAYERS."""
    t: Dict[str, tuple] = {}
    for blk, (_, co, ci, k) in zip(SPO_BLOCKS, SP_LAYERS):
        t[f"{blk}.conv.weight"] = (co, ci, k, k)
        t[f"{blk}.conv.bias"] = (co,)
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            t[f"{blk}.bn.{leaf}"] = (co,)
        t[f"{blk}.bn.num_batches_tracked"] = ()
    return t


def validate_superpoint_open_state_dict(sd: Dict[str, torch.Tensor]) -> None:
    """KeyError for a missing / unexpected tensor, ValueError for a wrong shape, a non-finite value or running_var + eps <= 0 — each naming the
    tensor — before anything native is called."""
    table = superpoint_open_state_dict_shapes()
    for k, shape in table.items():
        if k not in sd:
            if k.endswith("num_batches_tracked"):
                continue
            raise KeyError(f"SuperPoint (open): state dict has no tensor {k!r}")
        if tuple(sd[k].shape) != tuple(shape):
            raise ValueError(f"SuperPoint (open): tensor {k!r} has shape {tuple(sd[k].shape)}, expected {tuple(shape)}")
        if sd[k].is_floating_point() and not bool(torch.isfinite(sd[k]).all()):
            raise ValueError(f"SuperPoint (open): tensor {k!r} holds a non-finite value")
        if k.endswith("running_var") and not bool((sd[k].double() + SPO_BN_EPS > 0).all()):
            raise ValueError(f"SuperPoint (open): tensor {k!r} has an entry with running_var + eps <= 0")
    for k in sd:
        if k not in table:
            raise KeyError(f"SuperPoint (open): unexpected tensor {k!r} in the state dict")


def synthetic_superpoint_open_state_dict(seed: int = 4321, negative_gamma: float = 0.3, off_centre: float = 1.0) -> Dict[str, torch.Tensor]:
    """Seeded synthetic weights in the checkpoint's layout.  He-normal convolutions, small biases; BatchNorm |gamma| in [0.5, 1) with about
    ``negative_gamma`` of the channels NEGATIVE (they turn the pool behind the BatchNorm into a min-pool of the ReLU output), beta ~ 0.1 N,
    running_mean in [0.2, 0.6) and running_var in [0.25, 0.75) — around the mean 0.40 and variance 0.34 of the ReLU of a unit normal, so the
    activations keep their scale from layer to layer and the 65 logits stay O(1): a score map that is neither uniform nor one-hot.
    ``off_centre`` < 1 multiplies the eight off-centre taps of the 3x3 kernels of stages 3 and 4 and of the two heads (the kernel is rescaled to
    its He variance): centre-heavy kernels narrow the effective receptive field, which for He-normal kernels spans most of a small test image
    (the descriptors of two overlapping crops then differ wherever a crop border is within ~40 px)."""
    g = torch.Generator().manual_seed(seed)
    sd: Dict[str, torch.Tensor] = {}
    for blk, (_, co, ci, k) in zip(SPO_BLOCKS, SP_LAYERS):
        sd[f"{blk}.conv.weight"] = torch.randn(co, ci, k, k, generator=g) * math.sqrt(2.0 / (ci * k * k))
        if off_centre != 1.0 and k == 3 and blk.startswith(("backbone.2", "backbone.3", "detector", "descriptor")):
            m = torch.full((3, 3), float(off_centre))
            m[1, 1] = 1.0
            sd[f"{blk}.conv.weight"] *= m * math.sqrt(9.0 / float((m * m).sum()))
        sd[f"{blk}.conv.bias"] = torch.randn(co, generator=g) * 0.01
        sign = torch.where(torch.rand(co, generator=g) < negative_gamma, -1.0, 1.0)
        sd[f"{blk}.bn.weight"] = (0.5 + 0.5 * torch.rand(co, generator=g)) * sign
        sd[f"{blk}.bn.bias"] = 0.1 * torch.randn(co, generator=g)
        sd[f"{blk}.bn.running_mean"] = 0.2 + 0.4 * torch.rand(co, generator=g)
        sd[f"{blk}.bn.running_var"] = 0.25 + 0.5 * torch.rand(co, generator=g)
        sd[f"{blk}.bn.num_batches_tracked"] = torch.tensor(0)
    return sd


def load_superpoint_open_state_dict(path: str | None = None, seed: int = 4321, allow_synthetic: bool = False) -> Dict[str, torch.Tensor]:
    """thirdparty/SuperPoint_open/weights/superpoint_v6_from_tf.pth (a plain state dict of superpoint_pytorch.SuperPoint), validated against the
    one table of keys and shapes.  ``path``: a file name or an open binary file."""
    if path is None:
        _no_weights("SuperPoint (open; thirdparty/SuperPoint_open/weights/superpoint_v6_from_tf.pth in the reference tree)", "DIM_SUPERPOINT_OPEN_WEIGHTS", allow_synthetic)
        return synthetic_superpoint_open_state_dict(seed)
    sd = torch.load(path if hasattr(path, "read") else str(Path(path)), map_location="cpu")
    sd = {k: (v.float().contiguous() if v.is_floating_point() else v) for k, v in sd.items()}
    validate_superpoint_open_state_dict(sd)
    return sd


# ---- XFeat (thirdparty/accelerated_features/modules/model.py; checkpoint weights/xfeat.pt) ---------------------------------------------------
# BasicLayer = conv (no bias) -> BatchNorm2d(affine=False) in eval mode -> ReLU (model.py:12-25): prefix, cout, cin, kernel, stride
XFEAT_BASIC = [
    ("block1.0", 4, 1, 3, 1), ("block1.1", 8, 4, 3, 2), ("block1.2", 8, 8, 3, 1), ("block1.3", 24, 8, 3, 2),
    ("block2.0", 24, 24, 3, 1), ("block2.1", 24, 24, 3, 1),
    ("block3.0", 64, 24, 3, 2), ("block3.1", 64, 64, 3, 1), ("block3.2", 64, 64, 1, 1),
    ("block4.0", 64, 64, 3, 2), ("block4.1", 64, 64, 3, 1), ("block4.2", 64, 64, 3, 1),
    ("block5.0", 128, 64, 3, 2), ("block5.1", 128, 128, 3, 1), ("block5.2", 128, 128, 3, 1), ("block5.3", 64, 128, 1, 1),
    ("block_fusion.0", 64, 64, 3, 1), ("block_fusion.1", 64, 64, 3, 1),
    ("heatmap_head.0", 64, 64, 1, 1), ("heatmap_head.1", 64, 64, 1, 1),
    ("keypoint_head.0", 64, 64, 1, 1), ("keypoint_head.1", 64, 64, 1, 1), ("keypoint_head.2", 64, 64, 1, 1),
]
# plain 1x1 convolutions with a bias: prefix, cout, cin
XFEAT_BIASED = [("skip1.1", 24, 1), ("block_fusion.2", 64, 64), ("heatmap_head.2", 1, 64), ("keypoint_head.3", 65, 64)]
XFEAT_BN_EPS = 1e-5


def _xfeat_layout():
    t = []
    for p, co, ci, k, _ in XFEAT_BASIC:
        t += [(f"{p}.layer.0.weight", (co, ci, k, k)), (f"{p}.layer.1.running_mean", (co,)), (f"{p}.layer.1.running_var", (co,)),
              (f"{p}.layer.1.num_batches_tracked", ())]
    for p, co, ci in XFEAT_BIASED:
        t += [(f"{p}.weight", (co, ci, 1, 1)), (f"{p}.bias", (co,))]
    return t


XFEAT_LAYOUT = _xfeat_layout()   # (key, shape) of every tensor detectAndCompute uses


def validate_xfeat_state_dict(sd: Dict[str, torch.Tensor]) -> None:
    """KeyError for a missing / unexpected tensor, ValueError for a wrong shape, a non-finite value or a negative running_var — each naming the
    tensor — before anything native is called.  ``fine_matcher.*`` (used by match_xfeat_star only) and ``num_batches_tracked`` are accepted and
    ignored, present or not."""
    table = dict(XFEAT_LAYOUT)
    for k, shape in XFEAT_LAYOUT:
        if k not in sd:
            if k.endswith("num_batches_tracked"):
                continue
            raise KeyError(f"XFeat: state dict has no tensor {k!r}")
        if tuple(sd[k].shape) != tuple(shape):
            raise ValueError(f"XFeat: tensor {k!r} has shape {tuple(sd[k].shape)}, expected {tuple(shape)}")
        if sd[k].is_floating_point() and not bool(torch.isfinite(sd[k]).all()):
            raise ValueError(f"XFeat: tensor {k!r} holds a non-finite value")
        if k.endswith("running_var") and not bool((sd[k] >= 0).all()):
            raise ValueError(f"XFeat: tensor {k!r} has a negative entry")
    for k in sd:
        if k not in table and not k.startswith("fine_matcher."):
            raise KeyError(f"XFeat: unexpected tensor {k!r} in the state dict")


def synthetic_xfeat_state_dict(seed: int = 21) -> Dict[str, torch.Tensor]:
    """Seeded synthetic XFeat weights in the checkpoint's layout (without fine_matcher.*): He-normal convolutions, biases and running means
    0.1 N(0, 1), running variances U(0.5, 1.5)."""
    g = torch.Generator().manual_seed(seed)
    sd: Dict[str, torch.Tensor] = {}
    for k, shape in XFEAT_LAYOUT:
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(0)
        elif k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(shape, generator=g)
        elif len(shape) == 1:
            sd[k] = 0.1 * torch.randn(shape, generator=g)
        else:
            sd[k] = torch.randn(shape, generator=g) * math.sqrt(2.0 / (shape[1] * shape[2] * shape[3]))
    return sd


def load_xfeat_state_dict(path: str | None = None, seed: int = 21, allow_synthetic: bool = False) -> Dict[str, torch.Tensor]:
    """thirdparty/accelerated_features/weights/xfeat.pt (a plain state dict of XFeatModel), validated against XFEAT_LAYOUT.
    ``path``: a file name or an open binary file."""
    if path is None:
        _no_weights("XFeat (thirdparty/accelerated_features/weights/xfeat.pt in the reference tree)", "DIM_XFEAT_WEIGHTS", allow_synthetic)
        return synthetic_xfeat_state_dict(seed)
    sd = torch.load(path if hasattr(path, "read") else str(Path(path)), map_location="cpu")
    sd = {k: (v.float().contiguous() if v.is_floating_point() else v) for k, v in sd.items()}
    validate_xfeat_state_dict(sd)
    return sd


# ---- SuperGlue (thirdparty/SuperGluePretrainedNetwork/models/superglue.py, SGN) ----------------------------------------------------------
SUPERGLUE_KENC = [3, 32, 64, 128, 256, 256]   # SGN:79,215: MLP([3] + keypoint_encoder + [descriptor_dim])
SUPERGLUE_BN_EPS = 1e-5
_SG_BN = ("weight", "bias", "running_mean", "running_var")


def superglue_n_layers(sd: Dict[str, torch.Tensor]) -> int:
    """len(GNN_layers) as the state dict has it (gnn.layers.{i}.*)."""
    idx = {int(k.split(".")[2]) for k in sd if k.startswith("gnn.layers.")}
    return max(idx) + 1 if idx else 0


def superglue_state_dict_shapes(n_layers: int = 18) -> Dict[str, tuple]:
    """Every tensor SuperGlueHIP reads, by the module's key (Conv1d weights keep their kernel axis)."""
    sh = {"bin_score": (), "final_proj.weight": (256, 256, 1), "final_proj.bias": (256,)}
    c = SUPERGLUE_KENC
    for s in range(5):
        sh[f"kenc.encoder.{3 * s}.weight"] = (c[s + 1], c[s], 1)
        sh[f"kenc.encoder.{3 * s}.bias"] = (c[s + 1],)
        if s < 4:
            sh.update({f"kenc.encoder.{3 * s + 1}.{n}": (c[s + 1],) for n in _SG_BN})
    for i in range(n_layers):
        t = f"gnn.layers.{i}."
        for nm in ("attn.merge", "attn.proj.0", "attn.proj.1", "attn.proj.2"):
            sh[t + nm + ".weight"], sh[t + nm + ".bias"] = (256, 256, 1), (256,)
        sh[t + "mlp.0.weight"], sh[t + "mlp.0.bias"] = (512, 512, 1), (512,)
        sh.update({t + f"mlp.1.{n}": (512,) for n in _SG_BN})
        sh[t + "mlp.3.weight"], sh[t + "mlp.3.bias"] = (256, 512, 1), (256,)
    return sh


def validate_superglue_state_dict(sd: Dict[str, torch.Tensor]) -> int:
    """Checks keys and shapes; returns the layer count (a positive multiple of 2: self / cross alternate, SGN:216)."""
    n_layers = superglue_n_layers(sd)
    if n_layers == 0 or n_layers % 2:
        raise ValueError(f"SuperGlue checkpoint: {n_layers} GNN layers (gnn.layers.*), expected a positive multiple of 2")
    for k, shape in superglue_state_dict_shapes(n_layers).items():
        if k not in sd:
            raise KeyError(f"SuperGlue checkpoint lacks '{k}'")
        if tuple(sd[k].shape) != shape:
            raise ValueError(f"SuperGlue checkpoint: '{k}' has shape {tuple(sd[k].shape)}, expected {shape}")
    return n_layers


def synthetic_superglue_state_dict(seed: int = 0, n_layers: int = 18, final_gain: float = 14.0, delta_gain: float = 0.25,
                                   bin_score: float = 2.0) -> Dict[str, torch.Tensor]:
    """Seeded synthetic weights with which the network really matches: variance-preserving convolutions, BatchNorm layers with non-trivial
    running statistics, the last convolution of every residual mlp damped by ``delta_gain`` (18 layers stay inside the fp16 split's range and
    keep corresponding descriptors close), final_proj = ``final_gain`` x a random orthogonal matrix (scores = gain^2 / 16 x the cosine)."""
    g = torch.Generator().manual_seed(seed)
    sd: Dict[str, torch.Tensor] = {}

    def conv(name, co, ci, gain=1.0, bias=0.02):
        sd[name + ".weight"] = torch.randn(co, ci, 1, generator=g) * (gain / math.sqrt(ci))
        sd[name + ".bias"] = torch.randn(co, generator=g) * bias

    def bn(name, c):
        sd[name + ".weight"] = 0.6 + 0.8 * torch.rand(c, generator=g)
        sd[name + ".bias"] = 0.1 * torch.randn(c, generator=g)
        sd[name + ".running_mean"] = 0.1 * torch.randn(c, generator=g)
        sd[name + ".running_var"] = 0.5 + torch.rand(c, generator=g)
        sd[name + ".num_batches_tracked"] = torch.tensor(1000)

    c = SUPERGLUE_KENC
    for s in range(5):
        conv(f"kenc.encoder.{3 * s}", c[s + 1], c[s], gain=1.4 if s < 4 else 0.05)
        if s < 4:
            bn(f"kenc.encoder.{3 * s + 1}", c[s + 1])
    sd["kenc.encoder.12.bias"] = torch.zeros(256)   # SGN:80
    for i in range(n_layers):
        t = f"gnn.layers.{i}."
        conv(t + "attn.merge", 256, 256)
        for j in range(3):
            conv(t + f"attn.proj.{j}", 256, 256, gain=4.0 if j < 2 else 1.0)
        conv(t + "mlp.0", 512, 512, gain=1.4)
        bn(t + "mlp.1", 512)
        conv(t + "mlp.3", 256, 512, gain=delta_gain)
        sd[t + "mlp.3.bias"] = torch.zeros(256)   # SGN:124
    q, _ = torch.linalg.qr(torch.randn(256, 256, generator=g, dtype=torch.float64))
    sd["final_proj.weight"] = (final_gain * q).float()[:, :, None].contiguous()
    sd["final_proj.bias"] = torch.randn(256, generator=g) * 0.01
    sd["bin_score"] = torch.tensor(float(bin_score))
    return sd


def superglue_head_permutation() -> torch.Tensor:
    """perm[h * 64 + d] = d * 4 + h: the module's attention channel (view(b, 64, 4, n), SGN:112) behind every head-major device channel."""
    c = torch.arange(256)
    return (c % 64) * 4 + c // 64


def prepare_superglue_weights(sd: Dict[str, torch.Tensor], dtype=torch.float32) -> Dict[str, torch.Tensor]:
    """What dim_sg_create takes: (out, in) fp32 matrices with BatchNorm1d (eval) folded into the convolution in front of it and the attention
    channels permuted to head-major (rows of proj.0-2, columns of merge).  All arithmetic in fp64, rounded once (``dtype`` = torch.float64: not
    at all — what the host-side test compares with the unfolded module)."""
    n_layers = validate_superglue_state_dict(sd)
    d = lambda k: sd[k].detach().double()
    mat = lambda k: d(k).reshape(sd[k].shape[0], sd[k].shape[1])

    def folded(conv, norm):
        s = d(norm + ".weight") / torch.sqrt(d(norm + ".running_var") + SUPERGLUE_BN_EPS)
        return mat(conv + ".weight") * s[:, None], (d(conv + ".bias") - d(norm + ".running_mean")) * s + d(norm + ".bias")

    out: Dict[str, torch.Tensor] = {}
    for s in range(5):
        if s < 4:
            out[f"kenc.{s}.w"], out[f"kenc.{s}.b"] = folded(f"kenc.encoder.{3 * s}", f"kenc.encoder.{3 * s + 1}")
        else:
            out[f"kenc.{s}.w"], out[f"kenc.{s}.b"] = mat("kenc.encoder.12.weight"), d("kenc.encoder.12.bias")
    perm = superglue_head_permutation()
    for i in range(n_layers):
        t = f"gnn.layers.{i}."
        for j, nm in enumerate("qkv"):
            out[f"{i}.{nm}_w"], out[f"{i}.{nm}_b"] = mat(t + f"attn.proj.{j}.weight")[perm], d(t + f"attn.proj.{j}.bias")[perm]
        out[f"{i}.merge_w"], out[f"{i}.merge_b"] = mat(t + "attn.merge.weight")[:, perm], d(t + "attn.merge.bias")
        out[f"{i}.mlp0_w"], out[f"{i}.mlp0_b"] = folded(t + "mlp.0", t + "mlp.1")
        out[f"{i}.mlp3_w"], out[f"{i}.mlp3_b"] = mat(t + "mlp.3.weight"), d(t + "mlp.3.bias")
    out["final_proj.w"], out["final_proj.b"] = mat("final_proj.weight"), d("final_proj.bias")
    out = {k: v.to(dtype).contiguous() for k, v in out.items()}
    out["bin_score"] = sd["bin_score"].detach().to(dtype).reshape(())
    return out


def load_superglue_state_dict(path: str | None = None, seed: int = 0, allow_synthetic: bool = False) -> Dict[str, torch.Tensor]:
    """superglue_{indoor,outdoor}.pth (SGN:244-247), shapes validated.  ``path`` None: the DIM_SUPERGLUE_WEIGHTS environment variable, else
    (opt-in) synthetic weights."""
    import os

    path = path or os.environ.get("DIM_SUPERGLUE_WEIGHTS") or None
    if path is None:
        _no_weights("SuperGlue (superglue_outdoor.pth / superglue_indoor.pth, SGN:244-247)", "DIM_SUPERGLUE_WEIGHTS", allow_synthetic)
        return synthetic_superglue_state_dict(seed)
    sd = torch.load(str(Path(path)), map_location="cpu")
    sd = {k: (v.float().contiguous() if v.is_floating_point() else v) for k, v in sd.items()}
    validate_superglue_state_dict(sd)
    return sd


# ---- NetVLAD (thirdparty/hloc/extractors/netvlad.py, NV) -------------------------------------------------------------------------------
# VGG16 features[:-2] (NV:66-68): (index in the Sequential = index in the checkpoint's net.layers, cout, cin); pools sit at 4, 9, 16, 23
NETVLAD_CONVS = [(0, 64, 3), (2, 64, 64), (5, 128, 64), (7, 128, 128), (10, 256, 128), (12, 256, 256), (14, 256, 256),
                 (17, 512, 256), (19, 512, 512), (21, 512, 512), (24, 512, 512), (26, 512, 512), (28, 512, 512)]
NETVLAD_DIM = 512
NETVLAD_MAT_LAYERS, NETVLAD_MAT_VLAD, NETVLAD_MAT_WHITEN = 35, 30, 33   # NV:79,93,107


def netvlad_state_shapes(K: int = 64, whiten_out: Optional[int] = 4096) -> Dict[str, tuple]:
    """The NetVLAD module's own state-dict keys (NV:68-73) plus ``preprocess.mean`` (NV:118); ``whiten_out`` None / 0: no whitening."""
    t = {}
    for i, co, ci in NETVLAD_CONVS:
        t[f"backbone.{i}.weight"] = (co, ci, 3, 3)
        t[f"backbone.{i}.bias"] = (co,)
    t["netvlad.score_proj.weight"] = (K, NETVLAD_DIM, 1)
    t["netvlad.centers"] = (NETVLAD_DIM, K)
    if whiten_out:
        t["whiten.weight"] = (whiten_out, NETVLAD_DIM * K)
        t["whiten.bias"] = (whiten_out,)
    t["preprocess.mean"] = (3,)
    return t


def validate_netvlad_state(sd: Dict[str, torch.Tensor]) -> tuple:
    """(K, whiten_out or 0).  KeyError for a missing / unexpected tensor, ValueError for a wrong shape, a cluster count that is no multiple of 8 up
    to 64 or a non-finite value — each naming the tensor — before anything native is called."""
    if "netvlad.centers" not in sd:
        raise KeyError("NetVLAD: state has no tensor 'netvlad.centers'")
    c = sd["netvlad.centers"]
    if c.dim() != 2 or c.shape[0] != NETVLAD_DIM or c.shape[1] % 8 != 0 or not 8 <= c.shape[1] <= 64:
        raise ValueError(f"NetVLAD: tensor 'netvlad.centers' has shape {tuple(c.shape)}, expected ({NETVLAD_DIM}, K) with K a multiple of 8 up to 64")
    K = int(c.shape[1])
    wo = int(sd["whiten.bias"].shape[0]) if "whiten.bias" in sd and sd["whiten.bias"].dim() == 1 else 0
    if ("whiten.weight" in sd) != ("whiten.bias" in sd):
        raise KeyError("NetVLAD: 'whiten.weight' and 'whiten.bias' come together")
    table = netvlad_state_shapes(K, wo)
    for k, shape in table.items():
        if k not in sd:
            raise KeyError(f"NetVLAD: state has no tensor {k!r}")
        if tuple(sd[k].shape) != tuple(shape):
            raise ValueError(f"NetVLAD: tensor {k!r} has shape {tuple(sd[k].shape)}, expected {tuple(shape)}")
        if not bool(torch.isfinite(sd[k]).all()):
            raise ValueError(f"NetVLAD: tensor {k!r} holds a non-finite value")
    for k in sd:
        if k not in table:
            raise KeyError(f"NetVLAD: unexpected tensor {k!r} in the state")
    return K, wo


def synthetic_netvlad_state(seed: int = 31, K: int = 64, whiten_out: Optional[int] = 4096) -> Dict[str, torch.Tensor]:
    """Seeded synthetic NetVLAD weights under the module's keys.  He-normal convolutions with 0.1 N(0, 1) biases keep the second moment of the
    activations from layer to layer (the normalised image has |x| <= 152), so they neither vanish nor leave the fp16x3 range; score weights
    4 N(0, 1) (unit-norm inputs: soft assignments that are neither uniform nor one-hot), centres N(0, 1) / sqrt(512), whitening N(0, 1) / sqrt(512 K)
    with a 0.01 N(0, 1) bias, mean = the ImageNet-like (123.68, 116.78, 103.94) the trained checkpoints carry to within a count."""
    g = torch.Generator().manual_seed(seed)
    sd: Dict[str, torch.Tensor] = {}
    for k, shape in netvlad_state_shapes(K, whiten_out).items():
        if k == "preprocess.mean":
            sd[k] = torch.tensor([123.68, 116.78, 103.94])
        elif k.startswith("backbone.") and len(shape) == 4:
            sd[k] = torch.randn(shape, generator=g) * math.sqrt(2.0 / (shape[1] * 9))
        elif k.startswith("backbone."):
            sd[k] = 0.1 * torch.randn(shape, generator=g)
        elif k == "netvlad.score_proj.weight":
            sd[k] = 4.0 * torch.randn(shape, generator=g)
        elif k == "netvlad.centers":
            sd[k] = torch.randn(shape, generator=g) / math.sqrt(NETVLAD_DIM)
        elif k == "whiten.weight":
            sd[k] = torch.randn(shape, generator=g) / math.sqrt(shape[1])
        else:
            sd[k] = 0.01 * torch.randn(shape, generator=g)
    return sd


def netvlad_state_to_mat(sd: Dict[str, torch.Tensor]) -> dict:
    """The dict ``scipy.io.savemat`` turns into the checkpoint layout NV:76-121 reads: ``net.layers`` a 35-element cell whose entries at the
    backbone's convolution indices hold weights {HWIO, bias}, entry 30 {score (D, K), -centres (D, K)}, entry 33 {whitening (1, 1, IN, OUT), bias};
    ``net.meta.normalization.averageImage`` a (2, 2, 3) array of the mean."""
    import numpy as np

    def cell(*items):
        c = np.empty(len(items), dtype=object)
        for i, it in enumerate(items):
            c[i] = np.ascontiguousarray(it, dtype=np.float32)
        return c

    layers = np.empty(NETVLAD_MAT_LAYERS, dtype=object)
    for i in range(NETVLAD_MAT_LAYERS):
        layers[i] = {"type": "other"}
    for i, _, _ in NETVLAD_CONVS:
        layers[i] = {"type": "conv", "weights": cell(sd[f"backbone.{i}.weight"].permute(2, 3, 1, 0).numpy(), sd[f"backbone.{i}.bias"].numpy())}
    layers[NETVLAD_MAT_VLAD] = {"type": "vlad", "weights": cell(sd["netvlad.score_proj.weight"][:, :, 0].t().numpy(), -sd["netvlad.centers"].numpy())}
    if "whiten.weight" in sd:
        layers[NETVLAD_MAT_WHITEN] = {"type": "conv", "weights": cell(sd["whiten.weight"].t().numpy()[None, None], sd["whiten.bias"].numpy())}
    mean = np.broadcast_to(sd["preprocess.mean"].numpy().astype(np.float32), (2, 2, 3)).copy()
    return {"net": {"layers": layers, "meta": {"normalization": {"averageImage": mean}}}}


def load_netvlad_mat(path, whiten: bool = True) -> Dict[str, torch.Tensor]:
    """A NetVLAD checkpoint in the MATLAB struct layout the reference downloads (Pitts30K_struct.mat / TokyoTM_struct.mat, NV:48-51), read as
    NV:76-121 reads it: HWIO -> OIHW, the score matrix transposed, centres negated, the whitening squeezed and transposed, averageImage[0, 0].
    K and the whitening width are whatever the file holds.  Validated (validate_netvlad_state) before it is returned."""
    import numpy as np
    from scipy.io import loadmat

    mat = loadmat(str(path), struct_as_record=False, squeeze_me=True)
    layers = mat["net"].layers
    if len(layers) <= NETVLAD_MAT_WHITEN:
        raise ValueError(f"NetVLAD: net.layers has {len(layers)} entries, at least {NETVLAD_MAT_WHITEN + 1} expected")
    f32 = lambda a: torch.tensor(np.asarray(a, dtype=np.float32))  # noqa: E731
    sd: Dict[str, torch.Tensor] = {}
    for i, co, ci in NETVLAD_CONVS:
        w, b = f32(layers[i].weights[0]), f32(layers[i].weights[1])
        if tuple(w.shape) != (3, 3, ci, co):
            raise ValueError(f"NetVLAD: tensor 'backbone.{i}.weight' has shape {tuple(w.shape)} in the file, expected (3, 3, {ci}, {co})")
        sd[f"backbone.{i}.weight"] = w.permute(3, 2, 0, 1).contiguous()
        sd[f"backbone.{i}.bias"] = b.reshape(-1)
    score, centers = f32(layers[NETVLAD_MAT_VLAD].weights[0]), -f32(layers[NETVLAD_MAT_VLAD].weights[1])
    if score.dim() != 2:
        raise ValueError(f"NetVLAD: tensor 'netvlad.score_proj.weight' has shape {tuple(score.shape)} in the file, expected (512, K)")
    sd["netvlad.score_proj.weight"] = score.t().contiguous()[:, :, None]
    sd["netvlad.centers"] = centers.contiguous()
    if whiten:
        w, b = f32(layers[NETVLAD_MAT_WHITEN].weights[0]).squeeze(), f32(layers[NETVLAD_MAT_WHITEN].weights[1])
        if w.dim() != 2:
            raise ValueError(f"NetVLAD: tensor 'whiten.weight' has shape {tuple(w.shape)} in the file, expected (1, 1, IN, OUT)")
        sd["whiten.weight"] = w.t().contiguous()
        sd["whiten.bias"] = b.reshape(-1)
    sd["preprocess.mean"] = f32(mat["net"].meta.normalization.averageImage[0, 0]).reshape(-1)
    validate_netvlad_state(sd)
    return sd


# ---- RIPE (thirdparty/RIPE/ripe: model_zoo/vgg_hyper.py, models/backbones/vgg.py, vgg_utils.py; checkpoint ripe_weights.pth) ------------------
# vgg19_bn().features[:40]: index of every 3x3 convolution in the Sequential (its BatchNorm sits at index + 1), cout, cin; pools at 6, 13, 26, 39
RIPE_ENCODER = [(0, 64, 3), (3, 64, 64), (7, 128, 64), (10, 128, 128), (14, 256, 128), (17, 256, 256), (20, 256, 256), (23, 256, 256),
                (27, 512, 256), (30, 512, 512), (33, 512, 512), (36, 512, 512)]
# ConvRefiner per decoder scale (vgg.py:38-71, mode "dect"): scale, in, hidden, out
RIPE_DECODER = [("8", 512, 512, 257), ("4", 512, 256, 129), ("2", 256, 128, 65), ("1", 128, 64, 2)]
RIPE_HIDDEN_BLOCKS = 8
RIPE_HYPER_DIM, RIPE_DESC_DIM = 960, 256
RIPE_BN_EPS = 1e-5
_RIPE_BN = (("weight", False), ("bias", False), ("running_mean", False), ("running_var", False), ("num_batches_tracked", True))


def _ripe_layout():
    t = []

    def bn(p, c):
        return [(f"{p}.{s}", () if scalar else (c,)) for s, scalar in _RIPE_BN]

    for i, co, ci in RIPE_ENCODER:
        t += [(f"net.encoder.layers.{i}.weight", (co, ci, 3, 3)), (f"net.encoder.layers.{i}.bias", (co,))] + bn(f"net.encoder.layers.{i + 1}", co)
    for s, cin, hid, out in RIPE_DECODER:
        p = f"net.decoder.layers.{s}"
        t += [(f"{p}.block1.0.weight", (hid, cin, 1, 1)), (f"{p}.block1.0.bias", (hid,))] + bn(f"{p}.block1.1", hid)
        t += [(f"{p}.block1.3.weight", (hid, hid, 1, 1)), (f"{p}.block1.3.bias", (hid,))]
        for j in range(RIPE_HIDDEN_BLOCKS):
            q = f"{p}.hidden_blocks.{j}"
            t += [(f"{q}.0.weight", (hid, 1, 5, 5)), (f"{q}.0.bias", (hid,))] + bn(f"{q}.1", hid)
            t += [(f"{q}.3.weight", (hid, hid, 1, 1)), (f"{q}.3.bias", (hid,))]
        t += [(f"{p}.out_conv.weight", (out, hid, 1, 1)), (f"{p}.out_conv.bias", (out,))]
    t += [("conv_dim_reduction_coarse_desc.weight", (RIPE_DESC_DIM, RIPE_HYPER_DIM, 1)), ("conv_dim_reduction_coarse_desc.bias", (RIPE_DESC_DIM,))]
    return t


RIPE_LAYOUT = _ripe_layout()   # (key, shape) of every tensor of vgg_hyper()'s state dict


def validate_ripe_state_dict(sd: Dict[str, torch.Tensor]) -> None:
    """KeyError for a missing / unexpected tensor, ValueError for a wrong shape, a non-finite value or a negative running_var — each naming the
    tensor — before anything native is called.  ``num_batches_tracked`` is accepted and ignored, present or not."""
    table = dict(RIPE_LAYOUT)
    for k, shape in RIPE_LAYOUT:
        if k not in sd:
            if k.endswith("num_batches_tracked"):
                continue
            raise KeyError(f"RIPE: state dict has no tensor {k!r}")
        if k.endswith("num_batches_tracked"):
            continue
        if tuple(sd[k].shape) != tuple(shape):
            raise ValueError(f"RIPE: tensor {k!r} has shape {tuple(sd[k].shape)}, expected {tuple(shape)}")
        if not bool(torch.isfinite(sd[k]).all()):
            raise ValueError(f"RIPE: tensor {k!r} holds a non-finite value")
        if k.endswith("running_var") and not bool((sd[k] >= 0).all()):
            raise ValueError(f"RIPE: tensor {k!r} has a negative entry")
    for k in sd:
        if k not in table:
            raise KeyError(f"RIPE: unexpected tensor {k!r} in the state dict")


def fold_ripe_batchnorm(sd: Dict[str, torch.Tensor], conv: str, bn: str, dtype=torch.float64):
    """(weight, bias) of the convolution ``conv`` with the eval-mode BatchNorm ``bn`` behind it folded in, evaluated in ``dtype``:
    w' = w gamma / sqrt(var + eps) per output channel, b' = (b - mean) gamma / sqrt(var + eps) + beta — what dim_ripe_create does in fp64."""
    sc = sd[f"{bn}.weight"].to(dtype) / torch.sqrt(sd[f"{bn}.running_var"].to(dtype) + RIPE_BN_EPS)
    w = sd[f"{conv}.weight"].to(dtype)
    return w * sc.reshape(-1, *([1] * (w.dim() - 1))), (sd[f"{conv}.bias"].to(dtype) - sd[f"{bn}.running_mean"].to(dtype)) * sc + sd[f"{bn}.bias"].to(dtype)


def synthetic_ripe_state_dict(seed: int = 41, logit_gain: float = 0.035, logit_bias: float = 0.2125) -> Dict[str, torch.Tensor]:
    """Seeded synthetic RIPE weights under the reference's own keys.  He-normal convolutions (the depthwise ones over their 25 taps) with 0.1 N(0, 1)
    biases; BatchNorm running means 0.2 N(0, 1), running variances U(0.5, 1.5), betas 0.1 N(0, 1) and gammas U(0.6, 1.4) of which every seventh
    channel is negated: the statistics are not the identity and a folded scale can be negative.  The pointwise convolution that closes a hidden
    block is scaled by 1 / sqrt(2), so the eight blocks keep the hidden tensor's second moment.  Row 0 of every out_conv (the logit channel) is
    scaled by ``logit_gain`` and biased by ``logit_bias``: the four scales then add up to a heat map whose 3 x 3 maxima lie on both sides of the
    reference's detect threshold 0.5 on noise images."""
    g = torch.Generator().manual_seed(seed)
    sd: Dict[str, torch.Tensor] = {}
    for k, shape in RIPE_LAYOUT:
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(0)
        elif k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(shape, generator=g)
        elif k.endswith("running_mean"):
            sd[k] = 0.2 * torch.randn(shape, generator=g)
        elif len(shape) == 1 and k.endswith(".weight"):   # only a BatchNorm has a one-dimensional weight
            gamma = 0.6 + 0.8 * torch.rand(shape, generator=g)
            gamma[3::7] *= -1.0
            sd[k] = gamma
        elif len(shape) == 1:
            sd[k] = 0.1 * torch.randn(shape, generator=g)
        else:
            fan_in = shape[1] * (shape[2] * shape[3] if len(shape) == 4 else 1)
            sd[k] = torch.randn(shape, generator=g) * math.sqrt(2.0 / fan_in)
            if ".hidden_blocks." in k and k.endswith(".3.weight"):
                sd[k] *= math.sqrt(0.5)
    for s, *_ in RIPE_DECODER:
        sd[f"net.decoder.layers.{s}.out_conv.weight"][0] *= logit_gain
        sd[f"net.decoder.layers.{s}.out_conv.bias"][0] = logit_bias
    return sd


def load_ripe_state_dict(path: str | None = None, seed: int = 41, allow_synthetic: bool = False) -> Dict[str, torch.Tensor]:
    """ripe_weights.pth (the state dict model_zoo/vgg_hyper.py loads into RIPE(VGG, HyperColumnFeatures)), validated against RIPE_LAYOUT.
    ``path``: a file name or an open binary file."""
    if path is None:
        _no_weights("RIPE (ripe_weights.pth, thirdparty/RIPE/ripe/model_zoo/vgg_hyper.py)", "DIM_RIPE_WEIGHTS", allow_synthetic)
        return synthetic_ripe_state_dict(seed)
    sd = torch.load(path if hasattr(path, "read") else str(Path(path)), map_location="cpu")
    sd = {k: (v.float().contiguous() if v.is_floating_point() else v) for k, v in sd.items()}
    validate_ripe_state_dict(sd)
    return sd
