"""Thin host wrapper around the dim_alike_* C ABI (one resident ALIKE extractor handle)."""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import torch

from . import capi
from .weights import ALIKE_BN, ALIKE_CFGS, validate_alike_state_dict

_F = ctypes.c_void_p
_CONVS = [("block1_conv1", "block1.conv1.weight"), ("block1_conv2", "block1.conv2.weight"), ("block2_conv1", "block2.conv1.weight"),
          ("block2_conv2", "block2.conv2.weight"), ("block3_conv1", "block3.conv1.weight"), ("block3_conv2", "block3.conv2.weight"),
          ("block4_conv1", "block4.conv1.weight"), ("block4_conv2", "block4.conv2.weight")]
_TAIL = [("block2_ds_w", "block2.downsample.weight"), ("block2_ds_b", "block2.downsample.bias"),
         ("block3_ds_w", "block3.downsample.weight"), ("block3_ds_b", "block3.downsample.bias"),
         ("block4_ds_w", "block4.downsample.weight"), ("block4_ds_b", "block4.downsample.bias"),
         ("conv1", "conv1.weight"), ("conv2", "conv2.weight"), ("conv3", "conv3.weight"), ("conv4", "conv4.weight"),
         ("convhead1", "convhead1.weight"), ("convhead2", "convhead2.weight")]


class _AkWeights(ctypes.Structure):
    _fields_ = [(n, _F) for n, _ in _CONVS] + [("bn_weight", _F * 8), ("bn_bias", _F * 8), ("bn_mean", _F * 8), ("bn_var", _F * 8)] + \
               [(n, _F) for n, _ in _TAIL]


class _AkConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("c1", "c2", "c3", "c4", "dim", "single_head", "radius", "top_k")] + \
               [("scores_th", ctypes.c_double), ("n_limit", ctypes.c_int), ("desc_stride", ctypes.c_int)]


def declare(lib) -> None:
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.dim_alike_create.argtypes = [ctypes.POINTER(_AkWeights), ctypes.POINTER(_AkConfig), ci, ci, ci, ci, ctypes.POINTER(vp)]
    lib.dim_alike_create.restype = ci
    lib.dim_alike_destroy.argtypes = [vp]
    lib.dim_alike_destroy.restype = None
    lib.dim_alike_extract.argtypes = [vp, vp, ci, ci, ci, vp, vp, vp, vp, vp]
    lib.dim_alike_extract.restype = ci
    lib.dim_alike_debug_buffers.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(ci), ctypes.POINTER(ci)]
    lib.dim_alike_debug_buffers.restype = ci


class AlikeHIP(capi.ResidentHandle):
    """Resident ALIKE on one GPU.  cfg keys follow AlikeExtractor._default_conf (extractors/alike.py:9-17): model, top_k, scores_th,
    n_limit; plus desc_stride (floats per descriptor row, 0 = the model's dim, at most 128; the extra columns are zeros).
    Arithmetic: "fp16x3" (default) runs the convolutions and head products as fp16 splits on the matrix cores; ALIKE has no bf16 split path, so
    "bf16x6" AND "fp32" (and the range guard's re-run) both take the fp32 MFMA kernels."""

    _destroy = "dim_alike_destroy"
    default_config = {"model": "alike-s", "top_k": 15000, "scores_th": 0.2, "n_limit": 15000, "desc_stride": 0}

    def __init__(self, state_dict: Dict[str, torch.Tensor], cfg: Optional[dict] = None, max_batch: int = 1, max_hw=(1024, 1024),
                 capacity: Optional[int] = None, device="cuda", lib=None):
        self.cfg = {**self.default_config, **(cfg or {})}
        on_sat, arith = self.cfg.pop("on_saturation", "fallback"), self.cfg.pop("arithmetic", None)
        model = self.cfg["model"]
        if model not in ALIKE_CFGS:
            raise ValueError(f"unknown ALIKE model {model!r}; expected one of {sorted(ALIKE_CFGS)}")
        validate_alike_state_dict(state_dict, model)
        self._open(device, lib, on_sat, arith)
        declare(self.lib)
        geo = ALIKE_CFGS[model]
        w = _AkWeights()
        for f, k in _CONVS + _TAIL:
            setattr(w, f, self._host(state_dict[k]) if k in state_dict else None)
        for i, b in enumerate(ALIKE_BN):
            w.bn_weight[i] = self._host(state_dict[b + ".weight"])
            w.bn_bias[i] = self._host(state_dict[b + ".bias"])
            w.bn_mean[i] = self._host(state_dict[b + ".running_mean"])
            w.bn_var[i] = self._host(state_dict[b + ".running_var"])
        self.dim = int(geo[4])
        self.desc_stride = int(self.cfg["desc_stride"]) or self.dim
        top_k, n_limit = int(self.cfg["top_k"]), int(self.cfg["n_limit"])
        self.capacity = int(capacity if capacity is not None else (top_k if top_k > 0 else n_limit))
        c = _AkConfig(*geo, top_k, float(self.cfg["scores_th"]), n_limit, int(self.cfg["desc_stride"]))
        self.max_batch, self.max_hw = int(max_batch), (int(max_hw[0]), int(max_hw[1]))
        self._last = (1, 0, 0)
        self._create(self.lib.dim_alike_create, ctypes.byref(w), ctypes.byref(c), self.max_batch, self.max_hw[0], self.max_hw[1], self.capacity)

    @torch.no_grad()
    def extract_batch(self, images: torch.Tensor, out=None):
        """images [B,H,W,3] float32 in [0,1] on self.device -> device tensors (kpts [B,cap,2], scores [B,cap], desc [B,cap,desc_stride],
        n [B] int32); no host sync.  Descriptor rows at or past n are not written.  ``out`` = a tuple of such tensors to write into."""
        assert images.dim() == 4 and images.shape[3] == 3 and images.dtype == torch.float32 and images.is_contiguous()
        B, H, W, _ = images.shape
        dev = images.device
        if out is not None:
            kp, sc, de, n = out
        else:
            kp = torch.empty(B, self.capacity, 2, dtype=torch.float32, device=dev)
            sc = torch.empty(B, self.capacity, dtype=torch.float32, device=dev)
            de = torch.empty(B, self.capacity, self.desc_stride, dtype=torch.float32, device=dev)
            n = torch.zeros(B, dtype=torch.int32, device=dev)
        with self._ctx():
            capi.check(self.lib, self.lib.dim_alike_extract(self._h, capi.ptr(images), B, H, W, capi.ptr(kp), capi.ptr(sc), capi.ptr(de), capi.ptr(n),
                                                            self._stream()))
        self._last = (B, H, W)
        return kp, sc, de, n

    def extract_batch_guarded(self, images: torch.Tensor, logger=None):
        """extract_batch under the fp16x3 range guard (capi.run_guarded): the convolutions and head products run as fp16 splits on the
        matrix cores (nhwc_conv.hip, gemm_x6.hip), exact for |activation| <= 4094; a call that leaves that range is repeated on the fp32
        paths.  Synchronises."""
        return self.guarded(lambda: self.extract_batch(images), "ALIKE", logger)

    @torch.no_grad()
    def __call__(self, image: torch.Tensor) -> dict:
        """image [1,3,H,W] float in [0,1].  Returns the reference's feature dict for one image (device tensors): keypoints (N,2),
        scores (N,), descriptors (D,N) with D = desc_stride (extractors/alike.py:39-44)."""
        img = image[0].permute(1, 2, 0).contiguous().to(self.device, torch.float32)[None]
        kp, sc, de, n = self.extract_batch_guarded(img)
        k = int(n[0].item())
        return {"keypoints": kp[0, :k], "scores": sc[0, :k], "descriptors": de[0, :k].t()}

    def debug_taps(self) -> dict:
        """Score map and border-cleared NMS map [B,H,W] of the last call, and the padded frame's size."""
        p1, p2, hp, wp = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int(), ctypes.c_int()
        capi.check(self.lib, self.lib.dim_alike_debug_buffers(self._h, ctypes.byref(p1), ctypes.byref(p2), ctypes.byref(hp), ctypes.byref(wp)))
        return {"score_map": capi.copy_from_device(self.lib, p1.value, self._last, self.device),
                "nms_map": capi.copy_from_device(self.lib, p2.value, self._last, self.device), "hp_wp": (hp.value, wp.value)}
