"""Thin host wrapper around the dim_xfeat_* C ABI (one resident XFeat extractor handle)."""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import torch

from . import capi
from .weights import XFEAT_BASIC, validate_xfeat_state_dict

_F = ctypes.c_void_p
_NB = len(XFEAT_BASIC)
_BIASED = [("skip_w", "skip1.1.weight"), ("skip_b", "skip1.1.bias"), ("fusion_w", "block_fusion.2.weight"), ("fusion_b", "block_fusion.2.bias"),
           ("heat_w", "heatmap_head.2.weight"), ("heat_b", "heatmap_head.2.bias"), ("kp_w", "keypoint_head.3.weight"), ("kp_b", "keypoint_head.3.bias")]


class _XfWeights(ctypes.Structure):
    _fields_ = [("basic_w", _F * _NB), ("basic_mean", _F * _NB), ("basic_var", _F * _NB)] + [(n, _F) for n, _ in _BIASED]


class _XfConfig(ctypes.Structure):
    _fields_ = [("top_k", ctypes.c_int), ("detection_threshold", ctypes.c_float), ("desc_stride", ctypes.c_int)]


def declare(lib) -> None:
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.dim_xfeat_create.argtypes = [ctypes.POINTER(_XfWeights), ctypes.POINTER(_XfConfig), ci, ci, ci, ci, ctypes.POINTER(vp)]
    lib.dim_xfeat_create.restype = ci
    lib.dim_xfeat_destroy.argtypes = [vp]
    lib.dim_xfeat_destroy.restype = None
    lib.dim_xfeat_extract.argtypes = [vp, vp, ci, ci, ci, ci, vp, vp, vp, vp, vp]
    lib.dim_xfeat_extract.restype = ci
    lib.dim_xfeat_debug_buffers.argtypes = [vp] + [ctypes.POINTER(vp)] * 4 + [ctypes.POINTER(ci)] * 2
    lib.dim_xfeat_debug_buffers.restype = ci
    lib.dim_op_xfeat_select_workspace_bytes.argtypes = [ci, ci, ci, ci]
    lib.dim_op_xfeat_select_workspace_bytes.restype = ctypes.c_size_t
    lib.dim_op_xfeat_select.argtypes = [vp, vp, ci, ci, ci, ctypes.c_float, ci, ci, vp, vp, vp, vp, vp]
    lib.dim_op_xfeat_select.restype = ci


class XFeatHIP(capi.ResidentHandle):
    """Resident XFeat (sparse detectAndCompute) on one GPU.  cfg keys: top_k (XFeatExtractor's max_num_keypoints), detection_threshold
    (0.05, the network's default: the reference's wrapper never hands its own on), desc_stride (floats per descriptor row, 0 = 64, a multiple
    of 4 up to 128; the extra columns are zeros).
    Arithmetic: "fp16x3" (default) runs the trunk convolutions as fp16 splits on the matrix cores; XFeat has no bf16 split path, so "bf16x6"
    AND "fp32" (and the range guard's re-run) both take the fp32 MFMA kernels.  The stem, the head tails and the samplers are fp32 in every mode."""

    _destroy = "dim_xfeat_destroy"
    default_config = {"top_k": 4096, "detection_threshold": 0.05, "desc_stride": 0}

    def __init__(self, state_dict: Dict[str, torch.Tensor], cfg: Optional[dict] = None, max_batch: int = 1, max_hw=(1024, 1024),
                 capacity: Optional[int] = None, device="cuda", lib=None):
        self.cfg = {**self.default_config, **(cfg or {})}
        on_sat, arith = self.cfg.pop("on_saturation", "fallback"), self.cfg.pop("arithmetic", None)
        validate_xfeat_state_dict(state_dict)
        self._open(device, lib, on_sat, arith)
        declare(self.lib)
        w = _XfWeights()
        for i, (p, *_r) in enumerate(XFEAT_BASIC):
            w.basic_w[i] = self._host(state_dict[p + ".layer.0.weight"])
            w.basic_mean[i] = self._host(state_dict[p + ".layer.1.running_mean"])
            w.basic_var[i] = self._host(state_dict[p + ".layer.1.running_var"])
        for f, k in _BIASED:
            setattr(w, f, self._host(state_dict[k]))
        self.dim = 64
        self.desc_stride = int(self.cfg["desc_stride"]) or self.dim
        top_k = int(self.cfg["top_k"])
        self.capacity = int(capacity if capacity is not None else top_k)
        c = _XfConfig(top_k, float(self.cfg["detection_threshold"]), int(self.cfg["desc_stride"]))
        self.max_batch, self.max_hw = int(max_batch), (int(max_hw[0]), int(max_hw[1]))
        self._last = (1, 0, 0)
        self._create(self.lib.dim_xfeat_create, ctypes.byref(w), ctypes.byref(c), self.max_batch, self.max_hw[0], self.max_hw[1], self.capacity)

    @torch.no_grad()
    def extract_batch(self, images: torch.Tensor, out=None):
        """images [B,H,W,C] float32 (C = 1 or 3, any scale: the network normalises every image) on self.device -> device tensors
        (kpts [B,cap,2], scores [B,cap], desc [B,cap,desc_stride], n [B] int32); no host sync.  Rows at or past n are not written.
        ``out`` = a tuple of such tensors to write into."""
        assert images.dim() == 4 and images.shape[3] in (1, 3) and images.dtype == torch.float32 and images.is_contiguous()
        B, H, W, C = images.shape
        dev = images.device
        if out is not None:
            kp, sc, de, n = out
        else:
            kp = torch.empty(B, self.capacity, 2, dtype=torch.float32, device=dev)
            sc = torch.empty(B, self.capacity, dtype=torch.float32, device=dev)
            de = torch.empty(B, self.capacity, self.desc_stride, dtype=torch.float32, device=dev)
            n = torch.zeros(B, dtype=torch.int32, device=dev)
        with self._ctx():
            capi.check(self.lib, self.lib.dim_xfeat_extract(self._h, capi.ptr(images), B, H, W, C, capi.ptr(kp), capi.ptr(sc), capi.ptr(de), capi.ptr(n),
                                                            self._stream()))
        self._last = (B, H // 32 * 32, W // 32 * 32)
        return kp, sc, de, n

    def extract_batch_guarded(self, images: torch.Tensor, logger=None):
        """extract_batch under the fp16x3 range guard (capi.run_guarded): the trunk runs as fp16 splits on the matrix cores (nhwc_conv.hip), exact for
        |activation| <= 4094; a call that leaves that range is repeated on the fp32 MFMA path.  Synchronises."""
        return self.guarded(lambda: self.extract_batch(images), "XFeat", logger)

    @torch.no_grad()
    def __call__(self, image: torch.Tensor) -> dict:
        """image [1,C,H,W] float, any scale.  Returns the reference's feature dict for one image (device tensors): keypoints (N,2), scores (N,),
        descriptors (N,D) with D = desc_stride — rows, NOT transposed (extractors/xfeat.py)."""
        img = image[0].permute(1, 2, 0).contiguous().to(self.device, torch.float32)[None]
        kp, sc, de, n = self.extract_batch_guarded(img)
        k = int(n[0].item())
        return {"keypoints": kp[0, :k], "scores": sc[0, :k], "descriptors": de[0, :k]}

    def debug_taps(self) -> dict:
        """Of the last call: the normalised image and the keypoint heat map K1h [B,_H,_W], the reliability map H1 [B,_H/8,_W/8], the L2-normalised
        dense descriptors M1 [B,_H/8,_W/8,64], and the resized frame's size (_H, _W)."""
        p = [ctypes.c_void_p() for _ in range(4)]
        hr, wr = ctypes.c_int(), ctypes.c_int()
        capi.check(self.lib, self.lib.dim_xfeat_debug_buffers(self._h, *[ctypes.byref(q) for q in p], ctypes.byref(hr), ctypes.byref(wr)))
        B, H, W = self._last[0], hr.value, wr.value
        cp = lambda q, shape: capi.copy_from_device(self.lib, q.value, shape, self.device)  # noqa: E731
        return {"norm": cp(p[0], (B, H, W)), "K1h": cp(p[1], (B, H, W)), "H1": cp(p[2], (B, H // 8, W // 8)), "M1": cp(p[3], (B, H // 8, W // 8, 64)),
                "hw": (H, W)}
