"""Thin host wrapper around the dim_ripe_* C ABI (one resident RIPE extractor handle) and the operator entries of its kernels."""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import torch

from . import capi
from .weights import RIPE_DECODER, RIPE_ENCODER, RIPE_HIDDEN_BLOCKS, validate_ripe_state_dict

_F = ctypes.c_void_p
_NB = RIPE_HIDDEN_BLOCKS
DESC_DIM, HYPER_DIM = 256, 960
LEVEL_CHANNELS = (64, 128, 256, 512)


class _ConvBn(ctypes.Structure):
    _fields_ = [(n, _F) for n in ("w", "b", "gamma", "beta", "mean", "var")]


class _Refiner(ctypes.Structure):
    _fields_ = [("block1_0", _ConvBn), ("block1_3_w", _F), ("block1_3_b", _F), ("dw", _ConvBn * _NB), ("pw_w", _F * _NB), ("pw_b", _F * _NB),
                ("out_w", _F), ("out_b", _F)]


class _RipeWeights(ctypes.Structure):
    _fields_ = [("enc", _ConvBn * len(RIPE_ENCODER)), ("dec", _Refiner * len(RIPE_DECODER)), ("desc_w", _F), ("desc_b", _F)]


def declare(lib) -> None:
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.dim_ripe_create.argtypes = [ctypes.POINTER(_RipeWeights), ci, ci, ci, ci, ctypes.POINTER(vp)]
    lib.dim_ripe_create.restype = ci
    lib.dim_ripe_destroy.argtypes = [vp]
    lib.dim_ripe_destroy.restype = None
    lib.dim_ripe_extract.argtypes = [vp, vp, ci, ci, ci, ci, cf, vp, vp, vp, vp, vp]
    lib.dim_ripe_extract.restype = ci
    lib.dim_ripe_debug_buffers.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp * 4), ctypes.POINTER(ci * 4), ctypes.POINTER(ci * 4), ctypes.POINTER(ci)]
    lib.dim_ripe_debug_buffers.restype = ci
    lib.dim_op_ripe_dw5x5_f32.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, vp]
    lib.dim_op_ripe_dw5x5_f32.restype = ci
    lib.dim_op_ripe_resize_bilinear_f32.argtypes = [vp, ci, ci, ci, ci, ci, ci, vp, ci, ci, vp]
    lib.dim_op_ripe_resize_bilinear_f32.restype = ci
    lib.dim_op_ripe_nms3_f32.argtypes = [vp, vp, cf, ci, ci, ci, vp]
    lib.dim_op_ripe_nms3_f32.restype = ci
    lib.dim_op_ripe_hypercolumn_f32.argtypes = [ctypes.POINTER(vp * 4), ctypes.POINTER(ci * 4), ctypes.POINTER(ci * 4), vp, vp, vp, ci, ci, ci, ci, vp]
    lib.dim_op_ripe_hypercolumn_f32.restype = ci


def _lib(lib):
    lib = lib if lib is not None else capi.load()
    declare(lib)
    return lib


def dw5x5(x: torch.Tensor, w_25c: torch.Tensor, bias: torch.Tensor, lib=None) -> torch.Tensor:
    """dim_op_ripe_dw5x5_f32: x [B, H, W, C], w_25c [25, C] (tap 5 dy + dx, BatchNorm folded), bias [C] -> relu(depthwise 5 x 5 + bias) [B, H, W, C]."""
    lib = _lib(lib)
    B, H, W, C = x.shape
    out = torch.empty_like(x)
    with capi.device_ctx(x.device):
        capi.check(lib, lib.dim_op_ripe_dw5x5_f32(capi.ptr(x.contiguous()), capi.ptr(w_25c.contiguous()), capi.ptr(bias.contiguous()), capi.ptr(out), B, H, W, C,
                                                  capi.stream_ptr(x.device)))
    return out


def resize_bilinear(x: torch.Tensor, size, c_off: int = 0, channels: Optional[int] = None, lib=None) -> torch.Tensor:
    """dim_op_ripe_resize_bilinear_f32: channels [c_off, c_off + channels) of x [B, h, w, ld] -> [B, H, W, channels], F.interpolate(bilinear,
    align_corners=False)."""
    lib = _lib(lib)
    B, h, w, ld = x.shape
    C = ld - c_off if channels is None else channels
    out = torch.empty(B, size[0], size[1], C, dtype=torch.float32, device=x.device)
    with capi.device_ctx(x.device):
        capi.check(lib, lib.dim_op_ripe_resize_bilinear_f32(capi.ptr(x.contiguous()), ld, c_off, C, B, h, w, capi.ptr(out), size[0], size[1],
                                                            capi.stream_ptr(x.device)))
    return out


def nms3(heat: torch.Tensor, threshold: float, lib=None) -> torch.Tensor:
    """dim_op_ripe_nms3_f32: heat [B, H, W] -> key map [B, H, W]: heat at the 3 x 3 maxima above the threshold, 0 elsewhere."""
    lib = _lib(lib)
    B, H, W = heat.shape
    key = torch.empty_like(heat)
    with capi.device_ctx(heat.device):
        capi.check(lib, lib.dim_op_ripe_nms3_f32(capi.ptr(heat.contiguous()), capi.ptr(key), ctypes.c_float(threshold), B, H, W, capi.stream_ptr(heat.device)))
    return key


def hypercolumn(maps, kpts: torch.Tensor, n_kpts: torch.Tensor, hw, lib=None) -> torch.Tensor:
    """dim_op_ripe_hypercolumn_f32: maps = four [B, h_l, w_l, 64 << l] tensors, kpts [B, cap, 2] (x, y) float, n_kpts [B] int32, hw = the image's
    (H, W) -> rows [B, cap, 960] (rows past n_kpts[b] zero)."""
    lib = _lib(lib)
    B, cap, _ = kpts.shape
    maps = [m.contiguous() for m in maps]
    rows = torch.zeros(B, cap, HYPER_DIM, dtype=torch.float32, device=kpts.device)
    p = (ctypes.c_void_p * 4)(*[m.data_ptr() for m in maps])
    hs, ws = (ctypes.c_int * 4)(*[m.shape[1] for m in maps]), (ctypes.c_int * 4)(*[m.shape[2] for m in maps])
    with capi.device_ctx(kpts.device):
        capi.check(lib, lib.dim_op_ripe_hypercolumn_f32(ctypes.byref(p), ctypes.byref(hs), ctypes.byref(ws), capi.ptr(kpts.contiguous()), capi.ptr(n_kpts), capi.ptr(rows),
                                                        cap, B, hw[0], hw[1], capi.stream_ptr(kpts.device)))
    return rows


class RipeHIP(capi.ResidentHandle):
    """Resident RIPE (vgg_hyper(): InstanceNorm, VGG19-BN encoder, DeDoDe-style decoder, 3 x 3 maxima, hypercolumn descriptors) on one GPU.
    conf keys: top_k (RIPEExtractor's max_keypoints), threshold (its detect_threshold, >= 0), arithmetic, on_saturation.  Arithmetic: "fp16x3"
    (default) runs the 3 x 3 and 1 x 1 convolutions as fp16 splits on the matrix cores under the range guard; "bf16x6" and "fp32" (and the guard's
    re-run) take the bf16 split, which has no range limit.  The first layer, the depthwise convolutions, the resizes and the samplers are fp32 in
    every mode."""

    _destroy = "dim_ripe_destroy"
    default_config = {"top_k": 4000, "threshold": 0.5}

    def __init__(self, state_dict: Dict[str, torch.Tensor], conf: Optional[dict] = None, max_batch: int = 1, max_hw=(1024, 1024),
                 capacity: Optional[int] = None, device="cuda", lib=None):
        self.conf = {**self.default_config, **(conf or {})}
        on_sat, arith = self.conf.pop("on_saturation", "fallback"), self.conf.pop("arithmetic", None)
        validate_ripe_state_dict(state_dict)
        self._open(device, lib, on_sat, arith)
        declare(self.lib)
        sd = state_dict

        def convbn(dst, conv, bn):
            for f, k in (("w", f"{conv}.weight"), ("b", f"{conv}.bias"), ("gamma", f"{bn}.weight"), ("beta", f"{bn}.bias"), ("mean", f"{bn}.running_mean"),
                         ("var", f"{bn}.running_var")):
                setattr(dst, f, self._host(sd[k]))

        w = _RipeWeights()
        for j, (i, _co, _ci) in enumerate(RIPE_ENCODER):
            convbn(w.enc[j], f"net.encoder.layers.{i}", f"net.encoder.layers.{i + 1}")
        for d, (s, *_r) in enumerate(RIPE_DECODER):
            p, r = f"net.decoder.layers.{s}", w.dec[d]
            convbn(r.block1_0, f"{p}.block1.0", f"{p}.block1.1")
            r.block1_3_w, r.block1_3_b = self._host(sd[f"{p}.block1.3.weight"]), self._host(sd[f"{p}.block1.3.bias"])
            for j in range(_NB):
                q = f"{p}.hidden_blocks.{j}"
                convbn(r.dw[j], f"{q}.0", f"{q}.1")
                r.pw_w[j], r.pw_b[j] = self._host(sd[f"{q}.3.weight"]), self._host(sd[f"{q}.3.bias"])
            r.out_w, r.out_b = self._host(sd[f"{p}.out_conv.weight"]), self._host(sd[f"{p}.out_conv.bias"])
        w.desc_w, w.desc_b = self._host(sd["conv_dim_reduction_coarse_desc.weight"]), self._host(sd["conv_dim_reduction_coarse_desc.bias"])
        self.dim = DESC_DIM
        self.top_k, self.threshold = int(self.conf["top_k"]), float(self.conf["threshold"])
        self.capacity = int(capacity if capacity is not None else self.top_k)
        self.max_batch, self.max_hw = int(max_batch), (int(max_hw[0]), int(max_hw[1]))
        self._create(self.lib.dim_ripe_create, ctypes.byref(w), self.max_batch, self.max_hw[0], self.max_hw[1], self.capacity)

    @torch.no_grad()
    def extract_batch(self, images: torch.Tensor, out=None):
        """images [B,H,W,3] float32 RGB in 0..1 on self.device -> device tensors (kpts [B,cap,2] integer pixels (x, y), scores [B,cap],
        desc [B,cap,256] unit-norm rows, n [B] int32), rows in descending score; no host sync.  n[b] == 0 is the reference's "No keypoints detected"."""
        assert images.dim() == 4 and images.shape[3] == 3 and images.dtype == torch.float32 and images.is_contiguous()
        B, H, W, _ = images.shape
        dev = images.device
        if out is not None:
            kp, sc, de, n = out
        else:
            kp = torch.zeros(B, self.capacity, 2, dtype=torch.float32, device=dev)
            sc = torch.empty(B, self.capacity, dtype=torch.float32, device=dev)
            de = torch.empty(B, self.capacity, DESC_DIM, dtype=torch.float32, device=dev)
            n = torch.zeros(B, dtype=torch.int32, device=dev)
        with self._ctx():
            capi.check(self.lib, self.lib.dim_ripe_extract(self._h, capi.ptr(images), B, H, W, self.top_k, ctypes.c_float(self.threshold), capi.ptr(kp), capi.ptr(sc),
                                                           capi.ptr(de), capi.ptr(n), self._stream()))
        return kp, sc, de, n

    def extract_batch_guarded(self, images: torch.Tensor, logger=None):
        """extract_batch under the fp16x3 range guard (capi.run_guarded): a call in which a stored activation leaves |x| <= 4094 (or a pixel is not
        finite) is repeated with the bf16x6 split.  Synchronises."""
        return self.guarded(lambda: self.extract_batch(images), "RIPE", logger)

    @torch.no_grad()
    def __call__(self, image: torch.Tensor) -> dict:
        """image [1,C,H,W] float in 0..1 (C = 1 is repeated to three channels).  Returns detectAndCompute's tensors for one image (device):
        keypoints (N,2), descriptors (N,256), scores (N,).  RuntimeError("No keypoints detected") as the reference raises it."""
        img = image[0].permute(1, 2, 0).to(self.device, torch.float32)
        if img.shape[2] == 1:
            img = img.repeat(1, 1, 3)
        kp, sc, de, n = self.extract_batch_guarded(img.contiguous()[None])
        k = int(n[0].item())
        if k == 0:
            raise RuntimeError("No keypoints detected")
        return {"keypoints": kp[0, :k], "scores": sc[0, :k], "descriptors": de[0, :k]}

    def debug_taps(self) -> dict:
        """Of the last call: the heat map [B,H,W] and the four encoder maps [B,h_l,w_l,64 << l] (CPU copies)."""
        heat, maps, hs, ws, b = ctypes.c_void_p(), (ctypes.c_void_p * 4)(), (ctypes.c_int * 4)(), (ctypes.c_int * 4)(), ctypes.c_int()
        capi.check(self.lib, self.lib.dim_ripe_debug_buffers(self._h, ctypes.byref(heat), ctypes.byref(maps), ctypes.byref(hs), ctypes.byref(ws), ctypes.byref(b)))
        cp = lambda q, shape: capi.copy_from_device(self.lib, q, shape, self.device)  # noqa: E731
        return {"heat": cp(heat.value, (b.value, hs[0], ws[0])),
                "maps": [cp(maps[l], (b.value, hs[l], ws[l], LEVEL_CHANNELS[l])) for l in range(4)]}
