"""Thin host wrapper around the dim_netvlad_* C ABI (one resident NetVLAD global-descriptor handle)."""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import torch

from . import capi
from .weights import NETVLAD_CONVS, validate_netvlad_state

_F, _Z = ctypes.c_void_p, ctypes.c_size_t
_NL = len(NETVLAD_CONVS)


class _NvWeights(ctypes.Structure):
    _fields_ = [("conv_w", _F * _NL), ("conv_b", _F * _NL), ("conv_w_elems", _Z * _NL), ("conv_b_elems", _Z * _NL),
                ("mean", _F), ("mean_elems", _Z), ("score_w", _F), ("score_w_elems", _Z), ("centers", _F), ("centers_elems", _Z),
                ("whiten_w", _F), ("whiten_w_elems", _Z), ("whiten_b", _F), ("whiten_b_elems", _Z), ("K", ctypes.c_int), ("whiten_out", ctypes.c_int)]


def declare(lib) -> None:
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.dim_netvlad_create.argtypes = [ctypes.POINTER(_NvWeights), ci, ci, ci, ctypes.POINTER(vp)]
    lib.dim_netvlad_create.restype = ci
    lib.dim_netvlad_destroy.argtypes = [vp]
    lib.dim_netvlad_destroy.restype = None
    lib.dim_netvlad_desc_dim.argtypes = [vp]
    lib.dim_netvlad_desc_dim.restype = ci
    lib.dim_netvlad_extract.argtypes = [vp, vp, ci, ci, ci, vp, vp]
    lib.dim_netvlad_extract.restype = ci
    lib.dim_netvlad_debug_buffers.argtypes = [vp, ctypes.POINTER(vp)] + [ctypes.POINTER(ci)] * 3
    lib.dim_netvlad_debug_buffers.restype = ci
    lib.dim_op_netvlad_head_workspace_bytes.argtypes = [ci, ci, ci]
    lib.dim_op_netvlad_head_workspace_bytes.restype = ctypes.c_size_t
    lib.dim_op_netvlad_head_f32.argtypes = [vp, ci, ci, ci, vp, vp, vp, vp, vp]
    lib.dim_op_netvlad_head_f32.restype = ci
    lib.dim_op_netvlad_whiten_workspace_bytes.argtypes = [ci, ci, ci]
    lib.dim_op_netvlad_whiten_workspace_bytes.restype = ctypes.c_size_t
    lib.dim_op_netvlad_whiten_f32.argtypes = [vp, ci, ci, vp, vp, ci, vp, vp, vp]
    lib.dim_op_netvlad_whiten_f32.restype = ci


def netvlad_head(x: torch.Tensor, score_w: torch.Tensor, centers: torch.Tensor, lib=None) -> torch.Tensor:
    """dim_op_netvlad_head_f32: x [b, n, 512] (the conv5_3 map, on the device the library runs on), score_w (K, 512), centers (512, K) as the module
    holds them -> the unit-norm VLAD vectors [b, 512 K]."""
    lib = lib if lib is not None else capi.load()
    declare(lib)
    b, n, _ = x.shape
    K = centers.shape[1]
    dev = x.device
    sdk = score_w.reshape(K, 512).t().contiguous().float().to(dev)
    ckd = centers.t().contiguous().float().to(dev)
    ws = torch.empty(max(1, lib.dim_op_netvlad_head_workspace_bytes(b, n, K) // 4), dtype=torch.float32, device=dev)
    out = torch.empty(b, 512 * K, dtype=torch.float32, device=dev)
    with capi.device_ctx(dev):
        capi.check(lib, lib.dim_op_netvlad_head_f32(capi.ptr(x.contiguous()), b, n, K, capi.ptr(sdk), capi.ptr(ckd), capi.ptr(ws), capi.ptr(out), capi.stream_ptr(dev)))
    return out


def netvlad_whiten(v: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, lib=None) -> torch.Tensor:
    """dim_op_netvlad_whiten_f32: v [b, in], weight (out, in), bias (out) on one device -> normalize(v W^T + b) [b, out]."""
    lib = lib if lib is not None else capi.load()
    declare(lib)
    b, n_in = v.shape
    n_out = weight.shape[0]
    dev = v.device
    ws = torch.empty(max(1, lib.dim_op_netvlad_whiten_workspace_bytes(b, n_in, n_out) // 4), dtype=torch.float32, device=dev)
    out = torch.empty(b, n_out, dtype=torch.float32, device=dev)
    with capi.device_ctx(dev):
        capi.check(lib, lib.dim_op_netvlad_whiten_f32(capi.ptr(v.contiguous()), b, n_in, capi.ptr(weight.contiguous()), capi.ptr(bias.contiguous()), n_out,
                                                      capi.ptr(ws), capi.ptr(out), capi.stream_ptr(dev)))
    return out


class NetVLADHIP(capi.ResidentHandle):
    """Resident NetVLAD (VGG16 features[:-2] -> NetVLAD layer -> whitening) on one GPU.  ``state``: the module's tensors (weights.load_netvlad_mat /
    synthetic_netvlad_state).  conf keys: whiten (True: the whitened descriptor; False: the 512 K VLAD vector, as hloc's conf), arithmetic,
    on_saturation.  Arithmetic: "fp16x3" (default) runs the convolutions as fp16 splits on the matrix cores under the range guard; "bf16x6" and
    "fp32" (and the guard's re-run) take the bf16 split, which has no range limit.  conv1_1, the head and the whitening are fp32 in every mode."""

    _destroy = "dim_netvlad_destroy"
    default_config = {"whiten": True}

    def __init__(self, state: Dict[str, torch.Tensor], conf: Optional[dict] = None, max_batch: int = 1, max_hw=(1024, 1024), device="cuda", lib=None):
        self.conf = {**self.default_config, **(conf or {})}
        on_sat, arith = self.conf.pop("on_saturation", "fallback"), self.conf.pop("arithmetic", None)
        if not self.conf["whiten"]:
            state = {k: v for k, v in state.items() if not k.startswith("whiten.")}
        self.K, wo = validate_netvlad_state(state)
        if self.conf["whiten"] and not wo:
            raise KeyError("NetVLAD: conf asks for whitening and the state has no tensor 'whiten.weight'")
        self._open(device, lib, on_sat, arith)
        declare(self.lib)
        w = _NvWeights()
        for j, (i, _co, _ci) in enumerate(NETVLAD_CONVS):
            w.conv_w[j], w.conv_w_elems[j] = self._host(state[f"backbone.{i}.weight"]), state[f"backbone.{i}.weight"].numel()
            w.conv_b[j], w.conv_b_elems[j] = self._host(state[f"backbone.{i}.bias"]), state[f"backbone.{i}.bias"].numel()
        for f, k in (("mean", "preprocess.mean"), ("score_w", "netvlad.score_proj.weight"), ("centers", "netvlad.centers")) + \
                ((("whiten_w", "whiten.weight"), ("whiten_b", "whiten.bias")) if wo else ()):
            setattr(w, f, self._host(state[k]))
            setattr(w, f + "_elems", state[k].numel())
        w.K, w.whiten_out = self.K, wo
        self.dim = wo if wo else 512 * self.K
        self.max_batch, self.max_hw = int(max_batch), (int(max_hw[0]), int(max_hw[1]))
        self._create(self.lib.dim_netvlad_create, ctypes.byref(w), self.max_batch, self.max_hw[0], self.max_hw[1])

    @torch.no_grad()
    def extract_batch(self, images: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """images [B,H,W,3] float32 RGB in 0..1 on self.device -> unit-norm descriptors [B, dim] on the device; no host sync."""
        assert images.dim() == 4 and images.shape[3] == 3 and images.dtype == torch.float32 and images.is_contiguous()
        B, H, W, _ = images.shape
        if out is None:
            out = torch.empty(B, self.dim, dtype=torch.float32, device=images.device)
        with self._ctx():
            capi.check(self.lib, self.lib.dim_netvlad_extract(self._h, capi.ptr(images), B, H, W, capi.ptr(out), self._stream()))
        return out

    def extract_batch_guarded(self, images: torch.Tensor, logger=None) -> torch.Tensor:
        """extract_batch under the fp16x3 range guard (capi.run_guarded): a call in which a stored activation leaves |x| <= 4094 (or a pixel is NaN)
        is repeated with the bf16x6 split.  Synchronises.  Images must be finite: the re-run reads a NaN pixel as 0 - mean and returns a finite
        descriptor where the reference returns NaN (include/dim_hip.h)."""
        return self.guarded(lambda: self.extract_batch(images), "NetVLAD", logger)

    @torch.no_grad()
    def __call__(self, image: torch.Tensor) -> dict:
        """image [1,3,H,W] float in 0..1 -> {"global_descriptor": [1, dim]} (NV:146)."""
        img = image[0].permute(1, 2, 0).contiguous().to(self.device, torch.float32)[None]
        return {"global_descriptor": self.extract_batch_guarded(img)}

    def debug_map(self) -> torch.Tensor:
        """The conv5_3 map [B, h, w, 512] of the last call (a CPU copy)."""
        p, b, mh, mw = ctypes.c_void_p(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        capi.check(self.lib, self.lib.dim_netvlad_debug_buffers(self._h, ctypes.byref(p), ctypes.byref(b), ctypes.byref(mh), ctypes.byref(mw)))
        return capi.copy_from_device(self.lib, p.value, (b.value, mh.value, mw.value, 512), self.device)
