"""Thin host wrapper around the dim_sp_* C ABI (one resident extractor handle).

Host code only allocates tensors and passes raw pointers; all compute is in
libdim_hip.so.  ``lib``/``device`` are injectable so the CPU tests can drive the very
same sources through the test-only emulator build; the product default is the
gfx950 library on ``cuda`` and there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import torch

from . import capi
from .weights import SP_LAYERS, SPO_BLOCKS, SPO_BN_EPS, validate_superpoint_open_state_dict


class _SpWeights(ctypes.Structure):
    _fields_ = [("conv_w", ctypes.c_void_p * 12), ("conv_b", ctypes.c_void_p * 12)]


class _SpConfig(ctypes.Structure):
    _fields_ = [
        ("nms_radius", ctypes.c_int),
        ("keypoint_threshold", ctypes.c_float),
        ("max_keypoints", ctypes.c_int),
        ("remove_borders", ctypes.c_int),
        ("fix_sampling", ctypes.c_int),
    ]


class SuperPointHIP(capi.ResidentHandle):
    """Resident SuperPoint on one GPU.  cfg keys follow SPN:112-118 (+ fix_sampling)."""

    _destroy = "dim_sp_destroy"
    default_config = {"nms_radius": 4, "keypoint_threshold": 0.005, "max_keypoints": -1, "remove_borders": 4,
                      "fix_sampling": False}

    def __init__(self, state_dict: Dict[str, torch.Tensor], cfg: Optional[dict] = None, max_batch: int = 1,
                 max_hw=(1024, 1024), capacity: Optional[int] = None, device="cuda", lib=None, on_saturation: str = "fallback", arithmetic=None):
        self.cfg = {**self.default_config, **(cfg or {})}
        mk = self.cfg["max_keypoints"]
        if mk == 0 or mk < -1:
            raise ValueError('"max_keypoints" must be positive or "-1"')  # SPN:152-154
        self._open(device, lib, on_saturation, arithmetic)
        self.max_batch, self.max_hw = int(max_batch), (int(max_hw[0]), int(max_hw[1]))
        self.capacity = int(capacity if capacity is not None else (mk if mk > 0 else 8192))
        w = _SpWeights()
        for i, (name, *_ ) in enumerate(SP_LAYERS):
            w.conv_w[i] = self._host(state_dict[name + ".weight"])
            w.conv_b[i] = self._host(state_dict[name + ".bias"])
        c = _SpConfig(int(self.cfg["nms_radius"]), float(self.cfg["keypoint_threshold"]), int(mk),
                      int(self.cfg["remove_borders"]), int(bool(self.cfg["fix_sampling"])))
        self._create(self.lib.dim_sp_create, ctypes.byref(w), ctypes.byref(c), self.max_batch, self.max_hw[0], self.max_hw[1], self.capacity)

    def candidate_counts(self, batch: int) -> torch.Tensor:
        """NMS survivors above threshold / border per image of the last call, BEFORE top-k / the capacity
        cut (host int32 tensor; synchronises).  > capacity in keep-all mode (max_keypoints = -1) means the call
        dropped keypoints the reference would return: re-create the handle with a larger capacity."""
        p = ctypes.c_void_p()
        capi.check(self.lib, self.lib.dim_sp_candidate_counts(self._h, ctypes.byref(p)))
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
            out = torch.empty(batch, dtype=torch.int32, device=self.device)
            rc = ctypes.CDLL("libamdhip64.so").hipMemcpy(ctypes.c_void_p(out.data_ptr()), p, ctypes.c_size_t(batch * 4), 3)
            if rc != 0:
                raise capi.DimHipError(f"hipMemcpy failed: {rc}")
            return out.cpu()
        return torch.frombuffer((ctypes.c_int32 * batch).from_address(p.value), dtype=torch.int32).clone()

    def desc_rows(self, batch: int):
        """How the last call ran the descriptor head (dim_sp_desc_rows; synchronises): None when it ran on the whole map, otherwise
        (slots, n_rows) — the rows reserved per image and a host int32 tensor [batch] with the number of distinct cells the keypoints sample."""
        p, slots = ctypes.c_void_p(), ctypes.c_int()
        capi.check(self.lib, self.lib.dim_sp_desc_rows(self._h, ctypes.byref(p), ctypes.byref(slots)))
        if slots.value == 0:
            return None
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
            out = torch.empty(batch, dtype=torch.int32, device=self.device)
            rc = ctypes.CDLL("libamdhip64.so").hipMemcpy(ctypes.c_void_p(out.data_ptr()), p, ctypes.c_size_t(batch * 4), 3)
            if rc != 0:
                raise capi.DimHipError(f"hipMemcpy failed: {rc}")
            return slots.value, out.cpu()
        return slots.value, torch.frombuffer((ctypes.c_int32 * batch).from_address(p.value), dtype=torch.int32).clone()

    @torch.no_grad()
    def extract_batch(self, images: torch.Tensor, out=None):
        """images [B,H,W] float32 in [0,1] on self.device.  Returns device tensors
        (kpts [B,cap,2], scores [B,cap], desc [B,cap,256], n [B] int32); no host sync.
        ``out`` = a previously returned tuple to write into (no allocation: needed when the call is
        issued on a side stream)."""
        assert images.dim() == 3 and images.dtype == torch.float32 and images.is_contiguous()
        B, H, W = images.shape
        dev = images.device
        if out is not None:
            kp, sc, de, n = out
        else:
            kp = torch.empty(B, self.capacity, 2, dtype=torch.float32, device=dev)
            sc = torch.empty(B, self.capacity, dtype=torch.float32, device=dev)
            de = torch.empty(B, self.capacity, 256, dtype=torch.float32, device=dev)
            n = torch.zeros(B, dtype=torch.int32, device=dev)
        with self._ctx():
            capi.check(self.lib, self.lib.dim_sp_extract(self._h, capi.ptr(images), B, H, W, capi.ptr(kp), capi.ptr(sc),
                                                         capi.ptr(de), capi.ptr(n), self._stream()))
        return kp, sc, de, n

    def extract_batch_guarded(self, images: torch.Tensor, out=None, logger=None):
        """extract_batch under the fp16x3 range guard (capi.run_guarded): synchronises."""
        return self.guarded(lambda: self.extract_batch(images, out=out), "SuperPoint", logger)

    @torch.no_grad()
    def __call__(self, image: torch.Tensor) -> dict:
        """image [1,1,H,W] (the reference's input, SPN:158).  Returns the reference's dict
        for one image with tensors on the device: keypoints (N,2), scores (N,), descriptors (256,N)."""
        img = image.reshape(image.shape[-2], image.shape[-1])[None].contiguous().to(self.device, torch.float32)
        kp, sc, de, n = self.extract_batch_guarded(img)
        k = int(n[0].item())
        return {"keypoints": kp[0, :k], "scores": sc[0, :k], "descriptors": de[0, :k].t()}

    def debug_taps(self, batch: int = 1) -> dict:
        """Intermediate tensors of the last call as CPU copies (parity tests)."""
        ptrs = [ctypes.c_void_p() for _ in range(5)]
        h8, w8 = ctypes.c_int(), ctypes.c_int()
        capi.check(self.lib, self.lib.dim_sp_debug_buffers(self._h, *[ctypes.byref(p) for p in ptrs], ctypes.byref(h8), ctypes.byref(w8)))
        H8, W8 = h8.value, w8.value
        h, w = H8 // 8, W8 // 8
        shapes = {"encoder": (batch, h, w, 128), "logits": (batch, h * w, 65), "score_map": (batch, H8, W8),
                  "nms_map": (batch, H8, W8), "dense_desc": (batch, h, w, 256)}
        out = {}
        for (name, shape), p in zip(shapes.items(), ptrs):
            out[name] = capi.copy_from_device(self.lib, p.value, shape, self.device)
        return out

    def debug_conv1b(self, batch: int, H: int, W: int) -> torch.Tensor:
        """conv1b's pooled output of the last call as a CPU tensor [batch, H/2, W/2, 64] (fp32 NHWC): dim_sp_debug_conv1b."""
        p, h2, w2 = ctypes.c_void_p(), ctypes.c_int(), ctypes.c_int()
        capi.check(self.lib, self.lib.dim_sp_debug_conv1b(self._h, int(batch), int(H), int(W), ctypes.byref(p), ctypes.byref(h2), ctypes.byref(w2)))
        return capi.copy_from_device(self.lib, p.value, (batch, h2.value, w2.value, 64), self.device)


class _SpoWeights(ctypes.Structure):
    """include/dim_hip.h: dim_spo_weights."""
    _fields_ = [(n, ctypes.c_void_p * 12) for n in ("conv_w", "conv_b", "bn_gamma", "bn_beta", "bn_mean", "bn_var")] + [("bn_eps", ctypes.c_double)]


class SuperPointOpenHIP(SuperPointHIP):
    """Resident open SuperPoint (thirdparty/SuperPoint_open/superpoint_pytorch.py) on one GPU: dim_spo_create returns an ordinary dim_sp handle, so
    extract_batch, the guard, the debug taps and candidate_counts are the base class's.  ``state_dict`` in the checkpoint's key layout
    (weights.load_superpoint_open_state_dict); cfg keys as SuperPointHIP — fix_sampling is always on (the network has the one sampler), and
    max_keypoints = -1 keeps every keypoint (the reference network would raise inside torch.topk)."""

    default_config = {**SuperPointHIP.default_config, "fix_sampling": True}

    def __init__(self, state_dict: Dict[str, torch.Tensor], cfg: Optional[dict] = None, max_batch: int = 1,
                 max_hw=(1024, 1024), capacity: Optional[int] = None, device="cuda", lib=None, on_saturation: str = "fallback", arithmetic=None):
        validate_superpoint_open_state_dict(state_dict)   # KeyError / ValueError naming the tensor, before any native call
        self.cfg = {**self.default_config, **(cfg or {}), "fix_sampling": True}
        mk = self.cfg["max_keypoints"]
        if mk == 0 or mk < -1:
            raise ValueError('"max_keypoints" must be positive or "-1"')
        if arithmetic == "fp32":
            raise ValueError("SuperPointOpenHIP: the BatchNorm epilogue exists in the fp16x3 / bf16x6 arithmetic only")
        self._open(device, lib, on_saturation, arithmetic)
        self.max_batch, self.max_hw = int(max_batch), (int(max_hw[0]), int(max_hw[1]))
        self.capacity = int(capacity if capacity is not None else (mk if mk > 0 else 8192))
        w = _SpoWeights()
        for i, blk in enumerate(SPO_BLOCKS):
            w.conv_w[i] = self._host(state_dict[blk + ".conv.weight"])
            w.conv_b[i] = self._host(state_dict[blk + ".conv.bias"])
            w.bn_gamma[i] = self._host(state_dict[blk + ".bn.weight"])
            w.bn_beta[i] = self._host(state_dict[blk + ".bn.bias"])
            w.bn_mean[i] = self._host(state_dict[blk + ".bn.running_mean"])
            w.bn_var[i] = self._host(state_dict[blk + ".bn.running_var"])
        w.bn_eps = SPO_BN_EPS
        c = _SpConfig(int(self.cfg["nms_radius"]), float(self.cfg["keypoint_threshold"]), int(mk), int(self.cfg["remove_borders"]), 1)
        self.lib.dim_spo_create.restype = ctypes.c_int
        self._create(self.lib.dim_spo_create, ctypes.byref(w), ctypes.byref(c), self.max_batch, self.max_hw[0], self.max_hw[1], self.capacity)
