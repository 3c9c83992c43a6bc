"""Thin host wrapper around the dim_sg_* C ABI: one resident SuperGlue matcher (reference thirdparty/SuperGluePretrainedNetwork/models/
superglue.py, SGN).

The host folds BatchNorm and permutes the attention heads (weights.prepare_superglue_weights, fp64), allocates tensors and passes raw pointers;
all compute is in libdim_hip.so.  ``lib`` / ``device`` are injectable for the CPU emulator tests; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import torch

from . import capi, weights

_F = ctypes.c_void_p
_LAYER_FIELDS = ["q_w", "q_b", "k_w", "k_b", "v_w", "v_b", "merge_w", "merge_b", "mlp0_w", "mlp0_b", "mlp3_w", "mlp3_b"]


class _SgLayer(ctypes.Structure):
    _fields_ = [(n, _F) for n in _LAYER_FIELDS]


class _SgWeights(ctypes.Structure):
    _fields_ = [("kenc_w", _F * 5), ("kenc_b", _F * 5), ("final_proj_w", _F), ("final_proj_b", _F), ("bin_score", ctypes.c_float),
                ("layers", ctypes.POINTER(_SgLayer))]


class _SgConfig(ctypes.Structure):
    _fields_ = [("n_layers", ctypes.c_int), ("descriptor_dim", ctypes.c_int)]


def declare(lib) -> None:
    """Argument / result types of the dim_sg_* entry points (idempotent)."""
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.dim_sg_create.argtypes = [ctypes.POINTER(_SgWeights), ctypes.POINTER(_SgConfig), ci, ci, ctypes.POINTER(vp)]
    lib.dim_sg_create.restype = ci
    lib.dim_sg_destroy.argtypes = [vp]
    lib.dim_sg_destroy.restype = None
    lib.dim_sg_max_kpts.argtypes = [vp]
    lib.dim_sg_max_kpts.restype = ci
    lib.dim_sg_match.argtypes = [vp, vp, vp, vp, vp, vp, ci, vp, ci, ci, cf, vp, vp, vp, vp, vp, vp]
    lib.dim_sg_match.restype = ci
    lib.dim_sg_debug.argtypes = [vp] + [ctypes.POINTER(vp)] * 6
    lib.dim_sg_debug.restype = ci
    lib.dim_sg_sinkhorn.argtypes = [vp, ci, ci, ci, vp]
    lib.dim_sg_sinkhorn.restype = ci
    lib.dim_sg_select.argtypes = [vp, ci, ci, cf, vp, vp, vp, vp, vp, vp]
    lib.dim_sg_select.restype = ci


class SuperGlueHIP(capi.ResidentHandle):
    """Resident SuperGlue on one GPU.  conf keys follow SuperGlue.default_config (SGN:212-219): ``sinkhorn_iterations`` (100) and
    ``match_threshold`` (0.2) are read at every call; the layer count comes from the state dict."""

    _destroy = "dim_sg_destroy"
    default_conf = {"descriptor_dim": 256, "sinkhorn_iterations": 100, "match_threshold": 0.2}

    def __init__(self, state_dict: Dict[str, torch.Tensor], conf: Optional[dict] = None, max_pairs: int = 1, max_kpts: int = 2048,
                 device="cuda", lib=None, on_saturation: str = "fallback", arithmetic=None):
        self.conf = {**self.default_conf, **(conf or {})}
        self._open(device, lib, on_saturation, arithmetic)
        declare(self.lib)
        n_layers = weights.superglue_n_layers(state_dict)
        if int(self.conf["descriptor_dim"]) == 256 and n_layers > 0 and n_layers % 2 == 0:
            prep = weights.prepare_superglue_weights(state_dict)
            host = lambda name: self._host(prep[name])
            layers = (_SgLayer * n_layers)()
            for i in range(n_layers):
                for f in _LAYER_FIELDS:
                    setattr(layers[i], f, host(f"{i}.{f}"))
            w = _SgWeights()
            for s in range(5):
                w.kenc_w[s], w.kenc_b[s] = host(f"kenc.{s}.w"), host(f"kenc.{s}.b")
            w.final_proj_w, w.final_proj_b = host("final_proj.w"), host("final_proj.b")
            w.bin_score = float(prep["bin_score"])
            w.layers = layers
        else:   # the library rejects the shape with its own text
            w = _SgWeights()
        self.n_layers = n_layers
        c = _SgConfig(n_layers, int(self.conf["descriptor_dim"]))
        self.max_pairs = int(max_pairs)
        self._create(self.lib.dim_sg_create, ctypes.byref(w), ctypes.byref(c), self.max_pairs, int(max_kpts))
        self.nk = self.lib.dim_sg_max_kpts(self._h)

    def match_batch_guarded(self, *a, logger=None, **k):
        """match_batch under the fp16x3 range guard (capi.run_guarded): synchronises."""
        return self.guarded(lambda: self.match_batch(*a, **k), "SuperGlue", logger)

    @torch.no_grad()
    def match_batch(self, kpts_tab, desc_tab, score_tab, n_tab, size_tab, pair_idx=None, n_pairs=None, out=None, sinkhorn_iterations=None,
                    match_threshold=None):
        """Device feature table -> device match tables; no host sync.  ``size_tab`` rows are (width, height).  See dim_hip.h:dim_sg_match."""
        cap = kpts_tab.shape[1]
        assert kpts_tab.dtype == torch.float32 and desc_tab.dtype == torch.float32 and score_tab.dtype == torch.float32 and n_tab.dtype == torch.int32
        assert kpts_tab.is_contiguous() and desc_tab.is_contiguous() and score_tab.is_contiguous() and size_tab.is_contiguous()
        assert desc_tab.shape[1] == cap and desc_tab.shape[2] == 256 and score_tab.shape[1] == cap and size_tab.dtype == torch.float32
        if pair_idx is not None:
            assert pair_idx.dtype == torch.int32 and pair_idx.is_contiguous()
            P = pair_idx.shape[0] if n_pairs is None else n_pairs
        else:
            P = kpts_tab.shape[0] // 2 if n_pairs is None else n_pairs
        iters = int(self.conf["sinkhorn_iterations"] if sinkhorn_iterations is None else sinkhorn_iterations)
        thr = float(self.conf["match_threshold"] if match_threshold is None else match_threshold)
        dev, NK = kpts_tab.device, self.nk
        if out is None:
            out = {
                "matches": torch.empty(P, NK, 2, dtype=torch.int64, device=dev),
                "scores": torch.empty(P, NK, dtype=torch.float32, device=dev),
                "n_matches": torch.zeros(P, dtype=torch.int32, device=dev),
                "matches01": torch.empty(P, 2, NK, dtype=torch.int32, device=dev),
                "mscores01": torch.empty(P, 2, NK, dtype=torch.float32, device=dev),
            }
        with self._ctx():
            capi.check(self.lib, self.lib.dim_sg_match(
                self._h, capi.ptr(kpts_tab), capi.ptr(desc_tab), capi.ptr(score_tab), capi.ptr(n_tab), capi.ptr(size_tab), int(cap),
                capi.ptr(pair_idx), int(P), iters, thr, capi.ptr(out["matches"]), capi.ptr(out["scores"]), capi.ptr(out["n_matches"]),
                capi.ptr(out["matches01"]), capi.ptr(out["mscores01"]), self._stream()))
        return out

    @torch.no_grad()
    def __call__(self, data: dict) -> dict:
        """Reference-style call for ONE pair (SGN:250-305): data = {keypoints0 [1,M,2], descriptors0 [1,256,M], scores0 [1,M], image0 (anything
        with a (1, 1, H, W) ``shape``), ...1}.  Returns the reference's four keys with the batch dimension kept at 1 (matches as int64), plus
        ``matches`` (S, 2) int64 and ``scores`` (S,)."""
        for k in ("scores0", "scores1"):
            if k not in data:
                raise ValueError(f"SuperGlue needs the detection scores: '{k}' is missing")
        k0, k1 = data["keypoints0"][0], data["keypoints1"][0]
        m, n = k0.shape[0], k1.shape[0]
        cap = max(m, n, 1)
        dev = self.device
        kt = torch.zeros(2, cap, 2, dtype=torch.float32, device=dev)
        dt = torch.zeros(2, cap, 256, dtype=torch.float32, device=dev)
        sc = torch.zeros(2, cap, dtype=torch.float32, device=dev)
        kt[0, :m], kt[1, :n] = k0.to(dev, torch.float32), k1.to(dev, torch.float32)
        dt[0, :m], dt[1, :n] = data["descriptors0"][0].T.to(dev, torch.float32), data["descriptors1"][0].T.to(dev, torch.float32)
        sc[0, :m], sc[1, :n] = data["scores0"][0].to(dev, torch.float32), data["scores1"][0].to(dev, torch.float32)
        nt = torch.tensor([m, n], dtype=torch.int32, device=dev)
        (h0, w0), (h1, w1) = tuple(data["image0"].shape)[-2:], tuple(data["image1"].shape)[-2:]
        st = torch.tensor([[w0, h0], [w1, h1]], dtype=torch.float32, device=dev)
        o = self.match_batch_guarded(kt, dt, sc, nt, st, n_pairs=1)
        S = int(o["n_matches"][0].item())
        return {
            "matches0": o["matches01"][0, 0, :m].long()[None], "matches1": o["matches01"][0, 1, :n].long()[None],
            "matching_scores0": o["mscores01"][0, 0, :m][None], "matching_scores1": o["mscores01"][0, 1, :n][None],
            "matches": o["matches"][0, :S], "scores": o["scores"][0, :S],
        }

    # ---- parity taps (dim_sg_debug) ----
    def _debug(self):
        p = [ctypes.c_void_p() for _ in range(6)]
        capi.check(self.lib, self.lib.dim_sg_debug(self._h, *[ctypes.byref(x) for x in p]))
        return dict(zip(("desc", "scores", "u", "v", "n_cur", "done"), (x.value for x in p)))

    def taps(self, m: int, n: int, pair: int = 0) -> dict:
        """After a call: the final descriptors, the score block and the Sinkhorn potentials of ``pair`` (m x n keypoints), as CPU tensors."""
        d, nk, lib, dev = self._debug(), self.nk, self.lib, self.device
        desc = capi.copy_from_device(lib, d["desc"] + 4 * (2 * pair) * nk * 256, (2, nk, 256), dev)
        u = capi.copy_from_device(lib, d["u"] + 4 * pair * (nk + 1), (nk + 1,), dev)
        v = capi.copy_from_device(lib, d["v"] + 4 * pair * (nk + 1), (nk + 1,), dev)
        out = {"desc0": desc[0, :m], "desc1": desc[1, :n], "u": u[:m + 1], "v": v[:n + 1]}
        if m * nk <= 1 << 24:
            out["scores"] = capi.copy_from_device(lib, d["scores"] + 4 * pair * nk * nk, (max(m, 1), nk), dev)[:m, :n]
        return out
