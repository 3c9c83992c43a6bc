"""Thin host wrapper around the dim_nn_* C ABI (one resident nearest-neighbour matcher handle).

The second matcher of the library next to ``LightGlueHIP``: kornia's ``DescriptorMatcher`` modes nn / mnn / snn / smnn on
a device feature table, with the same batched surface (``match_batch``, ``match_batch_guarded``, ``.nk``, ``.device``) and
the same ``(matches [P][NK][2] int64, n_matches [P])`` output layout, so ``BatchedImageMatcher``, ``PairMatchingPipeline``,
the tile matcher and ``DeviceVerifier`` take either.  ``lib`` / ``device`` are injectable for the CPU emulator tests; there
is no CPU fallback.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import capi

MODES = tuple(capi.NN_MODES)


def check_mode(mode) -> str:
    if mode not in capi.NN_MODES:
        raise ValueError(f"match_mode must be one of {list(MODES)} (kornia's other DescriptorMatcher modes are not implemented), got {mode!r}")
    return mode


class NearestNeighborHIP(capi.ResidentHandle):
    """Resident nearest-neighbour descriptor matcher on one GPU (csrc/nn_match.hip)."""

    _destroy = "dim_nn_destroy"

    def __init__(self, mode: str = "smnn", th: float = 0.8, dim: int = 256, max_pairs: int = 1, max_kpts: int = 2048, device="cuda",
                 lib=None, on_saturation: str = "fallback", arithmetic=None, f16_exact: bool = False):
        self.mode, self.th, self.input_dim = check_mode(mode), float(th), int(dim)
        self.f16_exact = bool(f16_exact)    # default of match_batch's f16_exact: the tables hold float16-exact values (features.h5)
        self._open(device, lib, on_saturation, arithmetic)
        capi.declare_nn(self.lib)
        self.max_pairs = int(max_pairs)
        cfg = capi.NnConfig(capi.NN_MODES[self.mode], self.th)
        self._create(self.lib.dim_nn_create, ctypes.byref(cfg), self.max_pairs, int(max_kpts), self.input_dim)
        self.nk = self.lib.dim_nn_max_kpts(self._h)

    def workspace_bytes(self) -> int:
        """Device bytes the handle owns (no M x N buffer among them)."""
        return int(self.lib.dim_nn_workspace_bytes(self._h))

    def match_batch_guarded(self, *a, logger=None, **k):
        """match_batch under the fp16x3 range guard (capi.run_guarded): synchronises."""
        return self.guarded(lambda: self.match_batch(*a, **k), "nearest-neighbour matcher", logger)

    @torch.no_grad()
    def match_batch(self, kpts_tab, desc_tab, n_tab, size_tab=None, pair_idx=None, n_pairs=None, out=None, taps: bool = False,
                    f16_exact: Optional[bool] = None):
        """Device feature table -> device match tables; no host sync.  See dim_hip.h:dim_nn_match.  ``kpts_tab`` / ``size_tab`` are accepted
        for the matcher interface and ignored.  ``taps``: also return row_stats / col_stats [P][3][NK] (argmin as int32 bits, min d2, second d2)."""
        cap = desc_tab.shape[1]
        assert desc_tab.dtype == torch.float32 and n_tab.dtype == torch.int32 and desc_tab.is_contiguous()
        assert desc_tab.shape[2] == self.input_dim
        if pair_idx is not None:
            assert pair_idx.dtype == torch.int32 and pair_idx.is_contiguous()
            P = pair_idx.shape[0] if n_pairs is None else n_pairs
        else:
            P = desc_tab.shape[0] // 2 if n_pairs is None else n_pairs
        dev, NK = desc_tab.device, self.nk
        if out is None:
            out = {"matches": torch.empty(P, NK, 2, dtype=torch.int64, device=dev), "scores": torch.empty(P, NK, dtype=torch.float32, device=dev),
                   "n_matches": torch.zeros(P, dtype=torch.int32, device=dev)}
        if taps:
            out["row_stats"] = torch.zeros(P, 3, NK, dtype=torch.float32, device=dev)
            out["col_stats"] = torch.zeros(P, 3, NK, dtype=torch.float32, device=dev)
        exact = self.f16_exact if f16_exact is None else bool(f16_exact)
        with self._ctx():
            capi.check(self.lib, self.lib.dim_nn_match(
                self._h, capi.ptr(desc_tab), capi.ptr(n_tab), int(cap), int(exact), capi.ptr(pair_idx), int(P), capi.ptr(out["matches"]),
                capi.ptr(out["scores"]), capi.ptr(out["n_matches"]), capi.ptr(out.get("row_stats")), capi.ptr(out.get("col_stats")), self._stream()))
        return out
