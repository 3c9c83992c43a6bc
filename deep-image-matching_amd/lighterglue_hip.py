"""LighterGlue on the dim_lg_* C ABI: LightGlue at XFeat's shape (reference thirdparty/accelerated_features/modules/lighterglue.py:12-27 —
input_dim 64, descriptor_dim 96, one head of 96, 6 layers, depth_confidence -1, width_confidence 0.95).

The handle comes from ``dim_lgl_create`` and is an ordinary ``dim_lg``: everything else (``match_batch``, the guarded call, the reference-style
``__call__``, the resident-matcher plumbing of the plugins) is ``LightGlueHIP``'s.  The reference's class wraps kornia's ``LightGlue``, a copy of the
vendored thirdparty/LightGlue module, which is what this port is pinned against (scripts/make_lighterglue_golden.py).
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import torch

from .lightglue_hip import LightGlueHIP


class LighterGlueHIP(LightGlueHIP):
    """Resident LighterGlue on one GPU.  ``descriptor_dim`` / ``num_heads`` are read from the state dict (Wqkv / posenc) unless given; the library
    builds (96, 1) and rejects every other shape."""

    # modules/lighterglue.py:12-27 (default_conf_xfeat); pruning_min_kpts -1 = the CPU path this library is parity-checked against
    default_conf = {"n_layers": 6, "depth_confidence": -1, "width_confidence": 0.95, "filter_threshold": 0.1, "pruning_min_kpts": -1}

    def __init__(self, state_dict: Dict[str, torch.Tensor], conf: Optional[dict] = None, max_pairs: int = 1, max_kpts: int = 2048,
                 device="cuda", lib=None, on_saturation: str = "fallback", arithmetic=None, descriptor_dim: Optional[int] = None,
                 num_heads: Optional[int] = None):
        if "input_proj.weight" not in state_dict:
            raise KeyError("LighterGlue state dict lacks 'input_proj.weight' (64 -> 96)")
        self.descriptor_dim = int(state_dict["transformers.0.self_attn.Wqkv.weight"].shape[1]) if descriptor_dim is None else int(descriptor_dim)
        self.num_heads = self.descriptor_dim // (2 * int(state_dict["posenc.Wr.weight"].shape[0])) if num_heads is None else int(num_heads)
        super().__init__(state_dict, conf, max_pairs, max_kpts, device, lib, on_saturation, arithmetic)

    def _create_handle(self, w, c, max_kpts):
        self.lib.dim_lgl_create.restype = ctypes.c_int
        self._create(self.lib.dim_lgl_create, ctypes.byref(w), ctypes.byref(c), int(self.descriptor_dim), int(self.num_heads), self.max_pairs,
                     max_kpts)
