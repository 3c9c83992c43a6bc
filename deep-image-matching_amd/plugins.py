"""Drop-in plugins for deep-image-matching's extractor / matcher plugin surface.

``SuperPointExtractor`` mirrors extractors/superpoint.py:64-146 and ``LightGlueMatcher``
mirrors matchers/lightglue.py:77-125: same class attributes (``_default_conf``,
``required_inputs``, ``grayscale``, ``descriptor_size`` …), same constructor arguments, same
``_extract(image) -> dict`` / ``_match_pairs(feats0, feats1) -> np.ndarray`` contracts and
error behaviour, with the network replaced by the gfx950 library.  When the real
``deep_image_matching`` package is importable the classes subclass its ``ExtractorBase`` /
``MatcherBase`` (so ``extractor_loader`` / ``matcher_loader`` discover them, extractor_base.py:29-52,
matcher_base.py:36-60); otherwise a minimal stand-in base with the same constructor contract
(extractor_base.py:119-160) is used so the hooks can be driven and tested on their own.
``KorniaMatcher`` mirrors matchers/kornia_matcher.py:9-53 (nearest-neighbour descriptor matching, no weights);
``SuperPointOpenExtractor`` mirrors extractors/superpoint_open.py:72-164 (the openly licensed SuperPoint);
``XfeatExtractor`` mirrors extractors/xfeat.py:11-63 (XFeat's sparse detectAndCompute);
``RIPEExtractor`` mirrors extractors/ripe.py:10-118 (RIPE, the extractor of the ``ripe+kornia_matcher`` pipeline);
``LighterGlueMatcher`` mirrors matchers/lighterglue.py:78-241 (the matcher of the shipped ``xfeat+lighterglue`` pipeline);
``SuperGlueMatcher`` mirrors matchers/superglue.py:54-106 (the matcher of the shipped ``superpoint+superglue`` pipeline).
See INTEGRATION.md for the module files a maintainer adds to the reference tree.
"""
from __future__ import annotations

import logging
import ctypes
import os
from typing import Optional

import numpy as np
import torch

from . import capi
from . import weights as _weights
from .alike_hip import AlikeHIP
from .aliked_hip import AlikedHIP
from .lightglue_hip import LightGlueHIP
from .lighterglue_hip import LighterGlueHIP
from .nn_hip import NearestNeighborHIP, check_mode as _check_nn_mode
from .superglue_hip import SuperGlueHIP
from .superpoint_hip import SuperPointHIP, SuperPointOpenHIP
from .tile_matching import BatchedTileMatchingMixin
from .tiling import BatchedTilingMixin
from .ripe_hip import RipeHIP
from .xfeat_hip import XFeatHIP

logger = logging.getLogger("dim")

try:  # pragma: no cover - the reference package is not importable in the build container
    from deep_image_matching.extractors.extractor_base import ExtractorBase as _ExtractorBase
    from deep_image_matching.matchers.matcher_base import MatcherBase as _MatcherBase

    HAVE_DIM = True
except Exception:  # noqa: BLE001
    HAVE_DIM = False

    class _StandInBase:
        """Constructor contract of ExtractorBase/MatcherBase (extractor_base.py:119-160,
        matcher_base.py:95-140): config exposes .general/.extractor/.matcher (or is a dict with
        those keys); self.config = {"general", "extractor"|"matcher"}; device honours force_cpu."""

        _role = "extractor"
        _default_conf: dict = {}

        def __init__(self, config):
            get = (lambda k: config.get(k, {})) if isinstance(config, dict) else (lambda k: getattr(config, k, {}) or {})
            if not isinstance(config, dict) and not all(hasattr(config, a) for a in ("general",)):
                raise TypeError("`config` must be a Config object (or a dict with 'general' / '%s')" % self._role)
            general = dict(get("general"))
            self.config = {"general": general, self._role: {**self._default_conf, **dict(get(self._role))}}
            self._device = "cuda" if torch.cuda.is_available() and not general.get("force_cpu", False) else "cpu"

    class _ExtractorBase(_StandInBase):
        _role = "extractor"

    class _MatcherBase(_StandInBase):
        _role = "matcher"


def _apply_arithmetic(conf: dict, lib):
    """Optional plugin option ``arithmetic``: "fp16x3" (library default: 2-way fp16 splits x 3 MFMA terms; activations
    exact up to |x| = 4094 — guarded: a call that leaves the range is repeated in bf16x6, option ``on_saturation``),
    "bf16x6" (exact 3-way bf16 splits x 6 terms, no range limit) or "fp32" (plain fp32 MFMA).
    The choice belongs to THIS plugin's library handles (dim_handle_tune_set key 1, set when a handle is created); without the option
    the handles follow the process default (capi.set_arithmetic).  Returns the validated name or None."""
    name = (conf or {}).get("arithmetic")
    if name is None:
        return None
    if name not in capi.ARITHMETIC:
        raise ValueError(f"arithmetic must be one of {sorted(capi.ARITHMETIC)}, got {name!r}")
    return name


def _saturation_policy(conf: dict) -> str:
    pol = (conf or {}).get("on_saturation", "fallback")
    if pol not in ("fallback", "raise", "off"):
        raise ValueError(f"on_saturation must be 'fallback', 'raise' or 'off', got {pol!r}")
    return pol


class _PinnedStaging:
    """Page-locked host staging for the per-call hooks (one image in, one feature set out per call).  The reference's
    ``torch.tensor(image / 255.0).to(device)`` / ``.cpu().numpy()`` go through pageable memory; on the MI355X box that cost 5 - 15 ms per
    call around 0.8 ms of kernels (profiles/r05_hook_profile.txt).  Buffers grow on demand and are reused: a call must have finished with
    them (the hooks synchronise before they return) before the next call touches them."""

    def __init__(self):
        self._buf = {}

    def get(self, tag: str, nbytes: int) -> torch.Tensor:
        b = self._buf.get(tag)
        if b is None or b.numel() < nbytes:
            b = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8).pin_memory()
            self._buf[tag] = b
        return b

    def upload_scaled(self, image: np.ndarray, device) -> torch.Tensor:
        """``image / 255.0`` as float32, computed by numpy STRAIGHT INTO the page-locked buffer (one pass, no torch CPU op: a 256-thread intra-op
        pool needs milliseconds to wake up for a 4 MB copy), then an asynchronous copy to the device on the current stream.  Same values as the
        reference's torch.tensor(image / 255.0, dtype=torch.float): numpy divides in the input's precision and the result is rounded to float32."""
        n = int(image.size) * 4
        pin = self.get("in", n)[:n].view(torch.float32).view(tuple(image.shape))
        np.divide(image, 255.0, out=pin.numpy(), casting="same_kind")
        return pin.to(device, non_blocking=True)

    def download(self, tensors, device) -> list:
        """device tensors -> owned numpy arrays through ONE pinned buffer and ONE synchronisation."""
        sizes = [t.numel() * t.element_size() for t in tensors]
        off = [0]
        for z in sizes:
            off.append(off[-1] + ((z + 255) & ~255))
        pin = self.get("out", off[-1])
        views = []
        for t, o, z in zip(tensors, off, sizes):
            v = pin[o:o + z].view(t.dtype).view(t.shape)
            v.copy_(t, non_blocking=True)
            views.append(v)
        torch.cuda.current_stream(device).synchronize()
        return [v.numpy().copy() for v in views]


def _frame2array(image: np.ndarray) -> np.ndarray:
    """The layout half of the reference's _frame2tensor (SPX:134-146, ALX:66-78): (H, W) -> [1, 1, H, W], (H, W, C) -> [1, C, H, W] (a view)."""
    if len(image.shape) == 2:
        return image[None][None]
    if len(image.shape) == 3:
        return image.transpose(2, 0, 1)[None]
    return image


def _resolve_device(device, what: str):
    """The plugin's device: the reference's ``self._device`` ("cuda" unless general.force_cpu).  There is no CPU
    path; the CPU tests install the emulator build through capi.install(), which also names the device."""
    forced = capi.installed_device()
    if forced is not None:
        return forced
    kind = getattr(device, "type", str(device))
    if not str(kind).startswith("cuda"):
        raise RuntimeError(f"{what}: the MI355X plugin has no CPU path (device={device!r}); "
                           "use the reference's own plugin when general.force_cpu is set")
    return device


class SuperPointExtractor(BatchedTilingMixin, _ExtractorBase):
    """extractors/superpoint.py:64 — SuperPoint on the gfx950 library."""

    _default_conf = {
        "name": "superpoint",
        "nms_radius": 4,
        "keypoint_threshold": 0.005,
        "max_keypoints": -1,
        "remove_borders": 4,
        "fix_sampling": False,
    }
    required_inputs = ["image"]
    grayscale = True
    as_float = True
    descriptor_size = 256
    features_as_half = True
    detection_noise = 2.0

    def __init__(self, config):
        super().__init__(config)
        self._lib = capi.load()
        self._device = _resolve_device(self._device, "SuperPointExtractor")
        cfg = self.config.get("extractor")
        self._arith = _apply_arithmetic(cfg, self._lib)
        self._on_sat = _saturation_policy(cfg)
        path = cfg.get("weights_path") or os.environ.get("DIM_SUPERPOINT_WEIGHTS")
        if path is None and cfg.get("allow_synthetic_weights"):
            logger.warning("SuperPoint: running on seeded SYNTHETIC weights (allow_synthetic_weights) - test / benchmark use only")
        self._sd = _weights.load_superpoint_state_dict(path, allow_synthetic=bool(cfg.get("allow_synthetic_weights", False)))
        self._net_cfg = {k: cfg[k] for k in ("nms_radius", "keypoint_threshold", "max_keypoints", "remove_borders", "fix_sampling")}
        self._net: Optional[SuperPointHIP] = None
        self._net_hw = (0, 0)
        self._min_capacity = 0  # raised when a keep-all extraction overflowed the slot (see _regrow)

    def _capacity(self, H: int, W: int) -> int:
        """Slot size per image.  max_keypoints > 0: exactly that.  Keep-all mode (-1, the plugin default): a first
        guess of 4 keypoints per 8x8 cell; a call that yields more candidates is repeated with a larger slot
        (_regrow), so nothing is ever dropped — the reference returns every keypoint (SPN:183-207)."""
        mk = self._net_cfg["max_keypoints"]
        return mk if mk > 0 else max(self._min_capacity, min(4096 * 4, max(1024, (H // 8) * (W // 8) * 4)))

    def _ensure(self, H: int, W: int):
        cap = self._capacity(H, W)
        if self._net is None or H > self._net_hw[0] or W > self._net_hw[1] or cap > self._net.capacity:
            hw = (max(H, self._net_hw[0]), max(W, self._net_hw[1]))
            self._net = SuperPointHIP(self._sd, self._net_cfg, max_batch=1, max_hw=hw, capacity=cap,
                                      device=self._device, lib=self._lib, on_saturation=self._on_sat, arithmetic=self._arith)
            self._net_hw = hw

    def _ensure_batch(self, H: int, W: int, batch: int):
        """Separate resident handle for batched tile extraction (tiling.BatchedTilingMixin)."""
        key = getattr(self, "_tile_key", None)
        cap = self._capacity(H, W)
        if key is None or H > key[0] or W > key[1] or batch > key[2] or cap > self._tile_net.capacity:
            self._tile_net = SuperPointHIP(self._sd, self._net_cfg, max_batch=batch, max_hw=(H, W), capacity=cap,
                                           device=self._device, lib=self._lib, on_saturation=self._on_sat, arithmetic=self._arith)
            self._tile_key = (H, W, batch)
        return self._tile_net

    def _regrow(self, net: SuperPointHIP, batch: int) -> bool:
        """Keep-all mode: True when the last call produced more candidates than the slot holds (the library then kept
        only the first `capacity` in row-major order).  The next _ensure / _ensure_batch builds a larger handle."""
        if self._net_cfg["max_keypoints"] > 0:
            return False
        worst = int(net.candidate_counts(batch).max())
        if worst <= net.capacity:
            return False
        self._min_capacity = 1 << (worst - 1).bit_length()
        logger.warning("SuperPoint: %d keypoints exceed the slot of %d - repeating the extraction with %d", worst, net.capacity,
                       self._min_capacity)
        return True

    @torch.no_grad()
    def _extract(self, image: np.ndarray) -> dict:
        """image: float32 HxW, values 0..255 (extractor_base.py:197-202).  Returns numpy
        keypoints (N,2) float32 (x,y), scores (N,), descriptors (256,N) (SPX:126-130)."""
        image_ = _to_device(self, _frame2array(image), self._device)      # (= _frame2tensor without its synchronisation: this call synchronises below)
        if image_.shape[1] != 1:
            raise ValueError("SuperPoint expects a single-channel image")
        H, W = int(image_.shape[-2]), int(image_.shape[-1])
        self._ensure(H, W)
        img = image_.reshape(1, H, W)
        out = self._net.extract_batch_guarded(img)
        if self._regrow(self._net, 1):
            self._ensure(H, W)
            out = self._net.extract_batch_guarded(img)
        return _features_to_numpy(self, out)

    def _frame2tensor(self, image: np.ndarray, device: str = "cuda"):
        """SPX:134-146 (through page-locked staging on a GPU)."""
        return _to_device(self, _frame2array(image), device, sync=True)


def _to_device(plugin, image: np.ndarray, device, sync: bool = False):
    """image / 255.0 (float32, the reference's values) on ``device``, same shape as ``image``.  The copy leaves a REUSED page-locked buffer
    asynchronously: ``sync=True`` (the public _frame2tensor hooks) waits for it, so that a second call cannot overwrite the source of a copy
    still in flight; _extract keeps the asynchronous form and synchronises before it returns."""
    if str(getattr(device, "type", device)).startswith("cuda"):
        st = plugin.__dict__.setdefault("_staging", _PinnedStaging())
        t = st.upload_scaled(image, device)
        if sync:
            torch.cuda.current_stream(t.device).synchronize()
        return t
    return torch.from_numpy(np.ascontiguousarray(image / 255.0, dtype=np.float32)).to(device)


def _features_to_numpy(plugin, out) -> dict:
    """(kpts [1,cap,2], scores [1,cap], desc [1,cap,D], n [1]) of a batch-1 library call -> the reference's numpy dict: keypoints (N,2), scores
    (N,), descriptors (D,N) (SPX:126-130, ALX:57-61).  On a GPU: one pinned buffer, one synchronisation; the descriptors come back as the
    transposed VIEW of an owned (N,D) array — (D,N) to every consumer, and featuresDict2Lightglue's (N,D) costs nothing."""
    kp, sc, de, n = out
    if kp.device.type == "cuda":
        st = plugin.__dict__.setdefault("_staging", _PinnedStaging())
        kp_h, sc_h, de_h, n_h = st.download([kp[0], sc[0], de[0], n[:1]], kp.device)
    else:
        kp_h, sc_h, de_h, n_h = kp[0].numpy().copy(), sc[0].numpy().copy(), de[0].numpy().copy(), n[:1].numpy()
    k = int(n_h[0])
    return {"keypoints": kp_h[:k], "scores": sc_h[:k], "descriptors": de_h[:k].T}


class AlikedExtractor(BatchedTilingMixin, _ExtractorBase):
    """extractors/aliked.py:10 — ALIKED on the gfx950 library (train-mode BatchNorm, Q7; scores are
    the dispersities, Q8 — both reproduced inside the library)."""

    _default_conf = {  # ALX:22-29 (the "name:" key with the stray colon is the reference's)
        "name:": "aliked",
        "model": "aliked-n16rot",
        "device": "cuda",
        "max_num_keypoints": 4000,
        "detection_threshold": 0.2,
        "nms_radius": 2,
    }
    required_inputs = []
    grayscale = False
    as_float = True
    descriptor_size = 128
    features_as_half = True

    def __init__(self, config):
        super().__init__(config)
        self._lib = capi.load()
        self._device = _resolve_device(self._device, "AlikedExtractor")
        cfg = self.config.get("extractor")
        # ALIKED(**cfg) reads conf.model_name (default "aliked-n16", ALN:562-567); DIM's "model" key is ignored by the net
        self._net_cfg = {"model_name": cfg.get("model_name", "aliked-n16"), "max_num_keypoints": cfg["max_num_keypoints"],
                         "detection_threshold": cfg["detection_threshold"], "nms_radius": cfg["nms_radius"]}
        path = cfg.get("weights_path") or os.environ.get("DIM_ALIKED_WEIGHTS")
        if path is None and cfg.get("allow_synthetic_weights"):
            logger.warning("ALIKED: running on seeded SYNTHETIC weights (allow_synthetic_weights) - test / benchmark use only")
        self._sd = _weights.load_aliked_state_dict(path, model_name=self._net_cfg["model_name"],
                                                   allow_synthetic=bool(cfg.get("allow_synthetic_weights", False)))
        self.descriptor_size = int(_weights.ALIKED_CFGS[self._net_cfg["model_name"]][4])   # 128; aliked-t16: 64 (the reference's class attribute says 128 for all)
        self._net: Optional[AlikedHIP] = None
        self._net_hw = (0, 0)

    def _ensure(self, H: int, W: int):
        if self._net is None or H > self._net_hw[0] or W > self._net_hw[1]:
            hw = (max(H, self._net_hw[0]), max(W, self._net_hw[1]))
            mk = self._net_cfg["max_num_keypoints"]
            self._net = AlikedHIP(self._sd, self._net_cfg, max_batch=1, max_hw=hw, capacity=mk if mk > 0 else None,
                                  device=self._device, lib=self._lib)
            self._net_hw = hw

    def _ensure_batch(self, H: int, W: int, batch: int):
        key = getattr(self, "_tile_key", None)
        if key is None or H > key[0] or W > key[1] or batch > key[2]:
            mk = self._net_cfg["max_num_keypoints"]
            self._tile_net = AlikedHIP(self._sd, self._net_cfg, max_batch=batch, max_hw=(H, W), capacity=mk if mk > 0 else None,
                                       device=self._device, lib=self._lib)
            self._tile_key = (H, W, batch)
        return self._tile_net

    @torch.no_grad()
    def _extract(self, image: np.ndarray) -> dict:
        """image: float32 HxWx3 RGB (or HxW), 0..255.  Returns numpy keypoints (N,2), descriptors
        (128,N) (ALX:57-58 transposes), scores (N,) (ALX:60-61 renames keypoint_scores)."""
        # the library reads HWC: the reference's CHW tensor (ALX:66-78, _frame2tensor below) would be transposed there and back
        a = image if image.ndim == 3 else image[..., None]
        self._ensure(a.shape[0], a.shape[1])
        return _features_to_numpy(self, self._net.extract_batch_guarded(_to_device(self, a, self._device)[None].contiguous()))

    def _frame2tensor(self, image: np.ndarray, device: str = "cuda"):
        """ALX:66-78 (through page-locked staging on a GPU)."""
        return _to_device(self, _frame2array(image), device, sync=True)


class AlikeExtractor(_ExtractorBase):
    """extractors/alike.py:8 — ALIKE (alike-t / s / n / l) on the gfx950 library: eval-mode BatchNorm, sub-pixel keypoints, scores = the score map
    sampled at the refined positions, descriptors sampled bilinearly from a descriptor map that is only ever evaluated around the keypoints."""

    _default_conf = {  # AKX:9-17 (the "name:" key with the stray colon is the reference's)
        "name:": "alike",
        "model": "alike-s",
        "device": "cuda",
        "top_k": 15000,
        "scores_th": 0.2,
        "n_limit": 15000,
        "subpixel": True,
    }
    required_inputs = []
    grayscale = False
    descriptor_size = 96

    def __init__(self, config):
        super().__init__(config)
        self._lib = capi.load()
        self._device = _resolve_device(self._device, "AlikeExtractor")
        cfg = self.config.get("extractor")
        if cfg["model"] not in _weights.ALIKE_CFGS:
            raise ValueError(f"AlikeExtractor: unknown model {cfg['model']!r}; expected one of {sorted(_weights.ALIKE_CFGS)}")
        # the reference always extracts with sub_pixel=True (AKX:39), whatever the "subpixel" key says
        self._net_cfg = {"model": cfg["model"], "top_k": int(cfg["top_k"]), "scores_th": float(cfg["scores_th"]), "n_limit": int(cfg["n_limit"])}
        arith = _apply_arithmetic(cfg, self._lib)
        if arith is not None:
            self._net_cfg["arithmetic"] = arith
        self._net_cfg["on_saturation"] = _saturation_policy(cfg)
        path = cfg.get("weights_path") or os.environ.get("DIM_ALIKE_WEIGHTS")
        if path is None and cfg.get("allow_synthetic_weights"):
            logger.warning("ALIKE: running on seeded SYNTHETIC weights (allow_synthetic_weights) - test / benchmark use only")
        self._sd = _weights.load_alike_state_dict(path, cfg["model"], allow_synthetic=bool(cfg.get("allow_synthetic_weights", False)))
        self.descriptor_size = int(_weights.ALIKE_CFGS[cfg["model"]][4])   # 64 / 96 / 128 / 128 (the reference's class attribute says 96 for all)
        self._net: Optional[AlikeHIP] = None
        self._net_hw = (0, 0)

    def _ensure(self, H: int, W: int):
        if self._net is None or H > self._net_hw[0] or W > self._net_hw[1]:
            hw = (max(H, self._net_hw[0]), max(W, self._net_hw[1]))
            self._net = AlikeHIP(self._sd, self._net_cfg, max_batch=1, max_hw=hw, device=self._device, lib=self._lib)
            self._net_hw = hw

    @torch.no_grad()
    def _extract(self, image: np.ndarray) -> dict:
        """image: HxWx3 RGB, 0..255 (uint8 as the reference's loader hands it over, or float).  Returns numpy keypoints (N,2), descriptors (D,N)
        (AKX:42 transposes), scores (N,)."""
        if image.ndim != 3 or image.shape[2] != 3:
            raise AssertionError("input image shape should be [HxWx3]")   # AKM:143-144
        self._ensure(image.shape[0], image.shape[1])
        return _features_to_numpy(self, self._net.extract_batch_guarded(_to_device(self, image, self._device)[None].contiguous()))

    def _frame2tensor(self, image: np.ndarray, device: str = "cuda"):
        """AKX:46-54: the reference's hook is empty (ALike.forward converts the array itself)."""
        return None


class SuperPointOpenExtractor(_ExtractorBase):
    """extractors/superpoint_open.py:72 — the openly licensed SuperPoint (thirdparty/SuperPoint_open) on the gfx950 library: every block
    conv -> ReLU -> BatchNorm(eval) with the BatchNorm in the convolution's epilogue.  DEVIATION, stated in INTEGRATION.md: with the class
    default ``max_keypoints = -1`` the reference's network raises inside torch.topk; here -1 keeps every keypoint (row-major order)."""

    _default_conf = {  # extractors/superpoint_open.py:94-101 (name and fix_sampling as the reference has them: its network knows one sampler)
        "name": "superpoint",
        "nms_radius": 4,
        "keypoint_threshold": 0.005,
        "max_keypoints": -1,
        "remove_borders": 4,
        "fix_sampling": False,
    }
    required_inputs = ["image"]
    grayscale = True
    descriptor_size = 256
    detection_noise = 2.0

    def __init__(self, config):
        super().__init__(config)
        self._lib = capi.load()
        self._device = _resolve_device(self._device, "SuperPointOpenExtractor")
        cfg = self.config.get("extractor")
        self._arith = _apply_arithmetic(cfg, self._lib)
        self._on_sat = _saturation_policy(cfg)
        path = cfg.get("weights_path") or os.environ.get("DIM_SUPERPOINT_OPEN_WEIGHTS")
        if path is None and cfg.get("allow_synthetic_weights"):
            logger.warning("SuperPoint (open): running on seeded SYNTHETIC weights (allow_synthetic_weights) - test / benchmark use only")
        self._sd = _weights.load_superpoint_open_state_dict(path, allow_synthetic=bool(cfg.get("allow_synthetic_weights", False)))
        self._net_cfg = {k: cfg[k] for k in ("nms_radius", "keypoint_threshold", "max_keypoints", "remove_borders")}
        self._net: Optional[SuperPointOpenHIP] = None
        self._net_hw = (0, 0)
        self._min_capacity = 0

    _capacity = SuperPointExtractor._capacity   # the slot size and the keep-all regrow are SuperPoint's
    _regrow = SuperPointExtractor._regrow

    def _ensure(self, H: int, W: int):
        cap = self._capacity(H, W)
        if self._net is None or H > self._net_hw[0] or W > self._net_hw[1] or cap > self._net.capacity:
            hw = (max(H, self._net_hw[0]), max(W, self._net_hw[1]))
            self._net = SuperPointOpenHIP(self._sd, self._net_cfg, max_batch=1, max_hw=hw, capacity=cap,
                                          device=self._device, lib=self._lib, on_saturation=self._on_sat, arithmetic=self._arith)
            self._net_hw = hw

    @torch.no_grad()
    def _extract(self, image: np.ndarray) -> dict:
        """image: float32 HxW, values 0..255.  Zero-padded at the bottom and the right to multiples of 8 as the reference's hook does
        (extractors/superpoint_open.py:131-135; borders are removed relative to the PADDED frame and keypoints inside the padding are kept, as
        there).  Returns numpy keypoints (N,2) float32 (x,y), scores (N,), descriptors (256,N)."""
        a = _frame2array(image)
        if a.shape[1] != 1:
            raise ValueError("SuperPoint expects a single-channel image")
        H, W = int(a.shape[-2]), int(a.shape[-1])
        Hp, Wp = -(-H // 8) * 8, -(-W // 8) * 8
        if (Hp, Wp) != (H, W):
            a = np.pad(a, [(0, 0), (0, 0), (0, Hp - H), (0, Wp - W)])
        self._ensure(Hp, Wp)
        img = _to_device(self, a, self._device).reshape(1, Hp, Wp)
        out = self._net.extract_batch_guarded(img)
        if self._regrow(self._net, 1):
            self._ensure(Hp, Wp)
            out = self._net.extract_batch_guarded(img)
        return _features_to_numpy(self, out)

    def _frame2tensor(self, image: np.ndarray, device: str = "cuda"):
        """extractors/superpoint_open.py:152-164 (through page-locked staging on a GPU)."""
        return _to_device(self, _frame2array(image), device, sync=True)


class XfeatExtractor(_ExtractorBase):
    """extractors/xfeat.py:11 — XFeat (sparse detectAndCompute) on the gfx950 library.  The reference's quirks are kept: ``detect_threshold`` is
    read from the config and never handed to the network, which always runs its own 0.05; the image reaches the network in 0..255; the
    descriptors come back as (N,64) ROWS, not transposed like every other extractor's (and ``descriptor_size`` says 128)."""

    _default_conf = {  # extractors/xfeat.py:12-16
        "name": "xfeat",
        "max_num_keypoints": 4000,
        "detect_threshold": 0.05,
    }
    required_inputs = []
    grayscale = False
    descriptor_size = 128

    def __init__(self, config):
        super().__init__(config)
        self._lib = capi.load()
        self._device = _resolve_device(self._device, "XfeatExtractor")
        cfg = self.config.get("extractor")
        self.max_num_keypoints = int(cfg.get("max_num_keypoints", self._default_conf["max_num_keypoints"]))
        self._net_cfg = {"top_k": self.max_num_keypoints, "detection_threshold": 0.05}   # (not cfg["detect_threshold"]: extractors/xfeat.py:28-30)
        arith = _apply_arithmetic(cfg, self._lib)
        if arith is not None:
            self._net_cfg["arithmetic"] = arith
        self._net_cfg["on_saturation"] = _saturation_policy(cfg)
        path = cfg.get("weights_path") or os.environ.get("DIM_XFEAT_WEIGHTS")
        if path is None and cfg.get("allow_synthetic_weights"):
            logger.warning("XFeat: running on seeded SYNTHETIC weights (allow_synthetic_weights) - test / benchmark use only")
        self._sd = _weights.load_xfeat_state_dict(path, allow_synthetic=bool(cfg.get("allow_synthetic_weights", False)))
        self._net: Optional[XFeatHIP] = None
        self._net_hw = (0, 0)

    def _ensure(self, H: int, W: int):
        if self._net is None or H > self._net_hw[0] or W > self._net_hw[1]:
            hw = (max(H, self._net_hw[0]), max(W, self._net_hw[1]))
            self._net = XFeatHIP(self._sd, self._net_cfg, max_batch=1, max_hw=hw, device=self._device, lib=self._lib)
            self._net_hw = hw

    @torch.no_grad()
    def _extract(self, image: np.ndarray) -> dict:
        """image: HxWx3 or HxW, 0..255, handed to the network unscaled (extractors/xfeat.py:37).  Returns numpy keypoints (N,2), scores (N,),
        descriptors (N,64)."""
        if image.ndim not in (2, 3):
            raise RuntimeError("For numpy arrays, only (H,W) or (H,W,C) format is supported.")   # XFM:227
        a = np.ascontiguousarray(image if image.ndim == 3 else image[..., None], dtype=np.float32)
        self._ensure(a.shape[0], a.shape[1])
        kp, sc, de, n = self._net.extract_batch_guarded(torch.from_numpy(a)[None].to(self._device))
        k = int(n[0].item())
        return {"keypoints": kp[0, :k].cpu().numpy(), "scores": sc[0, :k].cpu().numpy(), "descriptors": de[0, :k, :64].cpu().numpy()}

    def _frame2tensor(self, image: np.ndarray, device: str = "cuda"):
        """extractors/xfeat.py:44-56."""
        return _to_device(self, _frame2array(image), device, sync=True)


class RIPEExtractor(_ExtractorBase):
    """extractors/ripe.py:10 — RIPE (vgg_hyper: VGG19-BN encoder, DeDoDe-style decoder, hypercolumn descriptors) on the gfx950 library.  The
    reference runs its CUDA path under fp16 autocast; this is pinned to its fp32 path.  ``descriptor_size`` says 128 as the reference's class does;
    the descriptors are 256-dimensional, returned as (256, N)."""

    _default_conf = {  # extractors/ripe.py:11-15
        "name": "ripe",
        "max_keypoints": 4000,
        "detect_threshold": 0.5,
    }
    required_inputs = []
    grayscale = False
    descriptor_size = 128

    def __init__(self, config):
        super().__init__(config)
        self._lib = capi.load()
        self._device = _resolve_device(self._device, "RIPEExtractor")
        cfg = self.config.get("extractor")
        self.max_num_keypoints = int(cfg.get("max_keypoints", self._default_conf["max_keypoints"]))
        self.detect_threshold = float(cfg.get("detect_threshold", self._default_conf["detect_threshold"]))
        self._net_cfg = {"top_k": self.max_num_keypoints, "threshold": self.detect_threshold}
        arith = _apply_arithmetic(cfg, self._lib)
        if arith is not None:
            self._net_cfg["arithmetic"] = arith
        self._net_cfg["on_saturation"] = _saturation_policy(cfg)
        path = cfg.get("weights_path") or os.environ.get("DIM_RIPE_WEIGHTS")
        if path is None and cfg.get("allow_synthetic_weights"):
            logger.warning("RIPE: running on seeded SYNTHETIC weights (allow_synthetic_weights) - test / benchmark use only")
        self._sd = _weights.load_ripe_state_dict(path, allow_synthetic=bool(cfg.get("allow_synthetic_weights", False)))
        self._net: Optional[RipeHIP] = None
        self._net_hw = (0, 0)

    def _ensure(self, H: int, W: int):
        if self._net is None or H > self._net_hw[0] or W > self._net_hw[1]:
            hw = (max(H, self._net_hw[0]), max(W, self._net_hw[1]))
            self._net = RipeHIP(self._sd, self._net_cfg, max_batch=1, max_hw=hw, device=self._device, lib=self._lib)
            self._net_hw = hw

    @torch.no_grad()
    def _extract(self, image: np.ndarray) -> dict:
        """image: HxWx3 or HxW, 0..255 (extractors/ripe.py:57-89).  Returns numpy keypoints (N,2), descriptors (256,N), scores (N,);
        RuntimeError("No keypoints detected") where the reference raises it."""
        t = self._frame2tensor(image, self._device)          # [1, C, H, W] in 0..1
        self._ensure(t.shape[2], t.shape[3])
        f = self._net(t)
        return {"keypoints": f["keypoints"].cpu().numpy(), "descriptors": f["descriptors"].cpu().numpy().T, "scores": f["scores"].cpu().numpy()}

    def _frame2tensor(self, image: np.ndarray, device: str = "cuda"):
        """extractors/ripe.py:91-112."""
        return _to_device(self, _frame2array(image), device, sync=True)


def featuresDict2Lightglue(feats: dict) -> dict:
    """matchers/lightglue.py:8-66 up to (not including) the tensor conversion: unwrap, fix the
    descriptor layout by the keypoint count ((D,N) -> (N,D)), drop path keys."""
    feats = {k: v[0] if isinstance(v, (list, tuple)) else v for k, v in feats.items()}
    if "keypoints" not in feats or "descriptors" not in feats:
        raise KeyError("features must contain 'keypoints' and 'descriptors'")
    kpts, desc = np.asarray(feats["keypoints"]), np.asarray(feats["descriptors"])
    if kpts.ndim != 2 or kpts.shape[1] != 2:
        raise ValueError(f"Invalid keypoints shape: {kpts.shape}")
    N = kpts.shape[0]
    if desc.ndim != 2:
        raise ValueError(f"Invalid descriptors shape: {desc.shape}")
    if desc.shape[1] == N and desc.shape[0] != N:
        desc = desc.T
    elif desc.shape[0] == N:
        pass
    else:
        raise ValueError(f"Descriptor / keypoint mismatch: descriptors={desc.shape}, keypoints={kpts.shape}")
    out = dict(feats)
    out["keypoints"], out["descriptors"] = kpts, desc
    out.pop("feature_path", None)
    out.pop("im_path", None)
    return out


class _ResidentMatcherMixin:
    """What LightGlueMatcher and KorniaMatcher share: the resize policy of their two resident handles (``_net``: one pair per call, ``_net_b``:
    batched) and the one-pair hand-over through raw staging.  The matcher supplies ``_new_net(pairs, n)`` and, where a handle can go stale
    for another reason than its size, ``_stale(net)``."""

    def _stale(self, net) -> bool:
        return False

    def _dev(self):
        return self._device if isinstance(self._device, (str, torch.device)) else "cuda"

    def _ensure(self, n: int):
        if self._net is None or n > self._net_n or self._stale(self._net):
            # a handle is rebuilt when a pair has more keypoints than it holds (LightGlue ~0.5 - 1 s: weight splitting, uploads, allocations).  Since round 6 an
            # oversized handle costs nothing measurable (launch shapes follow the pair, not the handle: 2048 keypoints on a 4096 / 8192-row handle 1.464 / 1.485 vs
            # 1.461 ms, scripts/gpu_lg_capacity_cost.py) and a 4096-row handle is ~0.2 GB (the NN matcher's O(n^2 / 128) bytes), so on a GPU the first one already
            # holds 4096 keypoints per image
            floor = 4096 if str(getattr(self._dev(), "type", self._dev())).startswith("cuda") else 256
            self._net_n = max(floor, 1 << (max(n, 1) - 1).bit_length())
            self._net = self._new_net(1, self._net_n)

    def _ensure_pairs(self, n: int, pairs: int):
        """Batched instance (BatchedImageMatcher.match_pairs, tile_matching.BatchedTileMatchingMixin)."""
        cur = getattr(self, "_net_b", None)
        if cur is None or n > self._net_b_n or pairs > self._net_b_p or self._stale(cur):
            self._net_b_n = max(256, 1 << (max(n, 1) - 1).bit_length(), getattr(self, "_net_b_n", 0))
            self._net_b_p = max(pairs, getattr(self, "_net_b_p", 0))
            self._net_b = self._new_net(self._net_b_p, self._net_b_n)
        return self._net_b

    def _match_one_pair(self, tag: str, what: str, header, arrays, describe, cap: int, D: int, raw_floor: int, extra_out, match) -> np.ndarray:
        """One pair on ``self._net`` with ONE host-to-device and ONE device-to-host transfer.  ``header``: (byte offset, array) words of the first 256
        staging bytes; ``arrays``: the raw arrays, each at the next 256-byte boundary behind it; ``describe(base, offs)``: the two LgRawFeatures of
        dim_lg_stage_features, which builds the fp32 (N, D) feature table on the device; ``raw_floor``: bytes of device staging a handle-sized pair
        needs; ``extra_out(NK, dev)``: the matcher's output tensors besides the flat [n_matches (int32) | pad | matches NK x 2] buffer that comes
        back; ``match(kt, dt, rawd, out)``: the match_batch call.  The buffers live on a GPU in page-locked memory (``_staging``) and on the device in
        ``_lean``, rebuilt when the handle changed or a pair outgrew them.  Returns the (S, 2) int64 index pairs."""
        net = self._net
        dev = torch.device(net.device)
        on_gpu = dev.type == "cuda"
        NK = net.nk
        offs, cur = [], 256
        for arr in arrays:
            offs.append(cur)
            cur += (arr.nbytes + 255) & ~255
        nbytes_out = (2 + NK * 2) * 8
        if on_gpu:
            st = self.__dict__.setdefault("_staging", _PinnedStaging())
            pin, pout = st.get(tag + "_in", cur)[:cur], st.get(tag + "_out", nbytes_out)[:nbytes_out]
        else:
            pin, pout = torch.empty(cur, dtype=torch.uint8), torch.empty(nbytes_out, dtype=torch.uint8)
        pout = pout.view(torch.int64)
        h = pin.numpy()
        for o, words in header:
            h[o:o + words.nbytes] = words.view(np.uint8)
        for arr, o in zip(arrays, offs):
            if arr.nbytes:
                h[o:o + arr.nbytes] = arr.reshape(-1).view(np.uint8)
        lean = self.__dict__.get("_lean")
        tab_floats = 2 * cap * (2 + D)
        if lean is None or lean["net"] is not net or lean["raw"].numel() < cur or lean["tab"].numel() < tab_floats:
            flat = torch.zeros(2 + NK * 2, dtype=torch.int64, device=dev)
            out = {"matches": flat[2:].view(1, NK, 2), "scores": torch.zeros(1, NK, dtype=torch.float32, device=dev),
                   "n_matches": flat[:1].view(torch.int32)[:1], **extra_out(NK, dev)}
            lean = {"net": net, "raw": torch.empty(max(cur, raw_floor), dtype=torch.uint8, device=dev),
                    "tab": torch.empty(max(tab_floats, 2 * NK * (2 + D)), dtype=torch.float32, device=dev), "flat": flat, "out": out}
            self.__dict__["_lean"] = lean
        rawd, tab = lean["raw"], lean["tab"]
        descr = describe(rawd.data_ptr(), offs)
        kt, dt = tab[: 4 * cap].view(2, cap, 2), tab[4 * cap: 4 * cap + 2 * cap * D].view(2, cap, D)

        def run():
            rawd[:cur].copy_(pin, non_blocking=True)
            capi.check(net.lib, net.lib.dim_lg_stage_features(ctypes.byref(descr[0]), ctypes.byref(descr[1]), int(cap), int(D), capi.ptr(kt), capi.ptr(dt), net._stream()))
            match(kt, dt, rawd, lean["out"])
            pout.copy_(lean["flat"], non_blocking=True)   # enqueued behind the match: the range guard's synchronisation covers it

        net.guarded(run, what, logger)
        if on_gpu:
            torch.cuda.current_stream(dev).synchronize()
        res = pout.numpy()
        S = int(res[:1].view(np.int32)[0])
        return res[2:2 + 2 * S].reshape(S, 2).copy()


class _LightGluePairMixin(_ResidentMatcherMixin):
    """The per-pair hook LightGlueMatcher and LighterGlueMatcher share: features.h5's arrays -> one call on the resident ``self._net`` (a LightGlueHIP
    or a subclass of it, from the matcher's ``_new_net``), staged with one upload and one download on a GPU.  ``_stage_tag`` names the matcher's
    page-locked buffers, ``_what`` is its name in the range guard's log lines."""

    _stage_tag = "lg"
    _what = "LightGlue"

    @torch.no_grad()
    def _match_pairs(self, feats0: dict, feats1: dict) -> np.ndarray:
        """feats: numpy dicts as read from features.h5 (keypoints (N,2), descriptors (D,N) or (N,D),
        image_size (2,) = (H,W), + ignored keys).  Returns (S,2) int64 index pairs (LGX:102-125)."""
        f0, f1 = featuresDict2Lightglue(feats0), featuresDict2Lightglue(feats1)
        self._ensure(max(f0["keypoints"].shape[0], f1["keypoints"].shape[0]))

        def img(f):
            d = {"keypoints": torch.as_tensor(f["keypoints"], dtype=torch.float32)[None],
                 "descriptors": torch.as_tensor(f["descriptors"], dtype=torch.float32)[None]}
            if "image_size" in f:
                d["image_size"] = torch.as_tensor(np.asarray(f["image_size"]), dtype=torch.float32).reshape(1, 2)
            else:  # LGN:26-27: size inferred from the keypoint extent
                k = d["keypoints"][0]
                d["image_size"] = (1 + k.max(0).values - k.min(0).values).reshape(1, 2) if k.numel() else torch.ones(1, 2)
            return d

        dev = torch.device(self._net.device)
        if dev.type == "cuda":
            return self._match_pairs_staged(f0, f1, dev)
        res = self._net({"image0": img(f0), "image1": img(f1)})
        return res["matches"][0].cpu().numpy()

    def _match_pairs_staged(self, f0: dict, f1: dict, dev) -> np.ndarray:
        """The same call with ONE host-to-device and ONE device-to-host transfer (round 5) of the arrays AS THE CALLER HOLDS THEM (round 6).
        The reference's loop hands ``_match_pairs`` what features.h5 holds: float16 arrays, SuperPoint / ALIKED descriptors as (D, N)
        (extractors/extractor_base.py:56-99, extractors/superpoint.py:121-127).  Converting them on the host — numpy's half -> float cast through a
        transposed view — costs 1.2 - 1.6 ms per image, more than the whole match on the device; here the raw bytes of both images' keypoints and
        descriptors go straight into one page-locked buffer (a memcpy), up in one copy, and ``dim_lg_stage_features`` builds the fp32 (N, D)
        feature table on the device (transpose through LDS; fp16 -> fp32 is exact, so the table equals the host conversion's).  The match count
        and the (S, 2) index table share one device buffer and come back in one copy, enqueued behind the match so that the range guard's
        synchronisation covers it."""
        net = self._net
        D = net.input_dim

        def raw(f):
            k, d = f["keypoints"], f["descriptors"]
            if k.dtype not in (np.float16, np.float32):
                k = k.astype(np.float32)
            k = np.ascontiguousarray(k)
            if d.dtype not in (np.float16, np.float32):
                d = d.astype(np.float32)
            dn = 0
            if not d.flags.c_contiguous:
                if d.T.flags.c_contiguous:    # featuresDict2Lightglue's transposed view of a (D, N) array: keep the array
                    d, dn = d.T, 1
                else:
                    d = np.ascontiguousarray(d)
            return k, d, dn

        def size_of(f, k):   # LGN:26-27: size inferred from the keypoint extent when the features carry none
            if "image_size" in f:
                return np.asarray(f["image_size"], dtype=np.float32).reshape(2)
            k = np.asarray(k, dtype=np.float32)
            return (1 + k.max(0) - k.min(0)).astype(np.float32) if k.size else np.ones(2, np.float32)

        (k0, d0, dn0), (k1, d1, dn1) = raw(f0), raw(f1)
        m, n = k0.shape[0], k1.shape[0]
        if (m and (d0.shape[0] if dn0 else d0.shape[1]) != D) or (n and (d1.shape[0] if dn1 else d1.shape[1]) != D):
            raise ValueError(f"descriptor dimension {d0.shape} / {d1.shape} does not match the matcher's input_dim {D}")
        NK = net.nk
        f16 = lambda a: int(a.dtype == np.float16)
        return self._match_one_pair(
            self._stage_tag, self._what,
            [(0, np.concatenate([size_of(f0, k0), size_of(f1, k1)]).astype(np.float32)), (16, np.array((m, n), dtype=np.int32))],   # [sizes 4 f32 | counts 2 i32 | pad]
            (k0, d0, k1, d1),
            lambda base, offs: [capi.LgRawFeatures(base + offs[0], base + offs[1], m, f16(k0), f16(d0), dn0), capi.LgRawFeatures(base + offs[2], base + offs[3], n, f16(k1), f16(d1), dn1)],
            max(m, n, 1), D, 256 + 4 * 2 * NK * (2 + D) + 1024,
            lambda NK, dev: {"matches01": torch.zeros(1, 2, NK, dtype=torch.int32, device=dev), "mscores01": torch.zeros(1, 2, NK, dtype=torch.float32, device=dev),
                             "stop": torch.zeros(1, dtype=torch.int32, device=dev), "prune01": torch.zeros(1, 2, NK, dtype=torch.int32, device=dev)},
            lambda kt, dt, rawd, out: net.match_batch(kt, dt, rawd[16:24].view(torch.int32), rawd[:16].view(torch.float32).view(2, 2), n_pairs=1, out=out))


class LightGlueMatcher(_LightGluePairMixin, BatchedTileMatchingMixin, _MatcherBase):
    """matchers/lightglue.py:77 — LightGlue on the gfx950 library."""

    _default_conf = {
        "flash": True,   # accepted for compatibility; attention here is always the flash-attention kernel of lg_attn_x6.hip (fp16x3 / bf16x6 split arithmetic, lg_attn.hip in fp32 MFMA mode)
        "mp": False,
        "depth_confidence": 0.95,
        "width_confidence": 0.99,
        "filter_threshold": 0.1,
        "weights": None,
        # LGN:318-323,606-610: below this many keypoints the reference does not prune.  "auto" = what the reference
        # uses on a GPU (1536 with flash attention, 1024 without); -1 = its CPU behaviour (always prune), which is
        # what the CPU-generated parity goldens need.
        "pruning_min_kpts": "auto",
    }
    required_inputs = []
    min_matches = 20
    max_feat_no_tiling = 200000
    _input_dims = {"superpoint": 256, "disk": 128, "aliked": 128, "sift": 128}  # LGN:331-349

    def __init__(self, config, local_features="superpoint") -> None:
        self._localfeatures = local_features
        super().__init__(config)
        self._lib = capi.load()
        self._device = _resolve_device(self._device, "LightGlueMatcher")
        cfg = {**self._default_conf, **self.config.get("matcher", {})}
        self._arith = _apply_arithmetic(cfg, self._lib)
        self._on_sat = _saturation_policy(cfg)
        if cfg.get("mp"):
            logger.warning("LightGlue: mixed precision ('mp') is not implemented on the MI355X path; running fp32")
        self._conf = {k: cfg[k] for k in ("depth_confidence", "width_confidence", "filter_threshold")}
        self._conf["n_layers"] = int(cfg.get("n_layers", 9))
        pm = cfg.get("pruning_min_kpts", "auto")
        self._conf["pruning_min_kpts"] = (1536 if cfg.get("flash", True) else 1024) if pm == "auto" else int(pm)
        path = cfg.get("weights_path") or os.environ.get("DIM_LIGHTGLUE_WEIGHTS")
        in_dim = self._input_dims.get(local_features, 256)
        if path is None and cfg.get("allow_synthetic_weights"):
            logger.warning("LightGlue: running on seeded SYNTHETIC weights (allow_synthetic_weights) - test / benchmark use only")
        self._sd = _weights.load_lightglue_state_dict(path, input_dim=in_dim, n_layers=self._conf["n_layers"],
                                                      allow_synthetic=bool(cfg.get("allow_synthetic_weights", False)))
        self._net: Optional[LightGlueHIP] = None
        self._net_n = 0
        if self._localfeatures == "disk":
            self.max_feat_no_tiling = 50000

    def _new_net(self, pairs: int, n: int) -> LightGlueHIP:
        return LightGlueHIP(self._sd, self._conf, max_pairs=pairs, max_kpts=n, device=self._dev(), lib=self._lib, on_saturation=self._on_sat, arithmetic=self._arith)


class LighterGlueMatcher(_LightGluePairMixin, _MatcherBase):
    """matchers/lighterglue.py:78 — LighterGlue (LightGlue at 64 -> 96, one head, 6 layers) on the gfx950 library, quirks included:
    only ``local_features == "xfeat"``; the NETWORK's depth / width confidence are its own fixed (-1, 0.95) whatever the matcher config says (the
    reference never hands them on, matchers/lighterglue.py:102,222); ``filter_threshold`` is read from the config at every call (:221);
    ``image_size`` (H, W) reaches the network as (W, H) (:205-207 — LightGlueMatcher feeds (H, W)); a missing ``image_size`` is a ValueError (:193);
    the result is an (S, 2) int32 array (:241).  No BatchedTileMatchingMixin: the tile loop hands no ``image_size`` on, which this matcher
    refuses, so the reference's per-pair tile loop applies as it is."""

    _default_conf = {
        "flash": True,   # accepted for compatibility: attention is always the flash-attention kernel of lg_attn_d96.hip
        "mp": False,
        "depth_confidence": 0.95,   # (ignored, as in the reference)
        "width_confidence": 0.99,   # (ignored, as in the reference)
        "filter_threshold": 0.1,
        "weights": None,
        "pruning_min_kpts": "auto",   # as LightGlueMatcher: "auto" = the reference's GPU value, -1 = its CPU behaviour (always prune)
    }
    required_inputs = []
    min_matches = 20
    max_feat_no_tiling = 200000
    _stage_tag = "lgl"
    _what = "LighterGlue"
    # thirdparty/accelerated_features/modules/lighterglue.py:12-27: what LightGlue(None) is built with
    _network_conf = {"n_layers": 6, "depth_confidence": -1, "width_confidence": 0.95}

    def __init__(self, config, local_features="superpoint") -> None:
        self._localfeatures = local_features
        super().__init__(config)
        if self._localfeatures != "xfeat":
            raise ValueError(f"Unsupported local feature extractor: {self._localfeatures}")
        self._lib = capi.load()
        self._device = _resolve_device(self._device, "LighterGlueMatcher")
        cfg = {**self._default_conf, **self.config.get("matcher", {})}
        self._arith = _apply_arithmetic(cfg, self._lib)
        self._on_sat = _saturation_policy(cfg)
        if cfg.get("mp"):
            logger.warning("LighterGlue: mixed precision ('mp') is not implemented on the MI355X path; running the split fp32-class arithmetic")
        pm = cfg.get("pruning_min_kpts", "auto")
        self._conf = {**self._network_conf, "filter_threshold": float(cfg["filter_threshold"]),
                      "pruning_min_kpts": (1536 if cfg.get("flash", True) else 1024) if pm == "auto" else int(pm)}
        path = cfg.get("weights_path")
        if path is None and not os.environ.get("DIM_LIGHTERGLUE_WEIGHTS") and cfg.get("allow_synthetic_weights"):
            logger.warning("LighterGlue: running on seeded SYNTHETIC weights (allow_synthetic_weights) - test / benchmark use only")
        self._sd = _weights.load_lighterglue_state_dict(path, allow_synthetic=bool(cfg.get("allow_synthetic_weights", False)))
        self._net: Optional[LighterGlueHIP] = None
        self._net_n = 0

    def _new_net(self, pairs: int, n: int) -> LighterGlueHIP:
        return LighterGlueHIP(self._sd, self._conf, max_pairs=pairs, max_kpts=n, device=self._dev(), lib=self._lib, on_saturation=self._on_sat, arithmetic=self._arith)

    def _stale(self, net) -> bool:
        """The threshold lives in the handle: a call with another ``filter_threshold`` in the config gets a new one."""
        self._conf["filter_threshold"] = float(self.config["matcher"]["filter_threshold"])
        return float(net.conf["filter_threshold"]) != self._conf["filter_threshold"]

    @staticmethod
    def _size_as_the_network_sees_it(f: dict) -> np.ndarray:
        """matchers/lighterglue.py:174-207: unwrap, int32, float32, (H, W) -> (W, H)."""
        s = f["image_size"]
        if isinstance(s, (list, tuple)):
            s = s[0]
        if isinstance(s, torch.Tensor):
            s = s.cpu().numpy()
        s = np.asarray(s, dtype=np.int32).astype(np.float32).reshape(-1)
        return np.array([s[1], s[0]], dtype=np.float32)

    @torch.no_grad()
    def _match_pairs(self, feats0: dict, feats1: dict) -> np.ndarray:
        """feats: numpy dicts as read from features.h5 (keypoints (N, 2), descriptors (N, 64) or (64, N), float16 or float32, image_size (H, W)).
        Returns (S, 2) int32 index pairs."""
        if "image_size" not in feats0 or "image_size" not in feats1:
            raise ValueError("image_size not found in features - required by XFeat's match_lighterglue")
        f0 = {**feats0, "image_size": self._size_as_the_network_sees_it(feats0)}
        f1 = {**feats1, "image_size": self._size_as_the_network_sees_it(feats1)}
        return super()._match_pairs(f0, f1).astype(np.int32)


class SuperGlueMatcher(_ResidentMatcherMixin, _MatcherBase):
    """matchers/superglue.py:54 — SuperGlue on the gfx950 library, quirks included: the class's ``default_config`` (20 iterations / 0.3) is never
    merged (MatcherBase merges ``_default_conf``, empty in the base), so a matcher section without ``sinkhorn_iterations`` / ``match_threshold``
    runs the NETWORK's defaults, 100 / 0.2 (SGN:212-219); ``weights`` must be "indoor" or "outdoor" (SGN:244); ``scores`` and ``image_size`` are
    required; ``image_size`` (H, W) gives image0 its shape (1, 1, H, W), so the network normalises with width = image_size[1]; every other key of
    the feature dicts is ignored; the result is the (S, 2) int64 array of (i, matches0[i]), ascending in i.  Both per-call values are read from
    the config at every call.  No BatchedTileMatchingMixin: tiled pairs go through the reference's per-pair tile loop as they are."""

    default_config = {"name": "superglue", "weights": "outdoor", "sinkhorn_iterations": 20, "match_threshold": 0.3}   # (as in the reference: not merged)
    _default_conf: dict = {}
    required_inputs = []
    min_matches = 20
    max_feat_no_tiling = 50000
    _network_conf = {"weights": "outdoor", "sinkhorn_iterations": 100, "match_threshold": 0.2}   # SuperGlue.default_config (SGN:212-219)

    def __init__(self, config) -> None:
        super().__init__(config)
        self._lib = capi.load()
        self._device = _resolve_device(self._device, "SuperGlueMatcher")
        cfg = {**self._network_conf, **self.config.get("matcher", {})}
        if cfg["weights"] not in ("indoor", "outdoor"):
            raise ValueError(f"SuperGlue weights must be 'indoor' or 'outdoor', got {cfg['weights']!r}")
        self._arith = _apply_arithmetic(cfg, self._lib)
        self._on_sat = _saturation_policy(cfg)
        path = cfg.get("weights_path")
        if path is None and not os.environ.get("DIM_SUPERGLUE_WEIGHTS") and cfg.get("allow_synthetic_weights"):
            logger.warning("SuperGlue: running on seeded SYNTHETIC weights (allow_synthetic_weights) - test / benchmark use only")
        self._sd = _weights.load_superglue_state_dict(path, allow_synthetic=bool(cfg.get("allow_synthetic_weights", False)))
        self._net: Optional[SuperGlueHIP] = None
        self._net_n = 0

    def _new_net(self, pairs: int, n: int) -> SuperGlueHIP:
        return SuperGlueHIP(self._sd, None, max_pairs=pairs, max_kpts=n, device=self._dev(), lib=self._lib, on_saturation=self._on_sat, arithmetic=self._arith)

    def _ensure(self, n: int):
        # the score block is max_kpts^2 floats: the handle follows the pair in steps of 1024 (a 4096-row floor as LightGlue's would pin 64 MiB for
        # nothing, the shipped configuration's 8000 keypoints take 256 MiB)
        if self._net is None or n > self._net_n:
            on_gpu = str(getattr(self._dev(), "type", self._dev())).startswith("cuda")
            self._net_n = max(1024 if on_gpu else 64, (max(n, 1) + 1023) // 1024 * 1024 if on_gpu else 1 << (max(n, 1) - 1).bit_length())
            self._net = self._new_net(1, self._net_n)

    @torch.no_grad()
    def _match_pairs(self, feats0: dict, feats1: dict) -> np.ndarray:
        """feats: numpy dicts as read from features.h5 (keypoints (N, 2), descriptors (256, N) — or (N, 256) —, scores (N,), float16 or float32,
        image_size (H, W), + ignored keys).  Returns (S, 2) int64 index pairs."""
        cfg = {**self._network_conf, **self.config.get("matcher", {})}
        iters, thr = int(cfg["sinkhorn_iterations"]), float(cfg["match_threshold"])
        fs = []
        for f in (feats0, feats1):
            for key in ("scores", "image_size"):
                if key not in f:
                    raise ValueError(f"{key} not found in features - required by SuperGlue")
            g = featuresDict2Lightglue({k: f[k] for k in ("keypoints", "descriptors", "scores", "image_size")})
            size = np.asarray(g["image_size"], dtype=np.float32).astype(int).reshape(-1)   # matchers/superglue.py:38: float, then int
            fs.append((np.asarray(g["keypoints"], dtype=np.float32), np.asarray(g["descriptors"], dtype=np.float32),
                       np.asarray(g["scores"], dtype=np.float32).reshape(-1), (int(size[0]), int(size[1]))))
        (k0, d0, s0, hw0), (k1, d1, s1, hw1) = fs
        m, n = k0.shape[0], k1.shape[0]
        if m == 0 or n == 0:   # SGN:255-262: nothing matches
            return np.zeros((0, 2), dtype=np.int64)
        if d0.shape[1] != 256 or d1.shape[1] != 256:
            raise ValueError(f"descriptor dimension {d0.shape} / {d1.shape}: SuperGlue takes 256-wide descriptors")
        self._ensure(max(m, n))
        net = self._net
        dev = torch.device(net.device)
        cap = max(m, n)
        kt, dt, sc = np.zeros((2, cap, 2), np.float32), np.zeros((2, cap, 256), np.float32), np.zeros((2, cap), np.float32)
        kt[0, :m], kt[1, :n], dt[0, :m], dt[1, :n], sc[0, :m], sc[1, :n] = k0, k1, d0, d1, s0, s1
        st = np.array([[hw0[1], hw0[0]], [hw1[1], hw1[0]]], dtype=np.float32)   # the library takes (width, height)
        up = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
        o = net.match_batch_guarded(up(kt), up(dt), up(sc), torch.tensor([m, n], dtype=torch.int32, device=dev), up(st), n_pairs=1,
                                    sinkhorn_iterations=iters, match_threshold=thr, logger=logger)
        S = int(o["n_matches"][0].item())
        return o["matches"][0, :S].cpu().numpy().astype(np.int64)


class KorniaMatcher(_ResidentMatcherMixin, BatchedTileMatchingMixin, _MatcherBase):
    """matchers/kornia_matcher.py:9 — kornia.feature.DescriptorMatcher(match_mode, th) on the gfx950 library (csrc/nn_match.hip): the matcher of the
    shipped ``superpoint+kornia_matcher`` pipeline and of the SIFT / KeyNet / DeDoDe pipelines.  match_mode nn / mnn / snn / smnn; kornia's other
    modes (fginn, adalam, lightglue) are rejected here, at construction.  The match list is always idx0-ascending (kornia's mnn lists by idx1 when
    image 0 has more descriptors: the same set)."""

    _default_conf = {
        "name": "kornia_matcher",
        "match_mode": "smnn",
        "th": 0.8,
    }
    required_inputs = []
    min_matches = 20
    max_feat_no_tiling = 200000

    def __init__(self, config) -> None:
        super().__init__(config)
        self._lib = capi.load()
        self._device = _resolve_device(self._device, "KorniaMatcher")
        cfg = {**self._default_conf, **self.config.get("matcher", {})}
        self._mode, self._th = _check_nn_mode(cfg["match_mode"]), float(cfg["th"])
        self._arith = _apply_arithmetic(cfg, self._lib)
        self._on_sat = _saturation_policy(cfg)
        self._dim = int(cfg.get("descriptor_size", 256))   # follows the features: every _match_pairs / batched call sets it (_set_dim)
        self._net: Optional[NearestNeighborHIP] = None
        self._net_n = 0

    def _set_dim(self, dim: int) -> None:
        self._dim = int(dim)

    def _new_net(self, pairs: int, n: int) -> NearestNeighborHIP:
        return NearestNeighborHIP(self._mode, self._th, dim=self._dim, max_pairs=pairs, max_kpts=n, device=self._dev(), lib=self._lib,
                                  on_saturation=self._on_sat, arithmetic=self._arith)

    def _stale(self, net) -> bool:
        return net.input_dim != self._dim   # the handle is built for one descriptor width

    @torch.no_grad()
    def _match_pairs(self, feats0: dict, feats1: dict) -> np.ndarray:
        """feats: numpy dicts as read from features.h5; only "descriptors" is used, (D, N) as the reference stores them (KMX:36-37 transposes),
        float16 or float32, C-contiguous or the transposed view of an (N, D) array.  Returns (S, 2) int64 index pairs (KMX:46-53).
        One upload of the raw bytes, dim_lg_stage_features builds the fp32 (N, D) table on the device, one download of [count | list]."""

        def raw(f):
            d = f["descriptors"]
            d = np.asarray(d[0] if isinstance(d, (list, tuple)) else d)
            if d.ndim != 2:
                raise ValueError(f"Invalid descriptors shape: {d.shape}")
            if d.dtype not in (np.float16, np.float32):
                d = d.astype(np.float32)
            if d.T.flags.c_contiguous and not d.flags.c_contiguous:
                return d.T, 0, d.shape[0], d.shape[1]          # the (N, D) array behind a transposed view
            return np.ascontiguousarray(d), 1, d.shape[0], d.shape[1]

        def widen(r):
            """The matcher's k-steps need a width that is a multiple of 64: any other width (ALIKE-s: 96) gets zero columns up to the next
            multiple, which leave every distance and ratio as they were (the device-side route to the same table is dim_alike_config.desc_stride)"""
            d, dn, D, cnt = r
            if D % 64 == 0 or D == 0:
                return r
            nd = d.T if dn else d                                   # (N, D)
            wide = np.zeros((nd.shape[0], (D + 63) // 64 * 64), dtype=nd.dtype)
            wide[:, :D] = nd
            return wide, 0, wide.shape[1], cnt

        (d0, dn0, D0, m), (d1, dn1, D1, n) = widen(raw(feats0)), widen(raw(feats1))
        if D0 != D1 or D0 % 64 != 0:
            raise ValueError(f"descriptor dimensions {D0} / {D1}: both images need the same width")
        D = D0
        self._set_dim(D)
        self._ensure(max(m, n))
        net, NK = self._net, self._net.nk
        f16 = [int(d0.dtype == np.float16), int(d1.dtype == np.float16)]
        exact = bool(f16[0] and f16[1])      # float16 inputs: every table value has a zero low piece (one MFMA term instead of three, same bits)
        return self._match_one_pair(
            "nn", "KorniaMatcher", [(0, np.array((m, n), dtype=np.int32))], (d0, d1),                                       # [counts 2 i32 | pad]
            # the staging kernel converts keypoints too; this matcher has none to give it: it reads the first 2 n descriptor values as stand-ins (into kt, unused)
            lambda base, offs: [capi.LgRawFeatures(base + offs[0], base + offs[0], m, f16[0], f16[0], dn0), capi.LgRawFeatures(base + offs[1], base + offs[1], n, f16[1], f16[1], dn1)],
            max(m, n, 1), D, 256 + 4 * 2 * NK * D + 1024, lambda NK, dev: {},
            lambda kt, dt, rawd, out: net.match_batch(None, dt, rawd[:8].view(torch.int32), None, n_pairs=1, out=out, f16_exact=exact))
