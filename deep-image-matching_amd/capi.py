"""ctypes binding of libdim_hip.so (the C ABI declared in include/dim_hip.h).

There is deliberately no CPU fallback: if the gfx950 library cannot be loaded
or no GPU is visible, loading fails with an exception."""
from __future__ import annotations

import contextlib
import ctypes
import math
from pathlib import Path

import torch

_LIB = None
_INSTALLED_DEVICE = None
LIB_PATH = Path(__file__).resolve().parent / "lib" / "libdim_hip.so"


class DimHipError(RuntimeError):
    pass


def load(path: str | None = None) -> ctypes.CDLL:
    global _LIB
    if _LIB is not None and path is None:
        return _LIB
    p = Path(path) if path else LIB_PATH
    if not p.exists():
        raise DimHipError(f"{p} not found: build it with `python __graft_entry__.py build` (hipcc --offload-arch=gfx950)")
    lib = ctypes.CDLL(str(p))
    lib.dim_last_error.restype = ctypes.c_char_p
    if path is None:
        _LIB = lib
    return lib


def install(lib, device: str = "cpu") -> None:
    """TEST HOOK (tests/ only): make ``load()`` return an already opened library object — the CPU tests install the
    emulator build of the same sources here, with ``device`` = "cpu" — instead of injecting it through the plugin
    constructors.  ``install(None)`` restores the product behaviour.  The package itself never calls this."""
    global _LIB, _INSTALLED_DEVICE
    _LIB, _INSTALLED_DEVICE = lib, (device if lib is not None else None)
    if lib is not None:
        lib.dim_last_error.restype = ctypes.c_char_p


def installed_device():
    """Device forced by ``install`` (None in the product: the plugins then use their own device)."""
    return _INSTALLED_DEVICE


class LgRawFeatures(ctypes.Structure):
    """include/dim_hip.h: dim_lg_raw_features (one image's keypoints / descriptors as uploaded, for dim_lg_stage_features)."""
    _fields_ = [("kpts_dev", ctypes.c_void_p), ("desc_dev", ctypes.c_void_p), ("n", ctypes.c_int), ("kpts_f16", ctypes.c_int),
                ("desc_f16", ctypes.c_int), ("desc_is_dn", ctypes.c_int)]


NN_MODES = {"nn": 0, "mnn": 1, "snn": 2, "smnn": 3}  # DIM_NN_MODE_*


class NnConfig(ctypes.Structure):
    """include/dim_hip.h: dim_nn_config."""
    _fields_ = [("mode", ctypes.c_int), ("th", ctypes.c_double)]


def declare_nn(lib) -> None:
    """Argument / result types of the dim_nn_* entry points (idempotent; called by NearestNeighborHIP on the library it uses)."""
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.dim_nn_create.argtypes = [ctypes.POINTER(NnConfig), ci, ci, ci, ctypes.POINTER(vp)]
    lib.dim_nn_create.restype = ci
    lib.dim_nn_destroy.argtypes = [vp]
    lib.dim_nn_destroy.restype = None
    lib.dim_nn_max_kpts.argtypes = [vp]
    lib.dim_nn_max_kpts.restype = ci
    lib.dim_nn_workspace_bytes.argtypes = [vp]
    lib.dim_nn_workspace_bytes.restype = ctypes.c_size_t
    lib.dim_nn_match.argtypes = [vp, vp, vp, ci, ci, vp, ci, vp, vp, vp, vp, vp, vp]
    lib.dim_nn_match.restype = ci


def check(lib, rc: int) -> None:
    if rc != 0:
        msg = lib.dim_last_error().decode(errors="replace")
        if "out of memory" in msg.lower():
            # keep the substring the reference's tile fallback keys on (matcher_base.py:251-256)
            raise DimHipError("CUDA out of memory (HIP): " + msg)
        raise DimHipError(msg)


def ptr(t):
    """Device (or, under the test emulator, host) pointer of a torch tensor / None."""
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream_ptr(device):
    """The ``void* stream`` argument of the C ABI: the CURRENT torch stream of ``device``, resolved at every call (None, the null
    stream, off the GPU: the test emulator)."""
    device = torch.device(device)
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream) if device.type == "cuda" else None


def device_ctx(device):
    """The library launches on the CURRENT HIP device: a context that makes it ``device``."""
    device = torch.device(device)
    return torch.cuda.device(device) if device.type == "cuda" else contextlib.nullcontext()


def copy_from_device(lib, addr: int, shape, device) -> torch.Tensor:
    """Copy a raw fp32 device buffer into a CPU tensor (hipMemcpy through torch)."""
    n = math.prod(shape)
    if device.type == "cuda":
        torch.cuda.synchronize(device)
        out = torch.empty(n, dtype=torch.float32, device=device)
        rc = ctypes.CDLL("libamdhip64.so").hipMemcpy(ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(addr), ctypes.c_size_t(n * 4), 3)
        if rc != 0:
            raise DimHipError(f"hipMemcpy failed: {rc}")
        return out.cpu().reshape(shape)
    buf = (ctypes.c_float * n).from_address(addr)
    return torch.frombuffer(buf, dtype=torch.float32).clone().reshape(shape)


# ---- arithmetic selection and the fp16x3 range guard ------------------------------------------------------
ARITHMETIC = {"fp16x3": 2, "bf16x6": 1, "fp32": 0}
SAT_SITES = 16  # DIM_SAT_SITES
SAT_NAMES = ["sp_image", "sp_encoder", "sp_heads", "lg_input", "lg_qkv", "lg_ffn", "lg_desc", "op", "aliked", "alike", "xfeat", "netvlad", "ripe"]
_arith = {}  # id(lib) -> current mode (the library default is fp16x3)


def get_arithmetic(lib) -> int:
    return _arith.get(id(lib), 2)


def set_arithmetic(lib, mode) -> int:
    """Process-wide DEFAULT matrix arithmetic (dim_tune_set key 1); returns the previous mode.  Handles may override it for themselves
    (set_handle_arithmetic)."""
    mode = ARITHMETIC[mode] if isinstance(mode, str) else int(mode)
    prev = get_arithmetic(lib)
    lib.dim_tune_set(1, mode)
    _arith[id(lib)] = mode
    return prev


def set_handle_arithmetic(lib, handle, mode) -> None:
    """Matrix arithmetic of ONE extractor / matcher handle (dim_handle_tune_set key 1); ``None`` = back to the process default."""
    v = -1 if mode is None else (ARITHMETIC[mode] if isinstance(mode, str) else int(mode))
    check(lib, lib.dim_handle_tune_set(handle, 1, v))


def saturation(lib, stream=None, reset: bool = True):
    """(total, {site: count}) of the fp16x3 range-guard counters (dim_saturation_read; synchronises `stream`)."""
    counts = (ctypes.c_uint * SAT_SITES)()
    total = ctypes.c_ulonglong()
    check(lib, lib.dim_saturation_read(counts, ctypes.byref(total), int(reset), stream))
    named = {SAT_NAMES[i] if i < len(SAT_NAMES) else str(i): int(counts[i]) for i in range(SAT_SITES) if counts[i]}
    return int(total.value), named


class SaturationError(DimHipError):
    pass


def run_guarded(lib, stream, fn, what: str, policy: str = "fallback", logger=None, handle=None, arithmetic=None):
    """Runs ``fn()`` (one extract / match call enqueued on ``stream``) under the fp16x3 range guard: when the
    default arithmetic is active and a kernel reported a value outside the exact range of the fp16 split
    (|x| > 4094), the call is repeated in bf16x6 (no range limit; policy "fallback") or a SaturationError is
    raised (policy "raise").  Synchronises the stream.  Other arithmetic modes run unguarded.
    ``handle`` / ``arithmetic``: the library handle ``fn`` calls and its own arithmetic override (None = process default) — the re-run then
    switches THAT handle to bf16x6 (dim_handle_tune_set) instead of the process-wide default, so other handles / threads are not affected."""
    mode = get_arithmetic(lib) if arithmetic is None else (ARITHMETIC[arithmetic] if isinstance(arithmetic, str) else int(arithmetic))
    if mode != 2 or policy == "off":
        return fn()
    check(lib, lib.dim_saturation_reset(stream))  # drop anything a previous unguarded call left behind (one enqueued memset: no read-back, no synchronisation)
    out = fn()
    total, sites = saturation(lib, stream, reset=True)
    if total == 0:
        return out
    if policy == "raise":
        raise SaturationError(f"{what}: fp16x3 range exceeded at {sites}; set arithmetic='bf16x6'")
    if logger is not None:
        logger.warning("%s: fp16x3 range exceeded at %s - repeating the call in bf16x6", what, sites)
    if handle is not None:
        set_handle_arithmetic(lib, handle, 1)
        try:
            return fn()
        finally:
            set_handle_arithmetic(lib, handle, arithmetic)
    prev = set_arithmetic(lib, 1)
    try:
        return fn()
    finally:
        set_arithmetic(lib, prev)


class ResidentHandle:
    """Base of the four wrappers of a resident ``dim_*_create`` handle: ``lib`` / ``device`` / ``_h``, the no-fallback rule, create and
    (idempotent) destroy, the stream / device context of a call and the fp16x3 range guard around one."""

    _destroy = ""   # name of the C destroy function
    _h = None       # null until create succeeded, None again after destroy

    def _open(self, device, lib, on_saturation="fallback", arithmetic=None):
        self.arithmetic = arithmetic        # None: the process default (set_arithmetic); "fp16x3" | "bf16x6" | "fp32": this handle only
        self.on_saturation = on_saturation  # fp16x3 range guard policy: "fallback" (bf16x6 re-run) | "raise" | "off"
        self.lib = lib if lib is not None else load()
        self.device = torch.device(device)
        if self.device.type != "cuda" and lib is None and installed_device() is None:
            raise DimHipError(f"{type(self).__name__} needs a HIP device; there is no CPU fallback")
        self._h = ctypes.c_void_p()
        self._keep = []

    def _host(self, t) -> int:
        """Address of ``t`` as contiguous fp32 host memory, kept alive until ``_create`` returns."""
        t = t.detach().float().contiguous().cpu()
        self._keep.append(t)
        return t.data_ptr()

    def _create(self, create, *args):
        """``create(*args, &handle)`` on the handle's device, then the handle's own arithmetic."""
        try:
            with self._ctx():
                check(self.lib, create(*args, ctypes.byref(self._h)))
        finally:
            self._keep = []
        if self.arithmetic is not None:
            set_handle_arithmetic(self.lib, self._h, self.arithmetic)

    def __del__(self):
        h, self._h = self._h, None
        if h:
            getattr(self.lib, self._destroy)(h)

    def _stream(self):
        return stream_ptr(self.device)

    def _ctx(self):
        return device_ctx(self.device)

    def guarded(self, fn, what: str, logger=None, policy=None):
        """``fn()`` (calls on this handle, enqueued on the current stream) under the fp16x3 range guard (run_guarded): synchronises."""
        with self._ctx():
            return run_guarded(self.lib, self._stream(), fn, what, self.on_saturation if policy is None else policy, logger,
                               handle=self._h, arithmetic=self.arithmetic)
