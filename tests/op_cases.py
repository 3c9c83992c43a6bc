"""Operator-level cases shared by the emulator tests (tests/test_ops_emu.py) and the hardware tests (tests/test_ops_gpu.py).

Every builder takes (lib, ..., device="cpu", runs=1):
  * the inputs come from a seeded CPU generator and are copied to `device`;
  * every output is allocated on `device`, pre-filled with SENTINEL and surrounded by a guard band (extra rows past M and ldc > N for
    matrices, extra trailing elements for dense tensors) that the operator must leave alone — on hardware an out-of-bounds store
    corrupts silently and the band is the only thing that shows it;
  * the library call is made `runs` times on the same inputs, each time into a fresh output, and synchronised when device != "cpu";
  * the result comes back on the CPU with the fp64 reference and the error scale (OpResult).
No tuning key is touched here: the tests set dim_tune_set keys inside try / finally.  The inputs and their fp64 references are cached per case
(they do not depend on the library or on a tuning key), so the variants of one kernel share one reference; nothing that is returned may be
modified by a caller.
"""
import ctypes
import functools
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

from oracle import superpoint_ref

SENTINEL = -7.0
GUARD_ROWS, GUARD_COLS, GUARD_ELEMS = 3, 8, 4096

SELU_LAMBDA, SELU_ALPHA = 1.0507009873554804934193349852946, 1.6732632423543772848170429916717


def p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class OpResult(NamedTuple):
    out: torch.Tensor                 # the live region of the first run (CPU)
    ref: torch.Tensor                 # fp64 (or bit-exact) reference, same shape as out
    scale: Optional[torch.Tensor]     # what the relative metric of this operator divides by (None: absolute / bit-exact)
    guard_ok: bool                    # every run left the whole guard band at SENTINEL
    raws: tuple                       # the full output buffers of all runs, guard band included (CPU)

    @property
    def repeatable(self):
        """All runs wrote the same bits (trivially true for one run)."""
        return all(torch.equal(self.raws[0], r) for r in self.raws[1:])

    @property
    def abs_err(self):
        return (self.out.double() - self.ref.double()).abs()

    @property
    def rel_err(self):
        return (self.abs_err / self.scale).max().item()


def _sync(device):
    if device != "cpu":
        torch.cuda.synchronize()


def _matrix_out(M, N, device):
    """[M + GUARD_ROWS][N + GUARD_COLS] of SENTINEL; the operator gets ldc = N + GUARD_COLS (same residue mod 8 as N: the same store path)."""
    return torch.full((M + GUARD_ROWS, N + GUARD_COLS), SENTINEL, device=device), N + GUARD_COLS


def _matrix_result(bufs, M, N, ref, scale):
    raws = tuple(b.cpu() for b in bufs)
    ok = all(bool((r[M:] == SENTINEL).all()) and bool((r[:, N:] == SENTINEL).all()) for r in raws)
    return OpResult(raws[0][:M, :N], ref, scale, ok, raws)


def _dense_out(numel, device):
    return torch.full((numel + GUARD_ELEMS,), SENTINEL, device=device)


def _dense_result(bufs, shape, ref, scale):
    raws = tuple(b.cpu() for b in bufs)
    n = 1
    for d in shape:
        n *= d
    ok = all(bool((r[n:] == SENTINEL).all()) for r in raws)
    return OpResult(raws[0][:n].view(*shape), ref, scale, ok, raws)


# ---------------------------------------------------------------------------------------------------------------- simple_nms
def nms_tie_map(radius):
    """2 x 45 x 70 (no multiple of a tile; the image border logic): heavy ties / plateaus (SURVEY App. D KATs)."""
    g = torch.Generator().manual_seed(radius)
    s = torch.rand(2, 45, 70, generator=g)
    s[0] = (s[0] * 6).round() / 6 + 0.01
    s[1, 10:20, 10:30] = 0.5
    return s


def nms_partial_tile_map(radius):
    """1 x 75 x 130: partial 64 x 64 tiles on both axes, quantised rows and a plateau."""
    g = torch.Generator().manual_seed(40 + radius)
    s = torch.rand(1, 75, 130, generator=g)
    s[0, :40] = (s[0, :40] * 5).round() / 5 + 0.01
    s[0, 50:70, 60:100] = 0.5
    return s


@functools.lru_cache(maxsize=1)
def nms_large_map():
    """4 x 500 x 500: 8 * 8 * 4 = 256 tiles of 64 x 64, the count at which launch_nms picks the 64 x 64 kernel by itself; quantised
    maps (ties everywhere), plateaus across tile seams at 64 and 32, and plain noise."""
    g = torch.Generator().manual_seed(500)
    s = torch.rand(4, 500, 500, generator=g)
    s[0] = (s[0] * 6).round() / 6 + 0.01
    s[1, :, :250] = (s[1, :, :250] * 50).round() / 50
    s[2, 50:80, 40:300] = 0.5
    s[2, 300:420, 250:262] = 0.75
    s[3, 490:, :] = 0.25
    s[3, :, 495:] = 0.25
    return s


def nms_case(lib, s, radius, device="cpu", runs=1):
    """dim_op_simple_nms_f32 vs oracle.superpoint_ref.simple_nms (bit-exact: scale None)."""
    B, H, W = s.shape
    sd = s.to(device).contiguous()
    bufs = []
    for _ in range(runs):
        out = _dense_out(B * H * W, device)
        assert lib.dim_op_simple_nms_f32(p(sd), p(out), B, H, W, radius, None) == 0, lib.dim_last_error()
        _sync(device)
        bufs.append(out)
    return _dense_result(bufs, (B, H, W), superpoint_ref.simple_nms(s, radius), None)


# ---------------------------------------------------------------------------------------------------------------- fp32 GEMM
@functools.lru_cache(maxsize=2)
def _gemm_f32_inputs(M, N, K, bt):
    g = torch.Generator().manual_seed(M)
    A = torch.randn(M, K, generator=g)
    B = torch.randn(N, K, generator=g) if bt else torch.randn(K, ((N + 3) // 4) * 4, generator=g)
    bias, R = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    Bd = B.double()
    ref = torch.relu((A.double() @ Bd.T if bt else A.double() @ Bd[:, :N]) + bias.double() + R.double())
    return A, B, bias, R, ref


def gemm_f32_case(lib, M, N, K, bt, device="cpu", runs=1):
    """relu(A B + bias + R) through dim_op_gemm_f32 (gemm_mfma_kernel<bt>, 128 x 128 blocks); B is [N][K] when bt else [K][ldb >= N]."""
    A, B, bias, R, ref = _gemm_f32_inputs(M, N, K, bt)
    Ad, Bd, bd, Rd = (t.to(device).contiguous() for t in (A, B, bias, R))
    bufs = []
    for _ in range(runs):
        C, ldc = _matrix_out(M, N, device)
        assert lib.dim_op_gemm_f32(p(Ad), K, p(Bd), B.shape[1], bt, p(bd), p(Rd), N, p(C), ldc, M, N, K, 1, None) == 0, lib.dim_last_error()
        _sync(device)
        bufs.append(C)
    return _matrix_result(bufs, M, N, ref, None)


# ---------------------------------------------------------------------------------------------------------------- split-precision GEMM
def selu64(x):
    return torch.where(x > 0, SELU_LAMBDA * x, SELU_LAMBDA * SELU_ALPHA * torch.expm1(x.clamp(max=0.0)))


@functools.lru_cache(maxsize=2)
def _gemm_x6_inputs(M, N, K, act, with_bias, with_residual):
    g = torch.Generator().manual_seed(K + M)
    A, W = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g).contiguous()
    bias, R = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    pre = A.double() @ W.double()
    if with_bias:
        pre = pre + bias.double()
    if with_residual:
        pre = pre + R.double()
    ref = torch.relu(pre) if act == 1 else selu64(pre) if act == 2 else pre
    mag = A.abs().double() @ W.abs().double()
    return A, W, bias if with_bias else None, R if with_residual else None, ref, mag


def gemm_x6_case(lib, M, N, K, act=0, bias=True, residual=True, device="cpu", runs=1):
    """act(A W + bias + R) through dim_x3_create + dim_op_gemm_x6_f32 in the split mode that is active at the call (the residual is added
    BEFORE the activation: gemm_x6.hip's epilogue); act 0 none / 1 ReLU / 2 SELU.  scale = |A| |W| (the pre-activation error scale)."""
    A, W, b, R, ref, mag = _gemm_x6_inputs(M, N, K, act, bool(bias), bool(residual))
    dev, npad = ctypes.c_void_p(), ctypes.c_int()
    assert lib.dim_x3_create(p(W), K, N, ctypes.byref(dev), ctypes.byref(npad)) == 0, lib.dim_last_error()
    bufs = []
    try:
        Ad = A.to(device).contiguous()
        bd = b.to(device).contiguous() if b is not None else None
        Rd = R.to(device).contiguous() if R is not None else None
        for _ in range(runs):
            C, ldc = _matrix_out(M, N, device)
            rc = lib.dim_op_gemm_x6_f32(p(Ad), K, dev, npad.value, p(bd), p(Rd), N if R is not None else 0, p(C), ldc, M, N, K, act, None)
            assert rc == 0, lib.dim_last_error()
            _sync(device)
            bufs.append(C)
    finally:
        lib.dim_x3_destroy(dev)
    return _matrix_result(bufs, M, N, ref, mag)


def selu_bound(mag, e=4e-7):
    """|err| bound after SELU for a pre-activation error of e * mag: lambda * alpha (SELU's Lipschitz constant) times that, plus a 4-ulp budget
    for expf on values of at most 1, scaled by lambda * alpha."""
    la = SELU_LAMBDA * SELU_ALPHA
    return la * e * mag + 4 * 2.0 ** -23 * la


@functools.lru_cache(maxsize=2)
def _gemm_nt_inputs(M, N, K):
    g = torch.Generator().manual_seed(M + N)
    A, B = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    return A, B, A.double() @ B.double().t(), A.double().abs() @ B.double().abs().t()


def gemm_x6_nt_case(lib, M, N, K, device="cpu", runs=1):
    """A B^T with both operands split on the fly (gemm_x6_nt_kernel<mode>, LightGlue's similarity) in the active split mode."""
    A, B, ref, scale = _gemm_nt_inputs(M, N, K)
    Ad, Bd = A.to(device).contiguous(), B.to(device).contiguous()
    bufs = []
    for _ in range(runs):
        C, ldc = _matrix_out(M, N, device)
        assert lib.dim_op_gemm_x6_nt_f32(p(Ad), K, p(Bd), K, p(C), ldc, M, N, K, None) == 0, lib.dim_last_error()
        _sync(device)
        bufs.append(C)
    return _matrix_result(bufs, M, N, ref, scale)


# ---------------------------------------------------------------------------------------------------------------- 3 x 3 convolutions
@functools.lru_cache(maxsize=8)
def _conv3x3_inputs(cin, cout, H, W, pool, batch):
    g = torch.Generator().manual_seed(cin + H)
    x = torch.randn(batch, cin, H, W, generator=g)
    w = (torch.randn(cout, cin, 3, 3, generator=g) * 0.1).contiguous()
    b = torch.randn(cout, generator=g)
    ref = torch.relu(F.conv2d(x.double(), w.double(), b.double(), padding=1))
    if pool:
        ref = F.max_pool2d(ref, 2, 2)
    mag = F.conv2d(x.abs().double(), w.abs().double(), padding=1).max().item()
    return x.permute(0, 2, 3, 1).contiguous(), w, b, ref.permute(0, 2, 3, 1).contiguous(), mag


def conv3x3_case(lib, cin, cout, H, W, pool, batch=2, split=False, device="cpu", runs=1):
    """relu(conv3x3(x) + b) [-> 2 x 2 max pool] on NHWC: dim_op_conv3x3_nhwc_f32 (conv3x3_mfma_kernel, variant = key 0), or with split=True
    dim_convx6_create + dim_op_conv3x3_x6_nhwc_f32 (conv3x3_x6_kernel in the active split mode; bf16x6 prefetch variant = key 2).
    scale = max of conv(|x|, |w|) (one number: the metric of the split-precision tests)."""
    xin, w, b, ref, mag = _conv3x3_inputs(cin, cout, H, W, pool, batch)
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    xd, bd = xin.to(device), b.to(device)
    handle = ctypes.c_void_p()
    if split:
        assert lib.dim_convx6_create(p(w), cin, cout, ctypes.byref(handle)) == 0, lib.dim_last_error()
    else:
        wk = w.permute(2, 3, 1, 0).contiguous().reshape(9, cin, cout).to(device)
    bufs = []
    try:
        for _ in range(runs):
            out = _dense_out(batch * Ho * Wo * cout, device)
            if split:
                rc = lib.dim_op_conv3x3_x6_nhwc_f32(p(xd), handle, p(bd), p(out), batch, H, W, cin, cout, pool, 1, None)
            else:
                rc = lib.dim_op_conv3x3_nhwc_f32(p(xd), p(wk), p(bd), p(out), batch, H, W, cin, cout, pool, 1, None)
            assert rc == 0, lib.dim_last_error()
            _sync(device)
            bufs.append(out)
    finally:
        if split:
            lib.dim_x3_destroy(handle)
    return _dense_result(bufs, (batch, Ho, Wo, cout), ref, torch.tensor(mag, dtype=torch.float64))


@functools.lru_cache(maxsize=2)
def _conv1a_inputs(batch, H, W):
    g = torch.Generator().manual_seed(batch + H + W)
    x = torch.rand(batch, 1, H, W, generator=g)                         # an image in [0, 1]
    w = (torch.randn(64, 1, 3, 3, generator=g) * 0.3).contiguous()
    b = torch.randn(64, generator=g) * 0.1
    ref = torch.relu(F.conv2d(x.double(), w.double(), b.double(), padding=1)).permute(0, 2, 3, 1).contiguous()
    return x[:, 0].contiguous(), w.reshape(64, 9).t().contiguous(), b, ref


def conv1a_case(lib, batch, H, W, device="cpu", runs=1):
    """SuperPoint's conv1a: relu(conv3x3(image) + b), [batch][H][W] -> [batch][H][W][64], weights [9][64] (dim_op_conv1a_f32, conv1a_kernel)."""
    x, wk, b, ref = _conv1a_inputs(batch, H, W)
    xd, wd, bd = x.to(device), wk.to(device), b.to(device)
    bufs = []
    for _ in range(runs):
        out = _dense_out(batch * H * W * 64, device)
        assert lib.dim_op_conv1a_f32(p(xd), p(wd), p(bd), p(out), batch, H, W, None) == 0, lib.dim_last_error()
        _sync(device)
        bufs.append(out)
    return _dense_result(bufs, (batch, H, W, 64), ref, None)


# ---------------------------------------------------------------------------------------------------------------- LightGlue feed-forward
def _ffn_ln_gelu_case(lib, M, K, seed, device="cpu"):
    """gelu(layer_norm(A W + b)) through dim_op_gemm_x6_ln_gelu_f32 -> (device result, fp64 reference)."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, K, generator=g) * 1.5
    W = (torch.randn(K, 512, generator=g) / K ** 0.5).contiguous()
    bias, gamma, beta = torch.randn(512, generator=g) * 0.1, 1.0 + 0.2 * torch.randn(512, generator=g), 0.1 * torch.randn(512, generator=g)
    dev, npad = ctypes.c_void_p(), ctypes.c_int()
    assert lib.dim_x3_create(p(W), K, 512, ctypes.byref(dev), ctypes.byref(npad)) == 0 and npad.value == 512
    Ad, bd, gd, btd = (t.to(device).contiguous() for t in (A, bias, gamma, beta))
    C = torch.full((M, 512), -7.0, device=device)
    try:
        rc = lib.dim_op_gemm_x6_ln_gelu_f32(p(Ad), K, dev, p(bd), p(gd), p(btd), p(C), 512, M, K, None)
        assert rc == 0, lib.dim_last_error()
        if device != "cpu":
            torch.cuda.synchronize()
    finally:
        lib.dim_x3_destroy(dev)
    h = A.double() @ W.double() + bias.double()
    ref = torch.nn.functional.gelu(torch.nn.functional.layer_norm(h, (512,), gamma.double(), beta.double(), 1e-5))
    return C.cpu(), ref


def _ffn_fused_case(lib, M, K, seed, device="cpu"):
    """residual + gelu(layer_norm(A W0 + b0)) W3 + b3 through dim_op_ffn_fused_f32 -> (device result, fp64 reference)."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, K, generator=g) * 1.5
    W0 = (torch.randn(K, 512, generator=g) / K ** 0.5).contiguous()
    W3 = (torch.randn(512, 256, generator=g) / 512 ** 0.5).contiguous()
    b0, gamma, beta = torch.randn(512, generator=g) * 0.1, 1.0 + 0.2 * torch.randn(512, generator=g), 0.1 * torch.randn(512, generator=g)
    b3, R = torch.randn(256, generator=g) * 0.1, torch.randn(M, 256, generator=g)
    h0, h3, npad = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int()
    assert lib.dim_x3_create(p(W0), K, 512, ctypes.byref(h0), ctypes.byref(npad)) == 0 and npad.value == 512
    assert lib.dim_x3_create_kperm(p(W3), 512, 256, ctypes.byref(h3), ctypes.byref(npad)) == 0 and npad.value == 256
    Ad, b0d, gd, btd, b3d, Rd = (t.to(device).contiguous() for t in (A, b0, gamma, beta, b3, R))
    C = torch.full((M, 256), -7.0, device=device)
    try:
        rc = lib.dim_op_ffn_fused_f32(p(Ad), K, h0, p(b0d), p(gd), p(btd), h3, p(b3d), p(Rd), 256, p(C), 256, M, K, None)
        assert rc == 0, lib.dim_last_error()
        if device != "cpu":
            torch.cuda.synchronize()
    finally:
        lib.dim_x3_destroy(h0); lib.dim_x3_destroy(h3)
    h = torch.nn.functional.gelu(torch.nn.functional.layer_norm(A.double() @ W0.double() + b0.double(), (512,), gamma.double(), beta.double(), 1e-5))
    return C.cpu(), R.double() + h @ W3.double() + b3.double()
