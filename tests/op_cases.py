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


# ---------------------------------------------------------------------------------------------------------------- NHWC implicit-GEMM convolution
# name: (kernel, cin, cin2, N, stride, (in_h, in_w), (H, W), pool, relu, form); a workgroup covers 16 x 8 output pixels, so every case has a partial tile
# and A, B, C, E full ones as well; N = 16 / 8, 48, 96, 128 -> 1, 2, 3, 4 column tiles
NHWC_CONV_CASES = {
    "A": (3, 16, 0, 16, 1, (9, 17), (9, 17), 0, 1, ""),
    "B": (3, 3, 0, 8, 1, (13, 19), (32, 32), 2, 1, "img3"),        # the image is smaller than the frame: what lies past it is zero padding
    "C": (3, 32, 16, 48, 1, (12, 20), (12, 20), 4, 1, ""),
    "D": (1, 48, 0, 96, 1, (5, 7), (5, 7), 0, 0, ""),
    "E": (3, 32, 0, 128, 2, (11, 23), (6, 12), 0, 1, ""),
    "F": (1, 64, 0, 64, 1, (24, 40), (3, 5), 0, 1, "unfold8"),     # the plane read as its 8 x 8 unfolding
}


def _nhwc_pad16(t):
    """[b][c][h][w] -> NHWC with the channel stride padded up to a multiple of 16 (zeros)."""
    t = t.permute(0, 2, 3, 1)
    return F.pad(t, (0, -t.shape[3] % 16)).contiguous()


@functools.lru_cache(maxsize=None)
def _nhwc_conv_inputs(name, batch):
    k, cin, cin2, N, stride, (ih, iw), (H, W), pool, relu, form = NHWC_CONV_CASES[name]
    g = torch.Generator().manual_seed(ord(name))
    w = (torch.randn(N, cin, k, k, generator=g) * 0.1).contiguous()
    b = torch.randn(N, generator=g)
    if form == "unfold8":
        plane = torch.randn(batch, 1, ih, iw, generator=g)
        x = F.unfold(plane, 8, stride=8).view(batch, 64, H, W)
        xin = plane[:, 0].contiguous()
    else:
        x = torch.randn(batch, cin, ih, iw, generator=g)
        xin = x.permute(0, 2, 3, 1).contiguous() if form == "img3" else _nhwc_pad16(x)
        if form == "img3":
            x = F.pad(x, (0, W - iw, 0, H - ih))
    pre = F.conv2d(x.double(), w.double(), b.double(), stride=stride, padding=k // 2)
    mag = F.conv2d(x.abs().double(), w.abs().double(), stride=stride, padding=k // 2)
    w2 = x2in = None
    if cin2:
        x2 = torch.randn(batch, cin2, H, W, generator=g)
        w2 = (torch.randn(N, cin2, 1, 1, generator=g) * 0.1).contiguous()
        pre = pre + F.conv2d(x2.double(), w2.double())
        mag = mag + F.conv2d(x2.abs().double(), w2.abs().double())
        x2in = _nhwc_pad16(x2)
    assert pre.shape == (batch, N, H, W), pre.shape
    ref = torch.relu(pre) if relu else pre
    ref_pool = _nhwc_pad16(F.max_pool2d(ref, pool)) if pool else None
    return xin, x2in, w, w2, b, _nhwc_pad16(ref), ref_pool, torch.tensor(mag.max().item(), dtype=torch.float64)


def nhwc_conv_case(lib, name, batch=2, device="cpu", runs=1):
    """One case of NHWC_CONV_CASES through dim_nhwc_conv_create + dim_op_nhwc_conv_f32 (nhwc_conv_kernel<MODE, NT> in the arithmetic form that is active at
    the call) vs fp64 conv2d (+ the 1x1 product of in2) / relu / max_pool2d on the zero-padded frame (img3) or on F.unfold's channels (unfold8).
    -> (out, pooled or None, N): two OpResults whose references carry the padding channels [N, pad16(N)) as zeros; scale = max of conv(|x|, |w|)."""
    k, cin, cin2, N, stride, (ih, iw), (H, W), pool, relu, form = NHWC_CONV_CASES[name]
    xin, x2in, w, w2, b, ref, ref_pool, mag = _nhwc_conv_inputs(name, batch)
    out_c = ref.shape[3]
    xd = xin.to(device)
    x2d = x2in.to(device) if x2in is not None else None
    handle = ctypes.c_void_p()
    assert lib.dim_nhwc_conv_create(p(w), N, cin, k, stride, p(w2), cin2, p(b), relu, ctypes.byref(handle)) == 0, lib.dim_last_error()
    outs, pools = [], []
    try:
        for _ in range(runs):
            out = _dense_out(batch * H * W * out_c, device)
            pooled = _dense_out(batch * (H // pool) * (W // pool) * out_c, device) if pool else None
            rc = lib.dim_op_nhwc_conv_f32(handle, p(xd), ih, iw, int(form == "img3"), int(form == "unfold8"), p(x2d), p(out), p(pooled), pool, batch, H, W, None)
            assert rc == 0, lib.dim_last_error()
            _sync(device)
            outs.append(out)
            pools.append(pooled)
    finally:
        lib.dim_nhwc_conv_destroy(handle)
    r_pool = _dense_result(pools, (batch, H // pool, W // pool, out_c), ref_pool, mag) if pool else None
    return _dense_result(outs, (batch, H, W, out_c), ref, mag), r_pool, N


def nhwc_conv_figure(r, x3):
    """(figure, bound) of one result: fp16x3 rel_err < 4e-7, fp32 max abs error < 1e-4 — the bounds of the 3 x 3 convolution tests on the same input
    distribution (x ~ randn, w ~ 0.1 randn, b ~ randn); every K here is below their 1152."""
    return (r.rel_err, 4e-7) if x3 else (r.abs_err.max().item(), 1e-4)


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


# ---------------------------------------------------------------------------------------------------------------- keypoint selection
# dim_op_select_topk_f32 = launch_select_ex -> launch_topk [-> launch_topk_zero_fill] (csrc/sp_post.hip), the chain between the NMS and the
# descriptor head of both extractors.  The reference is exact (no arithmetic, only comparisons), so every comparison below is bit for bit.
# Domain: scores >= 0 and thresholds >= 0 (the sort key is the score's bit pattern; include/dim_hip.h).
I32_SENTINEL = -7
_vp, _ci = ctypes.c_void_p, ctypes.c_int


def _bind_selection(lib):
    """Explicit argument types: a bare Python float would otherwise be passed as an int."""
    lib.dim_op_select_topk_workspace_bytes.argtypes = [_ci, _ci, _ci, _ci]
    lib.dim_op_select_topk_workspace_bytes.restype = ctypes.c_size_t
    lib.dim_op_select_topk_f32.argtypes = [_vp, _ci, _ci, _ci, ctypes.c_float, _vp, _ci, _ci, _ci, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _vp]
    lib.dim_op_select_topk_f32.restype = _ci
    lib.dim_op_sample_descriptors_f32.argtypes = [_vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _vp]
    lib.dim_op_sample_descriptors_f32.restype = _ci


def score_map(H, W, seed, levels=None, density=None, value=None):
    """One H x W map: rand * 0.9 + 0.05, optionally quantised to `levels` values (round(m * L) / L + 0.01: ties everywhere), thinned to `density`
    by zeroing, or constant `value`."""
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(H, W, generator=g) * 0.9 + 0.05
    if value is not None:
        m = torch.full((H, W), float(value))
    if levels is not None:
        m = (m * levels).round() / levels + 0.01
    if density is not None:
        m = torch.where(torch.rand(H, W, generator=g) < density, m, torch.zeros(()))
    return m


@functools.lru_cache(maxsize=None)
def select_maps(name):
    """The crafted maps of the selection cases, [batch][H][W] (cached: read only)."""
    if name == "equal":          # all scores equal: the radix select has to walk the four index bytes
        return score_map(72, 100, 0, value=0.5)[None]
    if name == "ties":           # six score levels: the k-th key falls inside a tie group
        return score_map(100, 132, 1, levels=6)[None]
    if name == "n_near_k":
        return score_map(96, 128, 2, density=0.35)[None]
    if name == "handover":       # n ~ 4800 around k = 4096
        return score_map(80, 100, 3, density=0.6)[None]
    if name == "mixed":          # per-image branches inside one launch: empty, under k, over k, ties, a single pixel
        one = torch.zeros(90, 124)
        one[40, 77] = 0.625
        return torch.stack([torch.zeros(90, 124), score_map(90, 124, 4, density=0.05), score_map(90, 124, 5, density=0.9),
                            score_map(90, 124, 6, levels=4), one])
    if name in ("mixed_sparse", "mixed_dense", "mixed_ties"):
        return select_maps("mixed")[{"mixed_sparse": 1, "mixed_dense": 2, "mixed_ties": 3}[name]][None].contiguous()
    if name == "keep_all":
        return torch.stack([score_map(50, 70, 7, density=0.5), score_map(50, 70, 8, density=0.5)])
    if name == "wide1300":       # W % 4 == 0: the float4 row loop's second 1024-column step
        return score_map(6, 1300, 9)[None]
    if name == "wide1301":       # its scalar twin
        return score_map(6, 1301, 10)[None]
    if name == "w260":           # just past one 256-column group
        return torch.stack([score_map(37, 260, 11), score_map(37, 260, 12)])
    if name == "tall":           # 1030 rows: scan_rows_kernel sums two rows per thread
        return torch.stack([score_map(1030, 8, 13, density=0.5), score_map(1030, 8, 14, density=0.5)])
    if name == "thr_dev":
        return torch.stack([score_map(60, 84, 15 + i) for i in range(3)])
    if name == "small":
        return score_map(20, 30, 18)[None]
    if name == "big_d07":
        return score_map(200, 200, 19, density=0.7)[None]
    if name == "big_full":
        return score_map(200, 200, 20)[None]
    if name == "big_ties":
        return score_map(200, 200, 21, levels=3)[None]
    if name == "occupancy128":   # 128 images: every selection kernel has at least 128 workgroups in flight
        return torch.stack([score_map(64, 96, 100 + i, levels=50) for i in range(128)])
    if name == "occupancy16":
        return torch.stack([score_map(100, 132, 300 + i, levels=6) for i in range(16)])
    raise KeyError(name)


def select_count(name, thr, border):
    """Number of candidates of a one-image map (for the cases whose k is derived from it)."""
    return int(select_topk_reference(select_maps(name), [thr], border, -1, 1 << 30, 0, 0)[3][0])


def select_topk_reference(maps, thr, border, k, capacity, sort_always, zero_fill):
    """The rule of include/dim_hip.h, per image -> (pixel indices, scores, kept, n) lists.  thr: one float per image."""
    B, H, W = maps.shape
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    inside = ((ys >= border) & (ys < H - border) & (xs >= border) & (xs < W - border)).reshape(-1)
    idxs, scs, kepts, ns = [], [], [], []
    for b in range(B):
        v = maps[b].reshape(-1)
        mask = (v > torch.tensor(thr[b], dtype=torch.float32)) & inside
        cand = mask.nonzero()[:, 0]
        n = int(cand.numel())
        if k < 0 or (n <= k and not sort_always):
            keep = cand[:min(n, capacity)]
        else:   # score descending, index ascending among equal scores: a stable sort of the row-major list
            keep = cand[torch.sort(v[cand], descending=True, stable=True)[1]][:min(n, k)]
        sc = v[keep]
        kept = int(keep.numel())
        if zero_fill and kept < k:
            fill = (~mask).nonzero()[:k - kept, 0]
            keep, sc = torch.cat([keep, fill]), torch.cat([sc, torch.zeros(fill.numel())])
            kept = int(keep.numel())
        idxs.append(keep); scs.append(sc); kepts.append(kept); ns.append(n)
    return idxs, scs, kepts, ns


class SelectBuffers:
    """Workspace and the four output buffers (each followed by a guard band) of dim_op_select_topk_f32.  A fresh workspace is filled with 0xff
    bytes: a key table that is read before it is written then holds keys above every real one."""

    def __init__(self, lib, batch, H, W, k, capacity, device):
        _bind_selection(lib)
        self.batch, self.capacity, self.limits = batch, capacity, (batch, H, W, k)
        self.ws = torch.full((int(lib.dim_op_select_topk_workspace_bytes(batch, H, W, k)) + 16,), 0xff, dtype=torch.uint8, device=device)
        self.kp = torch.empty(batch * capacity * 2 + GUARD_ELEMS, device=device)
        self.sc = torch.empty(batch * capacity + GUARD_ELEMS, device=device)
        self.n = torch.empty(batch + GUARD_ELEMS, dtype=torch.int32, device=device)
        self.nc = torch.empty(batch + GUARD_ELEMS, dtype=torch.int32, device=device)
        self.refill()

    def refill(self):
        self.kp.fill_(SENTINEL); self.sc.fill_(SENTINEL); self.n.fill_(I32_SENTINEL); self.nc.fill_(I32_SENTINEL)

    def cpu(self):
        """Copies (also on the CPU: the buffers may be re-filled and used again)."""
        return tuple(t.to("cpu", copy=True) for t in (self.kp, self.sc, self.n, self.nc))


class SelectResult(NamedTuple):
    raws: tuple          # per run: (kpts, scores, n_out, n_candidates) full buffers, guard bands included (CPU)
    ref: tuple           # select_topk_reference's lists
    shape: tuple         # (batch, H, W, capacity)

    @property
    def repeatable(self):
        return all(all(torch.equal(a, b) for a, b in zip(self.raws[0], r)) for r in self.raws[1:])

    def check(self):
        """Everything the selection promises, exactly: counts, coordinates, score bits, untouched rows past n_out, untouched guard bands, and the
        same bits from every run."""
        B, H, W, cap = self.shape
        idxs, scs, kepts, ns = self.ref
        for kp, sc, n_out, n_cand in self.raws:
            assert n_cand[:B].tolist() == ns, ("n_candidates", n_cand[:B].tolist(), ns)
            assert n_out[:B].tolist() == kepts, ("n_out", n_out[:B].tolist(), kepts)
            assert bool((n_out[B:] == I32_SENTINEL).all()) and bool((n_cand[B:] == I32_SENTINEL).all()), "guard band of the counts was written"
            assert bool((kp[B * cap * 2:] == SENTINEL).all()) and bool((sc[B * cap:] == SENTINEL).all()), "guard band of the tables was written"
            kp, sc = kp[:B * cap * 2].view(B, cap, 2), sc[:B * cap].view(B, cap)
            for b in range(B):
                m = kepts[b]
                want = torch.stack([(idxs[b] % W).float(), (idxs[b] // W).float()], dim=1)
                assert torch.equal(kp[b, :m], want), ("keypoints of image", b, int((kp[b, :m] != want).any(dim=1).nonzero()[0]))
                assert torch.equal(sc[b, :m].view(torch.int32), scs[b].view(torch.int32)), ("scores of image", b)
                assert bool((kp[b, m:] == SENTINEL).all()) and bool((sc[b, m:] == SENTINEL).all()), ("rows past n_out were written, image", b)
        assert self.repeatable, "two runs on the same inputs differ"


def select_topk_case(lib, maps, thr, border, k, capacity, sort_always, zero_fill, thr_dev=None, device="cpu", runs=1, bufs=None):
    """dim_op_select_topk_f32 on `maps` [batch][H][W] vs select_topk_reference.  thr_dev: a list with one threshold per image (passed on the
    device; replaces thr).  bufs: a SelectBuffers to REUSE (re-filled with SENTINEL, workspace left as the previous call left it); by default
    every run gets fresh buffers and a fresh, poisoned workspace."""
    _bind_selection(lib)
    B, H, W = maps.shape
    md = maps.to(device).contiguous()
    td = torch.tensor(thr_dev, dtype=torch.float32).to(device) if thr_dev is not None else None
    raws = []
    for _ in range(runs):
        if bufs is None:
            bf = SelectBuffers(lib, B, H, W, k, capacity, device)
        else:
            bf = bufs
            assert bf.batch == B and bf.capacity == capacity
            assert int(lib.dim_op_select_topk_workspace_bytes(B, H, W, k)) <= bf.ws.numel()
            bf.refill()
        rc = lib.dim_op_select_topk_f32(p(md), B, H, W, float(thr), p(td), border, k, capacity, sort_always, zero_fill, p(bf.ws), p(bf.kp), p(bf.sc),
                                        p(bf.n), p(bf.nc), None)
        assert rc == 0, lib.dim_last_error()
        _sync(device)
        raws.append(bf.cpu())
    per_image = [float(t) for t in thr_dev] if thr_dev is not None else [float(thr)] * B
    return SelectResult(tuple(raws), select_topk_reference(maps, per_image, border, k, capacity, sort_always, zero_fill), (B, H, W, capacity))


def _select_cases():
    """(id, map name, thr, border, k, capacity, sort_always, zero_fill, thr_dev); k may be a function of the candidate count n."""
    c = []
    for k in (300, 4096, 4097, 5000):
        c.append((f"equal-k{k}", "equal", 0.0, 0, k, k, 0, 0, None))
    for k in (1000, 4096, 4097, 8192, 8193):
        c.append((f"ties-k{k}", "ties", 0.0, 2, k, k, 0, 0, None))
    n = select_count("n_near_k", 0.005, 4)
    assert 3000 < n < 4096, n
    for dk in (-1, 0, 1):
        for sa, zf in ((0, 0), (1, 0), (1, 1)):
            c.append((f"n_near_k-n{dk:+d}-s{sa}z{zf}", "n_near_k", 0.005, 4, n + dk, n + 1, sa, zf, None))
    for k in (4095, 4096, 4097):
        for sa, zf in ((0, 0), (1, 1)):
            c.append((f"handover-k{k}-s{sa}z{zf}", "handover", 0.0, 0, k, 8000, sa, zf, None))
    for k in (500, 4096, 6000):
        for sa, zf in ((0, 0), (1, 0), (1, 1)):
            c.append((f"mixed-k{k}-s{sa}z{zf}", "mixed", 0.0, 3, k, k, sa, zf, None))
    for cap in (1000, 4096):
        c.append((f"keep_all-cap{cap}", "keep_all", 0.0, 0, -1, cap, 0, 0, None))
    c.append(("wide1300", "wide1300", 0.0, 1, 200, 200, 0, 0, None))
    c.append(("wide1301", "wide1301", 0.0, 1, 200, 200, 0, 0, None))
    c.append(("w260", "w260", 0.0, 5, 300, 300, 1, 1, None))
    c.append(("tall", "tall", 0.0, 0, 700, 700, 0, 0, None))
    c.append(("thr_dev", "thr_dev", 0.0, 2, 400, 400, 0, 0, (0.2, 0.9, 2.0)))
    c.append(("border_removes_all", "small", 0.0, 10, 50, 50, 1, 1, None))
    c.append(("big_d07-k20000", "big_d07", 0.0, 0, 20000, 20000, 1, 1, None))
    c.append(("big_full-k32768", "big_full", 0.0, 0, 32768, 32768, 0, 0, None))
    c.append(("big_ties-k32768", "big_ties", 0.0, 0, 32768, 32768, 1, 1, None))
    return c


SELECT_CASES = _select_cases()
# many workgroups resident at once (hardware only)
SELECT_OCCUPANCY_CASES = [(f"{m}-k{k}-s{sa}z{zf}", m, 0.0, 2, k, k, sa, zf, None)
                          for m, k in (("occupancy128", 1000), ("occupancy16", 5000)) for sa, zf in ((0, 0), (1, 1))]


def run_select_case(lib, case, device="cpu", runs=1):
    _, name, thr, border, k, cap, sa, zf, thr_dev = case
    return select_topk_case(lib, select_maps(name), thr, border, k, cap, sa, zf, thr_dev=thr_dev, device=device, runs=runs)


def select_reused_workspace_results(lib, device="cpu", runs=1):
    """One workspace and one set of output buffers through three calls: the dense map at k = 6000 (fills the two-chunk key table), the sparse map
    at k = 6000 with sort_always and zero_fill (few keys: whatever the table held must not come back), the tie map at k = 300 (the one-workgroup
    form after the chunked one)."""
    H, W = select_maps("mixed").shape[1:]
    bufs = SelectBuffers(lib, 1, H, W, 6000, 6000, device)
    calls = (("mixed_dense", 6000, 0, 0), ("mixed_sparse", 6000, 1, 1), ("mixed_ties", 300, 0, 0))
    return [select_topk_case(lib, select_maps(m), 0.0, 3, k, 6000, sa, zf, device=device, runs=runs, bufs=bufs) for m, k, sa, zf in calls]


def select_error_case(lib, device="cpu"):
    """zero_fill with k > H * W: an error return that names the size (torch.topk's 'selected index k out of range'); nothing is launched."""
    _bind_selection(lib)
    bf = SelectBuffers(lib, 1, 4, 5, 50, 64, device)
    md = score_map(4, 5, 0)[None].to(device).contiguous()
    rc = lib.dim_op_select_topk_f32(p(md), 1, 4, 5, 0.0, None, 0, 50, 64, 1, 1, p(bf.ws), p(bf.kp), p(bf.sc), p(bf.n), p(bf.nc), None)
    _sync(device)
    return rc, lib.dim_last_error().decode(), bf.cpu()


# ---------------------------------------------------------------------------------------------------------------- descriptor sampling
class SampleResult(NamedTuple):
    out: torch.Tensor          # [batch][capacity][256] of the first run (CPU)
    ref: torch.Tensor          # fp64 reference, rows past n_kpts[b] = SENTINEL
    live: torch.Tensor         # [batch][capacity] bool: rows below n_kpts[b]
    zero_rows: torch.Tensor    # [batch][capacity] bool: live keypoints whose four cells lie in the all-zero block
    oracle_err: float          # max |oracle fp32 - fp64| over the live rows
    guard_ok: bool
    raws: tuple

    @property
    def repeatable(self):
        return all(torch.equal(self.raws[0], r) for r in self.raws[1:])

    @property
    def err(self):
        return (self.out.double() - self.ref)[self.live].abs().max().item() if bool(self.live.any()) else 0.0


def _sample_coords64(k, h, w, fix_sampling):
    """Input-pixel coordinates (ix, iy) in cell units of the integer keypoints k [N][2], in fp64, by the formulas of
    oracle.superpoint_ref.sample_descriptors and grid_sample's un-normalisation of the branch's align_corners."""
    k = k.double()
    wh = torch.tensor([w, h], dtype=torch.float64)
    if fix_sampling:
        g = (k + 0.5) / (wh * 8) * 2 - 1
        return g, ((g + 1) * wh - 1) / 2, False
    g = (k - 4 + 0.5) / (wh * 8 - 4 - 0.5) * 2 - 1
    return g, (g + 1) / 2 * (wh - 1), True


@functools.lru_cache(maxsize=2)
def _sample_inputs(h, w, batch, capacity, n_kpts, fix_sampling):
    g = torch.Generator().manual_seed(h * 1000 + w + (7 if fix_sampling else 0))
    dense = torch.randn(batch, h, w, 256, generator=g)
    zy, zx = h // 2, w // 2                                   # the all-zero 2 x 2 block of cells
    dense[:, zy:zy + 2, zx:zx + 2] = 0.0
    Wp, Hp = 8 * w, 8 * h
    if fix_sampling:   # ix = (kx + 0.5) / 8 - 0.5 = zx + 0.5
        cx, cy = 8 * (zx + 1), 8 * (zy + 1)
    else:              # ix = (kx - 3.5) / (8 w - 4.5) * (w - 1) = zx + 0.5
        cx, cy = round(3.5 + (zx + 0.5) * (Wp - 4.5) / (w - 1)), round(3.5 + (zy + 0.5) * (Hp - 4.5) / (h - 1))
    fixed = torch.tensor([(0, 0), (Wp - 1, 0), (0, Hp - 1), (Wp - 1, Hp - 1), (Wp // 2, 0), (Wp // 2, Hp - 1), (0, Hp // 2), (Wp - 1, Hp // 2),
                          (cx, cy), (cx + 1, cy - 1)], dtype=torch.float32)
    kp = torch.stack([torch.randint(0, Wp, (batch, capacity), generator=g), torch.randint(0, Hp, (batch, capacity), generator=g)], dim=2).float()
    nf = min(len(fixed), capacity)
    kp[:, :nf] = fixed[:nf]
    n = torch.tensor(n_kpts, dtype=torch.int32)
    live = torch.arange(capacity)[None, :] < n[:, None]
    # fp64 reference and the fp32 oracle on the same inputs
    dn64 = dense.double() / dense.double().norm(dim=3, keepdim=True).clamp_min(1e-12)
    dn32 = F.normalize(dense.permute(0, 3, 1, 2), p=2, dim=1)
    ref = torch.full((batch, capacity, 256), SENTINEL, dtype=torch.float64)
    zero_rows = torch.zeros(batch, capacity, dtype=torch.bool)
    oracle_err = 0.0
    for b in range(batch):
        m = int(n[b])
        if m == 0:
            continue
        grid, ixy, ac = _sample_coords64(kp[b, :m], h, w, fix_sampling)
        s = F.grid_sample(dn64[b].permute(2, 0, 1)[None], grid.view(1, 1, -1, 2), mode="bilinear", padding_mode="zeros", align_corners=ac)
        r = F.normalize(s.reshape(256, m), p=2, dim=0, eps=1e-12).t()
        ref[b, :m] = r
        f = ixy.floor()
        zero_rows[b, :m] = (f[:, 0] == zx) & (f[:, 1] == zy)
        o32 = superpoint_ref.sample_descriptors(kp[b, :m], dn32[b][None], fix_sampling=bool(fix_sampling)).t()
        oracle_err = max(oracle_err, (o32.double() - r).abs().max().item())
    if min(n_kpts) >= nf >= 10:   # the two zero-block keypoints sit well inside the block (at least 0.05 cells from its cells' centres)
        assert bool(zero_rows[:, 8:10].all())
        assert not bool(ref[:, 8:10].any())
    return dense, kp, n, ref, live, zero_rows, oracle_err


def sample_descriptors_case(lib, h, w, batch, capacity, n_kpts, fix_sampling, device="cpu", runs=1):
    """dim_op_sample_descriptors_f32 (sample_desc_kernel: one wave per keypoint) on an h x w x 256 randn cell map with an all-zero 2 x 2 block, at
    the image's corners, edge midpoints, the zero block's centre and seeded random integer positions, vs fp64 (cells L2-normalised in fp64, the
    coordinates of oracle.superpoint_ref.sample_descriptors in fp64, F.grid_sample in fp64, L2-normalised).  oracle_err: the error of the oracle
    itself in fp32 on the same inputs — the yardstick of the kernel's error."""
    _bind_selection(lib)
    dense, kp, n, ref, live, zero_rows, oracle_err = _sample_inputs(h, w, batch, capacity, tuple(n_kpts), int(bool(fix_sampling)))
    dd, kd, nd = dense.to(device).contiguous(), kp.to(device).contiguous(), n.to(device)
    bufs = []
    for _ in range(runs):
        out = _dense_out(batch * capacity * 256, device)
        assert lib.dim_op_sample_descriptors_f32(p(dd), p(kd), p(nd), p(out), batch, h, w, capacity, int(bool(fix_sampling)), None) == 0, lib.dim_last_error()
        _sync(device)
        bufs.append(out)
    raws = tuple(b.cpu() for b in bufs)
    numel = batch * capacity * 256
    ok = all(bool((r[numel:] == SENTINEL).all()) for r in raws)
    return SampleResult(raws[0][:numel].view(batch, capacity, 256), ref, live, zero_rows, oracle_err, ok, raws)


def check_sample(r):
    """Rows past n_kpts untouched, guard band untouched, zero-block keypoints exactly zero, every run the same bits, and the error within 4 x the
    fp32 oracle's own (a different order of the same dozen roundings, not a different algorithm).  Returns (kernel error, oracle error)."""
    print(f"sample_descriptors: kernel err {r.err:.4g} oracle fp32 err {r.oracle_err:.4g}")
    assert r.guard_ok, "the guard band behind the descriptors was written"
    assert bool((r.out[~r.live] == SENTINEL).all()), "rows at or past n_kpts were written"
    assert r.repeatable, "two runs on the same inputs differ"
    assert bool((r.out[r.zero_rows] == 0).all()), "a keypoint inside the all-zero block did not give an exactly zero descriptor"
    assert r.err <= 4 * r.oracle_err, (r.err, r.oracle_err)
    return r.err, r.oracle_err


SAMPLE_CASES = [(5, 7, 3, 64, (0, 1, 64)), (12, 20, 2, 300, (300, 37))]       # (h, w, batch, capacity, n_kpts)
SAMPLE_OCCUPANCY_CASE = (128, 128, 2, 2048, (2048, 2047))                       # cdiv(2048, 4) * 2 = 1024 workgroups (hardware only)


# ---------------------------------------------------------------------------------------------------------------- attention (LightGlue, LighterGlue, SuperGlue)
# dim_op_lg_attention_f32 / dim_op_lg_qkv_attention_f32 (include/dim_hip.h) = the matchers' launchers on caller-supplied projections:
#   width 256  launch_lg_attention -> attn_kernel (fp32, behind launch_lg_rotary for kind 0) | launch_lg_attention_x6 -> kv_prep_kernel<MODE>,
#              attn_x6_kernel<MODE> [, attn_combine_kernel<2 | 4>]
#   width 96   launch_lgl_attention -> kv_prep96_kernel<MODE>, attn_d96_kernel<MODE> [, attn_combine96_kernel]
# against a plain fp64 evaluation.  Figure: max |out - ref| / max|v|, max|v| per (key item, head), over the live rows.  Yardstick: the same figure of a
# plain fp32 torch evaluation of the same fp32 inputs (fp32 rotary, matmul, softmax, matmul), the largest of ATTN_PERMS evaluations with permuted key
# order.  Bound: ATTN_FACTOR x yardstick, the factor of the project's other fp32-accuracy claims (goldens, lighterglue attention_undamped, Sinkhorn).
# An item is (n, seed): its rows depend on nothing else, so the same item can sit in calls of different sizes.
ATTN_FACTOR, ATTN_PERMS = 2.0, 4
LOG2E = 1.4426950408889634


def _bind_attention(lib):
    lib.dim_op_lg_attention_workspace_bytes.argtypes = [_ci, _ci, _ci, _ci]
    lib.dim_op_lg_attention_workspace_bytes.restype = ctypes.c_size_t
    lib.dim_op_lg_attention_f32.argtypes = [_ci, _ci, _vp, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _vp, _vp]
    lib.dim_op_lg_attention_f32.restype = _ci
    lib.dim_op_lg_qkv_attention_f32.argtypes = [_ci, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _vp, _vp]
    lib.dim_op_lg_qkv_attention_f32.restype = _ci


def attn_heads(width):
    return (4, 64) if width == 256 else (1, 96)


@functools.lru_cache(maxsize=None)
def _attn_item(width, n, family, seed):
    """One item: q, k [n][width] ~ gain randn, v ~ randn, enc [n][width / heads] = cos | sin of angles uniform in [0, 2 pi).  flat: gain 1 (logits within
    about +-5).  ramp: gain 1.5 and k times linspace(0.2, 2, n) along the keys: the running maximum rises tile after tile."""
    g = torch.Generator().manual_seed(seed)
    gain = 1.5 if family == "ramp" else 1.0
    q, k, v = gain * torch.randn(n, width, generator=g), gain * torch.randn(n, width, generator=g), torch.randn(n, width, generator=g)
    if family == "ramp":
        k = k * torch.linspace(0.2, 2.0, n)[:, None]
    ang = torch.rand(n, attn_heads(width)[1] // 2, generator=g) * (2 * torch.pi)
    return q, k, v, torch.cat([torch.cos(ang), torch.sin(ang)], dim=1)


def _attn_rotate(x, enc):
    """x [heads][n][hd], enc [n][hd] = cos[hd / 2] | sin[hd / 2]: the pairs (x[2f], x[2f + 1]) rotated by (cos[f], sin[f]), in x's precision."""
    hf = enc.shape[1] // 2
    c, s = enc[None, :, :hf].to(x.dtype), enc[None, :, hf:].to(x.dtype)
    x0, x1 = x[..., 0::2], x[..., 1::2]
    return torch.stack([x0 * c - x1 * s, x1 * c + x0 * s], dim=-1).flatten(-2)


def _attn_split_rows(width, kind, rows):
    """One item's qkv rows -> (q, k, v), each [n][width]."""
    if kind == 1:
        return rows[:, :width], rows[:, :width], rows[:, width:2 * width]
    return rows[:, :width], rows[:, width:2 * width], rows[:, 2 * width:]


def _attn_eval(width, kind, qkv, enc, n, dtype, perm_seed=None):
    """softmax(q k^T scale) v per item and head in `dtype` over the first n[key item] keys (kind 1 / 3: the keys and values of item ^ 1), rotary on q and
    k for kind 0; an empty key set gives zeros.  qkv [items][nmax][3 width] -> ([items][nmax][width] (rows past n: 0), per-item tile events).
    perm_seed: the keys of every item are visited in a seeded random order.  events[i] = (a key tile of 32 whose maximum exceeds the running one by
    more than 8 in log2, one that exceeds it by 0 .. 8), by the rule of the kernels: the running maximum only moves in the first case."""
    heads, hd = attn_heads(width)
    scale = 0.125 if width == 256 else 96.0 ** -0.5
    I, nmax = qkv.shape[:2]
    out = torch.zeros(I, nmax, width, dtype=dtype)
    events = []
    for i in range(I):
        j = i ^ 1 if kind in (1, 3) else i
        nq, nk = int(n[i]), int(n[j])
        events.append((False, False))
        if nq == 0 or nk == 0:
            continue
        q = _attn_split_rows(width, kind, qkv[i, :nq])[0].to(dtype).view(nq, heads, hd).transpose(0, 1)
        _, k, v = _attn_split_rows(width, kind, qkv[j, :nk])
        k, v = k.to(dtype).view(nk, heads, hd).transpose(0, 1), v.to(dtype).view(nk, heads, hd).transpose(0, 1)
        if kind == 0:
            q, k = _attn_rotate(q, enc[i, :nq]), _attn_rotate(k, enc[j, :nk])
        if perm_seed is not None:
            perm = torch.randperm(nk, generator=torch.Generator().manual_seed(perm_seed * 1000 + i))
            k, v = k[:, perm], v[:, perm]
        s = (q @ k.transpose(1, 2)) * scale
        out[i, :nq] = (torch.softmax(s, dim=-1) @ v).transpose(0, 1).reshape(nq, width)
        if perm_seed is None and nk > 32:
            tiles = -(-nk // 32)
            tm = F.pad(s * LOG2E, (0, tiles * 32 - nk), value=float("-inf")).view(heads, nq, tiles, 32).amax(dim=-1)
            m, jump, defer = tm[..., 0], False, False
            for t in range(1, tiles):
                d = tm[..., t] - m
                jump, defer = jump or bool((d > 8).any()), defer or bool(((d > 0) & (d <= 8)).any())
                m = torch.where(d > 8, tm[..., t], m)
            events[-1] = (jump, defer)
    return out, events


def _attn_vmax(width, kind, qkv, n):
    """[items][heads]: max|v| over the live keys of the KEY item of every item (1 where there is none: such rows are exact zeros)."""
    heads, hd = attn_heads(width)
    I = qkv.shape[0]
    vm = torch.ones(I, heads, dtype=torch.float64)
    for i in range(I):
        j = i ^ 1 if kind in (1, 3) else i
        if int(n[j]) > 0:
            vm[i] = _attn_split_rows(width, kind, qkv[j, :int(n[j])])[2].double().abs().view(-1, heads, hd).amax(dim=(0, 2))
    return vm


def _attn_item_figures(width, out, ref, vmax, n):
    """[items]: max over the item's live rows of |out - ref| / max|v| (0 for an item without rows; NaN if the output holds one)."""
    heads, hd = attn_heads(width)
    I, nmax = ref.shape[:2]
    err = (out.double() - ref).abs().view(I, nmax, heads, hd) / vmax[:, None, :, None]
    return torch.stack([err[i, :int(n[i])].max() if int(n[i]) > 0 else torch.zeros((), dtype=torch.float64) for i in range(I)])


def _attn_yardsticks(width, kind, qkv, enc, n, ref, vmax):
    y = torch.zeros(qkv.shape[0], dtype=torch.float64)
    for s in range(ATTN_PERMS):
        o32, _ = _attn_eval(width, kind, qkv, enc, n, torch.float32, perm_seed=s if s else None)
        y = torch.maximum(y, _attn_item_figures(width, o32, ref, vmax, n))
    return y


GUARD_ROW, GUARD_VALUE = 5, 3000.0


@functools.lru_cache(maxsize=8)
def _attn_inputs(width, kind, items, nmax, family):
    """items: ((n, seed), ...).  -> qkv [items][nmax][3 width] in the layout of `kind` (NaN in every row at or past n and in the unused third block of
    kind 1: nothing may read them), enc, n (int32), the fp64 reference, max|v| and the fp32 yardstick per item.
    family "guard" (fp16x3 range guard): flat, with key row GUARD_ROW of item 0 holding the pair (3000, 3000) in dims 0, 1 of head 0 under a rotation
    by 45 degrees -> (0, 4243), above 4094 where every unrotated value is below it; item 0's q is 1e-3 of the others' in those two dims, so that the logits
    stay in the range of `flat`.  In the layout of kind 1 q and k are one block: the pair stands there unrotated."""
    heads, hd = attn_heads(width)
    I = len(items)
    qkv = torch.full((I, nmax, 3 * width), float("nan"))
    enc = torch.full((I, nmax, hd), float("nan"))
    for i, (ni, seed) in enumerate(items):
        q, k, v, e = _attn_item(width, ni, "flat" if family == "guard" else family, seed)
        if family == "guard" and i == 0:
            q, k, e = q.clone(), k.clone(), e.clone()
            q[:, 0:2] *= 1e-3
            k[GUARD_ROW, 0:2] = GUARD_VALUE
            e[GUARD_ROW, 0] = e[GUARD_ROW, hd // 2] = 0.5 ** 0.5
        if kind == 1:   # one block serves as q and as k: the one that carries the ramp
            q = k
        qkv[i, :ni] = torch.cat([q, v, torch.full_like(v, float("nan"))] if kind == 1 else [q, k, v], dim=1)
        enc[i, :ni] = e
    n = torch.tensor([it[0] for it in items], dtype=torch.int32)
    ref, events = _attn_eval(width, kind, qkv, enc, n, torch.float64)
    if family == "ramp":
        assert any(j for j, _ in events) and any(d for _, d in events), ("ramp: some key tile must force a rescale and some tile must be deferred", events)
    vmax = _attn_vmax(width, kind, qkv, n)
    return qkv, enc, n, ref, vmax, _attn_yardsticks(width, kind, qkv, enc, n, ref, vmax)


class AttnResult(NamedTuple):
    out: torch.Tensor          # [items][nmax][width] of the first run (CPU)
    ref: torch.Tensor          # fp64
    live: torch.Tensor         # [items][nmax] bool: rows below n[item] of pairs with done == 0
    n: torch.Tensor
    figure: float              # max over the live rows of |out - ref| / max|v|
    yardstick: float           # the fp32 evaluation's figure over the same items
    untouched: bool            # rows at or past n, rows of stopped pairs and the guard band are still SENTINEL in every run
    raws: tuple

    @property
    def repeatable(self):
        return all(torch.equal(self.raws[0], r) for r in self.raws[1:])


def _attn_result(width, bufs, ref, vmax, yard, n, done):
    I, nmax = ref.shape[:2]
    raws = tuple(b.cpu() for b in bufs)
    numel = I * nmax * width
    running = torch.tensor(done, dtype=torch.int32).repeat_interleave(2) == 0
    live = (torch.arange(nmax)[None, :] < n[:, None]) & running[:, None]
    untouched = all(bool((r[numel:] == SENTINEL).all()) and bool((r[:numel].view(I, nmax, width)[~live] == SENTINEL).all()) for r in raws)
    out = raws[0][:numel].view(I, nmax, width)
    n_live = torch.where(running, n, torch.zeros_like(n))
    fig = _attn_item_figures(width, out, ref, vmax, n_live)
    figure = float("nan") if bool(fig.isnan().any()) else fig.max().item()
    return AttnResult(out, ref, live, n_live, figure, yard[running].max().item() if bool(running.any()) else 0.0, untouched, raws)


def attn_items(ns, seed):
    return tuple((int(ni), seed * 1000 + i) for i, ni in enumerate(ns))


def lg_attention_case(lib, width, kind, items, nmax, nsel, split_items, family, done=None, device="cpu", runs=1):
    """dim_op_lg_attention_f32 in the arithmetic that is active at the call.  Every run gets a fresh copy of qkv (the fp32 path rotates it in place), a
    ctx of SENTINEL with a guard band behind it and a workspace of 0xff bytes: a tile image or a partial record that is read before it is written is NaN."""
    _bind_attention(lib)
    qkv, enc, n, ref, vmax, yard = _attn_inputs(width, kind, tuple(items), nmax, family)
    I = len(items)
    done = [0] * (I // 2) if done is None else list(done)
    ed, nd, dd = enc.to(device), n.to(device), torch.tensor(done, dtype=torch.int32).to(device)
    nbytes = int(lib.dim_op_lg_attention_workspace_bytes(width, I, nmax, split_items))
    bufs = []
    for _ in range(runs):
        qd = qkv.to(device, copy=True)
        ctx = _dense_out(I * nmax * width, device)
        ws = torch.full((nbytes + 16,), 0xff, dtype=torch.uint8, device=device)
        rc = lib.dim_op_lg_attention_f32(width, kind, p(qd), p(ed), p(nd), p(dd), p(ctx), I, nmax, nsel, split_items, p(ws), None)
        assert rc == 0, lib.dim_last_error()
        _sync(device)
        bufs.append(ctx)
    return _attn_result(width, bufs, ref, vmax, yard, n, done)


def lg_attention_error(lib, width, kind, device="cpu"):
    """A (width, kind, arithmetic) that the library does not have: the return code and the message; nothing may be written."""
    _bind_attention(lib)
    items = attn_items((40, 40), 1)
    qkv, enc, n, _, _, _ = _attn_inputs(width, kind, items, 64, "flat")
    ctx = _dense_out(2 * 64 * width, device)
    ws = torch.full((int(lib.dim_op_lg_attention_workspace_bytes(width, 2, 64, 0)) + 16,), 0xff, dtype=torch.uint8, device=device)
    rc = lib.dim_op_lg_attention_f32(width, kind, p(qkv.to(device, copy=True)), p(enc.to(device)), p(n.to(device)),
                                     p(torch.zeros(1, dtype=torch.int32, device=device)), p(ctx), 2, 64, 64, 0, p(ws), None)
    _sync(device)
    return rc, lib.dim_last_error().decode(), bool((ctx.cpu() == SENTINEL).all())


def check_attention(r, what=""):
    """Same bits from every run, nothing written outside the live rows, and the figure (printed first) within ATTN_FACTOR x the fp32 yardstick.
    -> (figure, yardstick)."""
    print(f"attention {what}: figure {r.figure:.4g} yardstick {r.yardstick:.4g} bound {ATTN_FACTOR * r.yardstick:.4g} "
          f"repeatable {r.repeatable} untouched {r.untouched}")
    assert r.repeatable, "two runs on the same inputs differ"
    assert r.untouched, "a row at or past n[item], a row of a stopped pair or the guard band was written"
    assert r.figure <= ATTN_FACTOR * r.yardstick, (r.figure, r.yardstick)
    return r.figure, r.yardstick


# ---- the cases (ids name what they reach) ----
ATTN_A = dict(ns=(70, 130), nmax=130, nsel=130)                                   # split_items 2 -> 4 parts: item 0's parts 2, 3 empty, part 1 six keys
ATTN_B = dict(ns=(33, 1, 0, 40, 129, 200, 64, 64), nmax=224, nsel=200)           # one key; no queries; no keys; tile + 1; tile-exact; pair 3 stopped
ATTN_C_PAIR = ((97, 90001), (130, 90002))                                        # the pair that sits in a 2-item and in a 6-item call
ATTN_C_NEIGHBOURS = ((130, 90003), (45, 90004), (1, 90005), (64, 90006))
ATTN_C = dict(nmax=130, nsel=130)


def attn_e_counts():
    """64 ragged counts in 0 .. 100 with 0, 1, 32, 33 and 100 among them."""
    ns = torch.randint(0, 101, (64,), generator=torch.Generator().manual_seed(64)).tolist()
    ns[3], ns[10], ns[17], ns[18], ns[40] = 0, 1, 32, 33, 100
    return tuple(ns)


ATTN_E = dict(ns=attn_e_counts(), nmax=100, nsel=100)                              # 4 heads x 64 items = 256 workgroups: two parts


def attn_ragged(items, nsel, seed):
    """`items` counts in 0 .. nsel, the first four pinned to nsel, 0, 1, nsel - 1."""
    ns = torch.randint(0, nsel + 1, (items,), generator=torch.Generator().manual_seed(seed)).tolist()
    ns[:4] = [nsel, 0, 1, nsel - 1]
    return tuple(ns)


# hardware only, many resident workgroups: (width, items, nsel, split_items, parts, attention workgroups = query blocks x heads x items x parts)
ATTN_OCCUPANCY = [(256, 64, 260, 0, 1, 768), (256, 32, 260, 32, 2, 768), (256, 20, 260, 20, 4, 960), (96, 64, 400, 64, 2, 512), (96, 128, 520, 0, 1, 640)]


def attn_parts(width, n_items, nsel, split_items):
    """The launchers' rule (launch_lg_attention_x6 / launch_lgl_attention) -> (parts, attention workgroups)."""
    wgs = -(-nsel // 128) * attn_heads(width)[0] * n_items
    parts = (1 if wgs >= 512 else 2 if wgs >= 256 else 4) if 0 < n_items <= split_items else 1
    return parts, wgs * parts


# ---- the fused entry: projection GEMM that writes the K | V images + attention with kv_ready ----
@functools.lru_cache(maxsize=4)
def _attn_fused_inputs(kind, items, nmax):
    """x ~ randn [items][nmax][256] (NaN at or past n), W ~ randn / 16 [256][768 | 512], bias ~ 0.1 randn; the fp64 reference of the WHOLE composition,
    the fp32 yardstick of the whole composition (fp32 projection, then the fp32 attention), and the fp64 projection rounded to fp32."""
    I, N = len(items), 768 if kind == 0 else 512
    g = torch.Generator().manual_seed(7000 + kind)
    W, bias = (torch.randn(256, N, generator=g) / 16).contiguous(), 0.1 * torch.randn(N, generator=g)
    x = torch.full((I, nmax, 256), float("nan"))
    enc = torch.full((I, nmax, 64), float("nan"))
    for i, (ni, seed) in enumerate(items):
        gi = torch.Generator().manual_seed(seed)
        x[i, :ni] = torch.randn(ni, 256, generator=gi)
        ang = torch.rand(ni, 32, generator=gi) * (2 * torch.pi)
        enc[i, :ni] = torch.cat([torch.cos(ang), torch.sin(ang)], dim=1)
    n = torch.tensor([it[0] for it in items], dtype=torch.int32)
    qkv64 = F.pad(x.double() @ W.double() + bias.double(), (0, 768 - N), value=float("nan"))
    ref, _ = _attn_eval(256, kind, qkv64, enc, n, torch.float64)
    vmax = _attn_vmax(256, kind, qkv64, n)
    qkv32 = F.pad(x @ W + bias, (0, 768 - N), value=float("nan"))
    yard = torch.zeros(I, dtype=torch.float64)
    for s in range(ATTN_PERMS):
        o32, _ = _attn_eval(256, kind, qkv32, enc, n, torch.float32, perm_seed=s if s else None)
        yard = torch.maximum(yard, _attn_item_figures(256, o32, ref, vmax, n))
    return x, W, bias, enc, n, ref, vmax, yard, qkv64.float()


def lg_qkv_attention_case(lib, kind, items, nmax, nsel, split_items, device="cpu", runs=1):
    """-> (fused, separate): dim_op_lg_qkv_attention_f32 on (x, W, bias), and dim_op_lg_attention_f32 on the fp64 projection rounded to fp32, both against
    the fp64 evaluation of the whole composition with the yardstick of the whole composition."""
    _bind_attention(lib)
    x, W, bias, enc, n, ref, vmax, yard, qkv_rounded = _attn_fused_inputs(kind, tuple(items), nmax)
    I, N = len(items), W.shape[1]
    done = [0] * (I // 2)
    xd, bd, ed, nd, dd = x.to(device), bias.to(device), enc.to(device), n.to(device), torch.zeros(I // 2, dtype=torch.int32, device=device)
    nbytes = int(lib.dim_op_lg_attention_workspace_bytes(256, I, nmax, split_items))
    handle, npad = ctypes.c_void_p(), ctypes.c_int()
    assert lib.dim_x3_create(p(W), 256, N, ctypes.byref(handle), ctypes.byref(npad)) == 0 and npad.value == N, lib.dim_last_error()
    fused, separate = [], []
    try:
        for _ in range(runs):
            for bufs in (fused, separate):
                ctx = _dense_out(I * nmax * 256, device)
                ws = torch.full((nbytes + 16,), 0xff, dtype=torch.uint8, device=device)
                if bufs is fused:
                    qd = torch.full((I, nmax, 768), SENTINEL, device=device)
                    rc = lib.dim_op_lg_qkv_attention_f32(kind, p(xd), handle, p(bd), p(ed), p(nd), p(dd), p(qd), p(ctx), I, nmax, nsel, split_items, p(ws), None)
                else:
                    qd = qkv_rounded.to(device, copy=True)
                    rc = lib.dim_op_lg_attention_f32(256, kind, p(qd), p(ed), p(nd), p(dd), p(ctx), I, nmax, nsel, split_items, p(ws), None)
                assert rc == 0, lib.dim_last_error()
                _sync(device)
                bufs.append(ctx)
    finally:
        lib.dim_x3_destroy(handle)
    return _attn_result(256, fused, ref, vmax, yard, n, done), _attn_result(256, separate, ref, vmax, yard, n, done)


def lg_qkv_attention_unfused_error(lib, device="cpu"):
    """A shape whose projection GEMM writes no tile images (bf16x6 never does; under fp16x3: 300 rows x 36 items runs the plain 64-row block)."""
    _bind_attention(lib)
    I, nmax = 36, 300
    W = torch.zeros(256, 768)
    handle, npad = ctypes.c_void_p(), ctypes.c_int()
    assert lib.dim_x3_create(p(W), 256, 768, ctypes.byref(handle), ctypes.byref(npad)) == 0, lib.dim_last_error()
    try:
        z = torch.zeros(16, device=device)
        zi = torch.zeros(I, dtype=torch.int32, device=device)
        rc = lib.dim_op_lg_qkv_attention_f32(0, p(z), handle, p(z), p(z), p(zi), p(zi), p(z), p(z), I, nmax, nmax, 0, p(z), None)
    finally:
        lib.dim_x3_destroy(handle)
    return rc, lib.dim_last_error().decode()


def saturation_op_count(lib, reset=False):
    """The DIM_SAT_OP counter (site 7 of include/dim_hip.h) through dim_saturation_read."""
    counts, total = (ctypes.c_uint * 16)(), ctypes.c_ulonglong()
    assert lib.dim_saturation_read(counts, ctypes.byref(total), int(reset), None) == 0, lib.dim_last_error()
    return int(counts[7])


# (width, kind, arithmetic = dim_tune_set key 1) that exist / that the library refuses: SuperGlue and width 96 have no fp32 form
ATTN_VARIANTS = [(256, k, m) for k in range(4) for m in (2, 1, 0) if not (k >= 2 and m == 0)] + [(96, k, m) for k in (0, 1) for m in (2, 1)]
ATTN_REFUSED = [(256, 2, 0), (256, 3, 0), (96, 0, 0), (96, 1, 0)]
ATTN_MODE_NAMES = {2: "fp16x3", 1: "bf16x6", 0: "fp32"}
ATTN_KIND_NAMES = ("self", "cross", "sg_self", "sg_cross")


def attn_variant_id(v):
    return f"w{v[0]}-{ATTN_KIND_NAMES[v[1]]}-{ATTN_MODE_NAMES[v[2]]}"


def attn_case_a(lib, width, kind, split_items, family, device="cpu", runs=2):
    return lg_attention_case(lib, width, kind, attn_items(ATTN_A["ns"], 1), ATTN_A["nmax"], ATTN_A["nsel"], split_items, family, device=device, runs=runs)


def attn_case_b(lib, width, kind, done3, split_items, device="cpu", runs=2):
    """Case B with done = (0, 0, 0, done3); besides the result, the exact-zero check of the empty key set: under kind 1 / 3 item 3 (40 rows) reads the keys
    of item 2, which has none (under kind 0 / 2 the item without keys has no queries either)."""
    r = lg_attention_case(lib, width, kind, attn_items(ATTN_B["ns"], 2), ATTN_B["nmax"], ATTN_B["nsel"], split_items, "flat", done=(0, 0, 0, done3),
                          device=device, runs=runs)
    assert not bool(r.live[6:].any()) and int(r.live.sum()) == sum(ATTN_B["ns"][:6])
    if kind in (1, 3):
        assert bool((r.out[3, :40] == 0.0).all()), "the rows of an item whose key set is empty are not exact zeros"
        assert not bool((r.out[1, :1] == 0.0).all())          # (item 1 reads item 0's 33 keys)
    return r


def attn_case_c(lib, width, kind, device="cpu", runs=2):
    """-> (the pair alone, the pair as items 4, 5 of a 6-item call), both with the key range in 4 parts."""
    alone = lg_attention_case(lib, width, kind, ATTN_C_PAIR, ATTN_C["nmax"], ATTN_C["nsel"], 2, "ramp", device=device, runs=runs)
    among = lg_attention_case(lib, width, kind, ATTN_C_NEIGHBOURS + ATTN_C_PAIR, ATTN_C["nmax"], ATTN_C["nsel"], 6, "ramp", device=device, runs=runs)
    assert attn_parts(width, 2, ATTN_C["nsel"], 2)[0] == 4 and attn_parts(width, 6, ATTN_C["nsel"], 6)[0] == 4
    return alone, among


def attn_case_e(lib, kind, device="cpu", runs=2):
    assert attn_parts(256, 64, ATTN_E["nsel"], 64) == (2, 512)
    return lg_attention_case(lib, 256, kind, attn_items(ATTN_E["ns"], 3), ATTN_E["nmax"], ATTN_E["nsel"], 64, "ramp", device=device, runs=runs)


def attn_case_guard(lib, kind, device="cpu", runs=1):
    """-> (result, DIM_SAT_OP count of the call) on the `guard` inputs (see _attn_inputs); the counter is cleared before and after."""
    saturation_op_count(lib, reset=True)
    r = lg_attention_case(lib, 256, kind, attn_items((40, 40), 4), 64, 40, 0, "guard", device=device, runs=runs)
    return r, saturation_op_count(lib, reset=True)


def attn_case_occupancy(lib, width, kind, items, nsel, split_items, parts, wgs, device="cuda", runs=2):
    assert attn_parts(width, items, nsel, split_items) == (parts, wgs)
    ns = attn_ragged(items, nsel, items + nsel)
    return lg_attention_case(lib, width, kind, attn_items(ns, 5), nsel, nsel, split_items, "ramp", device=device, runs=runs)


# ---------------------------------------------------------------------------------------------------------------- LightGlue head: confidence, decide, prune, assign, finalize
# dim_op_lg_confidence_f32 / dim_op_lg_decide / dim_op_lg_prune / dim_op_lg_assign_f32 / dim_op_lg_finalize (include/dim_hip.h) = the launchers of
# csrc/lg_kernels.hip (96-wide forms: lgl_kernels.hip) over caller tensors.  References: plain torch in fp64 on the CPU, written from the operation.
#   floating-point outputs   figure = max |out - fp64| over the live entries, yardstick = the same figure of an fp32 torch evaluation of the same formula
#                            (largest of HEAD_PERMS row / column / channel orders), bound = HEAD_FACTOR x yardstick.  Match scores exp(best): 2 ulp (below).
#   integer outputs          exact, every entry.  The builders assert on the fp64 reference that every decision has a margin of HEAD_MARGIN x the bound
#                            (top-two gaps, exp(best) against the filter threshold, conf / mtch against their thresholds); a seed that does not is skipped.
# Every buffer an op writes starts as 0xff bytes (NaN / -1) with a guard band of GUARD_ELEMS behind it; rows at or past n_cur hold NaN in every input.
HEAD_FACTOR, HEAD_PERMS, HEAD_MARGIN = 2.0, 4, 16.0
HEAD_PTRS = ("desc", "enc", "sim", "conf", "mtch", "zls", "rmax", "rlse", "best", "arg", "n_cur", "n_new", "n_orig", "ind", "dest", "prune", "done", "cnt_lt")
HEAD_LAYERS = 9
ARG_NONE = 0x7fffffff


class LgHeadState(ctypes.Structure):
    _fields_ = [("width", _ci), ("n_pairs", _ci), ("nmax", _ci), ("nsel", _ci)] + [(k, _vp) for k in HEAD_PTRS]


def _bind_head(lib):
    sp, cf = ctypes.POINTER(LgHeadState), ctypes.c_float
    lib.dim_op_lg_confidence_f32.argtypes = [sp, _vp, _vp, _vp, _vp, cf, _ci, _vp]
    lib.dim_op_lg_decide.argtypes = [sp, _ci, cf, _ci, _ci, _vp]
    lib.dim_op_lg_prune_workspace_bytes.argtypes = [_ci, _ci, _ci]
    lib.dim_op_lg_prune_workspace_bytes.restype = ctypes.c_size_t
    lib.dim_op_lg_prune.argtypes = [sp, _ci, ctypes.c_double, cf, _ci, _ci, _vp, _vp]
    lib.dim_op_lg_assign_f32.argtypes = [sp, _ci, _vp, _vp, _vp, _vp]
    lib.dim_op_lg_finalize.argtypes = [sp, _ci, _ci, cf, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
    for f in (lib.dim_op_lg_confidence_f32, lib.dim_op_lg_decide, lib.dim_op_lg_prune, lib.dim_op_lg_assign_f32, lib.dim_op_lg_finalize):
        f.restype = _ci


def _head_state(width, n_pairs, nmax, nsel, **tensors):
    hs = LgHeadState(width, n_pairs, nmax, nsel)
    for k, t in tensors.items():
        assert k in HEAD_PTRS
        setattr(hs, k, t.data_ptr())
    return hs


def _filled(numel, dtype, device, fill=0xff):
    """numel + GUARD_ELEMS elements of `dtype`, every byte `fill`."""
    item = torch.empty((), dtype=dtype).element_size()
    return torch.full(((numel + GUARD_ELEMS) * item,), fill, dtype=torch.uint8, device=device).view(dtype)


def _guarded(t, device, fill=0xff):
    """An in / out tensor: its values, flat, with the guard band behind them."""
    out = _filled(t.numel(), t.dtype, "cpu", fill)
    out[:t.numel()] = t.contiguous().view(-1)
    return out.to(device)


def _is_fill(flat, fill=0xff):
    """flat (CPU, 1-D) -> bool per element: every byte still holds `fill`."""
    return (flat.contiguous().view(torch.uint8).view(flat.numel(), flat.element_size()) == fill).all(dim=1)


def _same_bits(raws):
    return all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for r in raws[1:] for a, b in zip(raws[0], r))


def _first_argmax(x, dim):
    """(max, the LOWEST index that holds it) along dim — Tensor.max on the CPU, spelled out."""
    best = x.amax(dim=dim)
    idx = torch.arange(x.shape[dim]).view(-1, 1) if dim == 0 else torch.arange(x.shape[dim]).view(1, -1)
    return best, torch.where(x == best.unsqueeze(dim), idx, x.shape[dim]).amin(dim=dim)


@functools.lru_cache(maxsize=None)
def head_weights(width):
    """[HEAD_LAYERS][width] weight rows ~ randn / sqrt(width) (logits ~ N(0, 1) on randn descriptors) and biases ~ 0.3 randn, for the token and the
    matchability heads."""
    g = torch.Generator().manual_seed(4242 + width)
    return (torch.randn(HEAD_LAYERS, width, generator=g) / width ** 0.5, 0.3 * torch.randn(HEAD_LAYERS, generator=g),
            torch.randn(HEAD_LAYERS, width, generator=g) / width ** 0.5, 0.3 * torch.randn(HEAD_LAYERS, generator=g))


# ---- assignment ----
ASSIGN_THR = 0.1
TIE_ROWS = (5, 76)                                    # row groups 5 and 12 of both column kernels (64 and 16 groups)
TIE_COLS = {"lanes": (9, 70), "float4": (8, 10), "lane": (9, 73), "lane16": (9, 265)}   # 16-byte kernels: lane = (j / 4) % 64; generic: j % 64


def _assign_eval(sim, d0, d1, w, b, dtype):
    """LightGlue's log assignment (LGN:246-275) in `dtype`: -> zls0, zls1, lse0 (rows), lse1 (columns), score."""
    sim, d0, d1, w, b = sim.to(dtype), d0.to(dtype), d1.to(dtype), w.to(dtype), b.to(dtype)
    z0, z1 = F.logsigmoid(d0 @ w + b), F.logsigmoid(d1 @ w + b)
    score = F.log_softmax(sim, dim=1) + F.log_softmax(sim, dim=0) + z0[:, None] + z1[None, :]
    return z0, z1, torch.logsumexp(sim, dim=1), torch.logsumexp(sim, dim=0), score


class AssignPair(NamedTuple):
    sim: torch.Tensor      # [m][n] fp32
    d0: torch.Tensor       # [m][width]
    d1: torch.Tensor
    ref: dict              # fp64: zls0, zls1, lse0, lse1, score, best0, best1, arg0, arg1
    yard: dict             # zls, lse, best, dense -> the fp32 evaluation's figure
    seed: int


def _assign_errors(out, ref):
    """out / ref: (zls0, zls1, lse0, lse1, best0, best1, score) -> {zls, lse, best, dense}: max |out - ref|."""
    e = [(o.double() - r).abs().max().item() if r.numel() else 0.0 for o, r in zip(out, ref)]
    return {"zls": max(e[0], e[1]), "lse": max(e[2], e[3]), "best": max(e[4], e[5]), "dense": e[6]}


def _assign_try(width, m, n, family, ties, wrow, seed):
    g = torch.Generator().manual_seed(seed)
    _, _, W, B = head_weights(width)
    w, b = W[wrow], B[wrow]
    d0, d1 = torch.randn(m, width, generator=g), torch.randn(n, width, generator=g)
    rows, cols = torch.arange(m), torch.arange(n)
    if family == "ramp":   # + 5 per group of 64 rows (the stride of a thread of lg_col_stats4_kernel), centred; one column per row lifted by 3: a clear row maximum
        sim = 0.25 * torch.randn(m, n, generator=g) + 5.0 * (rows // 64)[:, None] - 2.5 * ((m - 1) // 64)
        sim[rows, torch.randint(0, n, (m,), generator=g)] += 3.0
    else:
        sim = 3.0 * torch.randn(m, n, generator=g)
    planted = None
    if family == "planted":
        k = max(1, round(0.6 * min(m, n)))
        pr, pc = torch.randperm(m, generator=g)[:k], torch.randperm(n, generator=g)[:k]
        sim[pr, pc] += 12.0
        for d, idx in ((d0, pr), (d1, pc)):   # matchability logits 1 .. 4 on the planted points
            d[idx] += ((1.0 + 3.0 * torch.rand(k, generator=g) - (d[idx] @ w + b)) / (w @ w))[:, None] * w
        planted = (pr, pc)
    keep_r, keep_c = torch.ones(m, dtype=torch.bool), torch.ones(n, dtype=torch.bool)
    tie_c = tie_r = None
    if ties:
        ca, cb = TIE_COLS[ties] if n > TIE_COLS[ties][1] else TIE_COLS["float4"]   # (a side of 37 columns: the pair inside one float4)
        sim[3:9, ca] += 15.0                      # rows whose maximum is the tied column
        if m > TIE_ROWS[1]:
            tie_r = TIE_ROWS
            sim[tie_r[0], 20:26] += 15.0          # columns whose maximum is the tied row
        sim[:, cb], d1[cb], keep_c[cb], tie_c = sim[:, ca], d1[ca], False, (ca, cb)
        if tie_r:
            sim[tie_r[1]], d0[tie_r[1]], keep_r[tie_r[1]] = sim[tie_r[0]], d0[tie_r[0]], False
    z0, z1, l0, l1, score = _assign_eval(sim, d0, d1, w, b, torch.float64)
    best0, arg0 = _first_argmax(score, 1)
    best1, arg1 = _first_argmax(score, 0)
    ref = dict(zls0=z0, zls1=z1, lse0=l0, lse1=l1, score=score, best0=best0, best1=best1, arg0=arg0, arg1=arg1)
    refs = (z0, z1, l0, l1, best0, best1, score)
    yard = dict(zls=0.0, lse=0.0, best=0.0, dense=0.0)
    for s in range(HEAD_PERMS):
        gp = torch.Generator().manual_seed(1000 * seed + s)
        pr_, pc_, pw_ = (torch.randperm(k_, generator=gp) if s else torch.arange(k_) for k_ in (m, n, width))
        y0, y1, yl0, yl1, ys = _assign_eval(sim[pr_][:, pc_], d0[pr_][:, pw_], d1[pc_][:, pw_], w[pw_], b, torch.float32)
        ir, ic = torch.argsort(pr_), torch.argsort(pc_)
        ys = ys[ir][:, ic]
        e = _assign_errors((y0[ir], y1[ic], yl0[ir], yl1[ic], ys.amax(dim=1), ys.amax(dim=0), ys), refs)
        yard = {k_: max(yard[k_], e[k_]) for k_ in yard}
    # margins of the integer outputs, on the reference (duplicates of a tie taken out: their gap is 0 by construction)
    need = HEAD_MARGIN * HEAD_FACTOR * max(yard["best"], yard["dense"])
    red = score[keep_r][:, keep_c]
    for dim in (1, 0):
        if red.shape[dim] >= 2:
            top = red.topk(2, dim=dim).values
            gap = (top.select(dim, 0) - top.select(dim, 1)).min().item()
            if gap < need:
                return None
    if family == "planted":
        mutual = arg1[arg0] == rows
        ms = torch.where(mutual, best0.exp(), torch.zeros_like(best0))
        if bool(((ms - ASSIGN_THR).abs()[mutual] < need).any()):
            return None
        on = torch.zeros(m, dtype=torch.bool)
        on[planted[0]] = True
        classes = (int((mutual & (ms > ASSIGN_THR) & on).sum()), int((~mutual).sum()), int((mutual & (ms <= ASSIGN_THR)).sum()))
        if min(m, n) >= 60:
            assert min(classes) > 0, ("planted: matches above the threshold on planted points, non-mutual rows and mutual rows below it", classes)
    if family == "ramp":
        for k_ in range(min(64, m)):   # the rows one thread of lg_col_stats4_kernel walks: its running maximum moves at every step
            chain = sim[k_::64]
            if chain.shape[0] > 1:
                assert bool((chain[1:] > chain[:-1].cummax(dim=0).values).all()), "ramp: a column's running maximum does not move"
    if tie_c:
        hit = (arg0 == tie_c[0]) & (score[:, tie_c[1]] == best0)
        assert bool(hit.any()), "ties: no row has its maximum in the tied columns"
    if tie_r:
        hit = (arg1 == tie_r[0]) & (score[tie_r[1]] == best1)
        assert bool(hit.any()), "ties: no column has its maximum in the tied rows"
    return AssignPair(sim, d0, d1, ref, yard, seed)


@functools.lru_cache(maxsize=None)
def assign_pair(width, m, n, family, ties, wrow, seed0):
    """The first seed from seed0 on whose fp64 reference has the margins (see the section head)."""
    for seed in range(seed0, seed0 + 300):
        r = _assign_try(width, m, n, family, ties, wrow, seed)
        if r is not None:
            return r
    raise AssertionError(f"no seed with the margins for {(width, m, n, family, ties)}")


class HeadResult(NamedTuple):
    figures: dict          # name -> (figure, yardstick) of the floating-point outputs
    exact: dict            # name -> bool: the integer output equals the reference in every entry
    untouched: bool        # every entry outside what the op must write, guard bands included, still holds the fill
    repeatable: bool       # every run wrote the same bits
    out: dict              # name -> the first run's tensor (CPU), for what a test looks at beyond this


def assign_case(lib, width, nmax, nsel, counts, family, tag, done=None, ties=None, seed=1, device="cpu", runs=2, items=None, pad=float("nan")):
    """dim_op_lg_assign_f32 on len(counts) pairs of (rows, columns) live points.  done: per pair (default: all == tag, or 1 .. for tag 0).  A pair runs
    when done == tag (tag > 0: weight row tag - 1) or, tag == 0, when done > 0 (row done - 1 of the tables); the others must keep the fill.
    items: (seed per pair), so that the same pair can sit in calls of different sizes.  pad: what the dead entries of sim hold (NaN; fmaxf and a compare
    drop a NaN by themselves, so a second form with a huge finite value shows a missing mask in the statistics)."""
    _bind_head(lib)
    P = len(counts)
    done = list(done) if done is not None else [tag if tag else 1 + i % HEAD_LAYERS for i in range(P)]
    _, _, W, B = head_weights(width)
    sim = torch.full((P, nmax, nmax), pad)
    desc = torch.full((2 * P, nmax, width), float("nan"))
    runs_pair = [(d == tag) if tag else d > 0 for d in done]
    pairs = []
    for i, (m, n) in enumerate(counts):
        wrow = (tag if tag else max(done[i], 1)) - 1
        pr = assign_pair(width, m, n, family, ties, wrow, (items[i] if items else 100 * seed + i)) if m and n else None
        pairs.append(pr)
        if pr is not None:
            sim[i, :m, :n], desc[2 * i, :m], desc[2 * i + 1, :n] = pr.sim, pr.d0, pr.d1
        else:   # an empty side: descriptors only
            gi = torch.Generator().manual_seed(7 + i)
            desc[2 * i, :m], desc[2 * i + 1, :n] = torch.randn(m, width, generator=gi), torch.randn(n, width, generator=gi)
    n_cur = torch.tensor([c for mn in counts for c in mn], dtype=torch.int32)
    simd, descd, nd, dd = sim.to(device), desc.to(device), n_cur.to(device), torch.tensor(done, dtype=torch.int32).to(device)
    wd, bd = (W[tag - 1].contiguous().to(device), B[tag - 1:tag].contiguous().to(device)) if tag else (W.contiguous().to(device), B.to(device))
    raws = []
    for _ in range(runs):
        o = {k: _filled(2 * P * nmax, torch.float32, device) for k in ("zls", "rmax", "rlse", "best")}
        o["arg"] = _filled(2 * P * nmax, torch.int32, device)
        dense = _filled(P * (nmax + 1) ** 2, torch.float32, device)
        hs = _head_state(width, P, nmax, nsel, desc=descd, sim=simd, n_cur=nd, done=dd, **o)
        rc = lib.dim_op_lg_assign_f32(ctypes.byref(hs), tag, p(wd), p(bd), p(dense), None)
        assert rc == 0, lib.dim_last_error()
        _sync(device)
        raws.append(tuple(o[k].cpu() for k in ("zls", "rmax", "rlse", "best", "arg")) + (dense.cpu(),))
    zls, rmax, rlse, best, arg, dense = raws[0]
    N = 2 * P * nmax
    live = torch.zeros(2 * P, nmax, dtype=torch.bool)
    dlive = torch.zeros(P, nmax + 1, nmax + 1, dtype=torch.bool)
    figs = {k: [0.0, 0.0] for k in ("zls", "lse", "best", "dense")}
    arg_ok = True
    v = lambda t: t[:N].view(2 * P, nmax)
    for i, (m, n) in enumerate(counts):
        if not runs_pair[i]:
            continue
        live[2 * i, :m], live[2 * i + 1, :n] = True, True
        pr = pairs[i]
        if pr is None:   # zls only: no row and no column statistics exist (the kernels write what they compute: -inf / log 0 / the sentinel index)
            wrow = (tag if tag else done[i]) - 1
            for s_, k_ in ((0, m), (1, n)):
                if k_:
                    zr = F.logsigmoid(desc[2 * i + s_, :k_].double() @ W[wrow].double() + B[wrow].double())
                    figs["zls"][0] = max(figs["zls"][0], (v(zls)[2 * i + s_, :k_].double() - zr).abs().max().item())
            continue
        dlive[i, :m, :n] = True
        out = (v(zls)[2 * i, :m], v(zls)[2 * i + 1, :n], v(rmax)[2 * i, :m].double() + v(rlse)[2 * i, :m].double(),
               v(rmax)[2 * i + 1, :n].double() + v(rlse)[2 * i + 1, :n].double(), v(best)[2 * i, :m], v(best)[2 * i + 1, :n],
               dense[:P * (nmax + 1) ** 2].view(P, nmax + 1, nmax + 1)[i, :m, :n])
        r = pr.ref
        e = _assign_errors(out, (r["zls0"], r["zls1"], r["lse0"], r["lse1"], r["best0"], r["best1"], r["score"]))
        for k in figs:
            figs[k] = [max(figs[k][0], e[k]), max(figs[k][1], pr.yard[k])]
        arg_ok = arg_ok and torch.equal(v(arg)[2 * i, :m].long(), r["arg0"]) and torch.equal(v(arg)[2 * i + 1, :n].long(), r["arg1"])
    untouched = True
    for raw in raws:
        for t in raw[:5]:   # (the live rows of an item whose other side is empty are written too, with -inf / the sentinel index: not compared)
            untouched = untouched and bool(_is_fill(t[N:]).all()) and bool(_is_fill(t[:N][~live.view(-1)]).all())
        D = P * (nmax + 1) ** 2
        untouched = untouched and bool(_is_fill(raw[5][D:]).all()) and bool(_is_fill(raw[5][:D][~dlive.view(-1)]).all())
    return HeadResult({k: tuple(x) for k, x in figs.items()}, {"arg": arg_ok}, untouched, _same_bits(raws),
                      dict(zls=v(zls), rmax=v(rmax), rlse=v(rlse), best=v(best), arg=v(arg), dense=dense[:P * (nmax + 1) ** 2].view(P, nmax + 1, nmax + 1), live=live))


def check_head(r, what=""):
    """Same bits from every run, nothing written outside the live entries, every integer output exact, every figure (printed first) within HEAD_FACTOR x
    its fp32 yardstick."""
    print(f"lg head {what}: " + " ".join(f"{k} {f:.4g}/{y:.4g}" for k, (f, y) in r.figures.items()) + f" exact {r.exact} repeatable {r.repeatable} untouched {r.untouched}")
    assert r.repeatable, "two runs on the same inputs differ"
    assert r.untouched, "an entry outside the live ones (a dead row, a stopped pair, the guard band) was written"
    assert all(r.exact.values()), r.exact
    for k, (f, y) in r.figures.items():
        assert f <= HEAD_FACTOR * y, (k, f, y)


ASSIGN_COUNTS = ((130, 129), (1, 131), (131, 1), (64, 65))
ASSIGN_BIG = ((37, 2049), (2049, 37))
# (name, nmax = nsel, counts): the 16-byte kernels with rows in 8 registers per lane, in 16, and the generic kernels (nmax no multiple of 4)
ASSIGN_PATHS = {"fast8": (132, ASSIGN_COUNTS), "fast16": (2052, ASSIGN_BIG), "generic": (134, ASSIGN_COUNTS)}


def assign_path_case(lib, width, path, family, ties=None, device="cpu", runs=2, pad=float("nan")):
    nmax, counts = ASSIGN_PATHS[path]
    if ties:   # the tied rows and columns need (130, 129) / (2049, 37) + (37, 2049)
        counts = counts[:1] if path != "fast16" else counts
    return assign_case(lib, width, nmax, nmax, counts, family, 3, ties=ties, seed=11 if path == "fast16" else 1, device=device, runs=runs, pad=pad)


def assign_stopped_case(lib, width, tag, device="cpu", runs=2):
    """tag 5: pairs 1 (stopped at layer 2) and 2 (left without keypoints) are not selected.  tag 0: pairs 0, 1, 3 stopped at layers 2, 5, 9 run with
    their own weight rows, pair 2 (still running) is not selected."""
    done = (5, 2, -3, 5) if tag else (2, 5, 0, 9)
    r = assign_case(lib, width, 132, 132, ASSIGN_COUNTS, "flat", tag, done=done, seed=2, device=device, runs=runs)
    skipped = [i for i, d in enumerate(done) if not ((d == tag) if tag else d > 0)]
    for i in skipped:   # (untouched covers it; spelled out because it is what the case is for)
        for k in ("zls", "rmax", "rlse", "best", "arg"):
            assert bool(_is_fill(r.out[k][2 * i:2 * i + 2].reshape(-1)).all()), (k, i)
        assert bool(_is_fill(r.out["dense"][i].reshape(-1)).all())
    return r


def head_ragged(n_items, nmax, seed):
    """Ragged counts in 0 .. nmax per item; the first pairs pinned to (nmax, 1), (0, nmax), (1, nmax - 1)."""
    ns = torch.randint(2, nmax + 1, (n_items,), generator=torch.Generator().manual_seed(seed)).tolist()
    ns[:6] = [nmax, 1, 0, nmax, 1, nmax - 1]
    return tuple((ns[2 * i], ns[2 * i + 1]) for i in range(n_items // 2))


def assign_occupancy_case(lib, width, device="cuda", runs=2):
    """16 pairs x nmax 260 with ragged counts (hardware: many workgroups resident at once), planted."""
    return assign_case(lib, width, 260, 260, head_ragged(32, 260, 5), "planted", 4, seed=3, device=device, runs=runs)


def assign_alone_and_among(lib, width, device="cuda"):
    """-> (a pair alone, the same pair as pair 9 of 16): its outputs must be the same bits."""
    counts = head_ragged(32, 260, 5)
    items = tuple(300 + i for i in range(16))
    among = assign_case(lib, width, 260, 260, counts, "flat", 4, device=device, runs=1, items=items)
    alone = assign_case(lib, width, 260, 260, counts[9:10], "flat", 4, device=device, runs=1, items=items[9:10])
    return alone, among


# ---- finalize ----
FINAL_THR, FINAL_LAYERS = 0.1, 9
ULP32 = 2.0 ** -23
# exp(best): the device's expf and the host's are specified to 1 ulp and the fp64 reference rounds once more, so a match score is within 2 ulp of exp in
# fp64 of the same fp32 `best`: figure = max relative error, "yardstick" 1 ulp, bound HEAD_FACTOR x that.


@functools.lru_cache(maxsize=None)
def _finalize_pair(m, n, mo, no, identity, bad, seed0):
    """Hand-built state of one pair: ind (a sorted subset of the original indices unless identity), arg with ~60 % of the smaller side mutual and the
    rest random (mostly not mutual), best0 = log of a score in 0.02 .. 0.98 — so there are valid matches, mutual rows below the threshold and
    non-mutual rows; prune counters 1 .. 8.  bad: row 7 and column 11 carry ARG_NONE (row 9 points at column 11, column 3 at row 7, the last column at row 7 and
    the last row at column 11)."""
    for seed in range(seed0, seed0 + 100):
        g = torch.Generator().manual_seed(seed)
        ind0 = torch.arange(m) if identity else torch.randperm(mo, generator=g)[:m].sort().values
        ind1 = torch.arange(n) if identity else torch.randperm(no, generator=g)[:n].sort().values
        k = max(1, round(0.6 * min(m, n)))
        pr, pc = torch.randperm(m, generator=g)[:k], torch.randperm(n, generator=g)[:k]
        arg0, arg1 = torch.randint(0, n, (m,), generator=g), torch.randint(0, m, (n,), generator=g)
        arg0[pr], arg1[pc] = pc, pr
        if bad:
            arg0[7], arg1[11], arg0[9], arg1[3] = ARG_NONE, ARG_NONE, 11, 7
            arg1[n - 1], arg0[m - 1] = 7, 11   # (what an index clamped into range would find: still no match)
        best0 = (0.02 + 0.96 * torch.rand(m, generator=g)).log()
        best1 = (0.02 + 0.96 * torch.rand(n, generator=g)).log()
        prune0, prune1 = torch.randint(1, 9, (mo,), generator=g), torch.randint(1, 9, (no,), generator=g)
        if bool(((best0.double().exp() - FINAL_THR).abs() < HEAD_MARGIN * HEAD_FACTOR * ULP32).any()):
            continue
        return ind0, ind1, arg0, arg1, best0, best1, prune0, prune1
    raise AssertionError("no seed with the margin")


def _finalize_reference(m, n, st, nmax, thr):
    """LightGlue's filter_matches (LGN:281-297) and the scatter through ind (LGN:543-566) in fp64; an arg outside the other side's range is "no match"."""
    ind0, ind1, arg0, arg1, best0 = st[0], st[1], st[2], st[3], st[4]
    in0, in1 = (arg0 >= 0) & (arg0 < n), (arg1 >= 0) & (arg1 < m)
    a0, a1 = arg0.clamp(0, max(n - 1, 0)), arg1.clamp(0, max(m - 1, 0))
    mutual0 = in0 & (arg1[a0] == torch.arange(m))
    mutual1 = in1 & (arg0[a1] == torch.arange(n))
    ms0 = torch.where(mutual0, best0.double().exp(), torch.zeros(m, dtype=torch.float64))
    ms1 = torch.where(mutual1, ms0[a1], torch.zeros(n, dtype=torch.float64))
    valid0 = mutual0 & (ms0 > thr)
    valid1 = mutual1 & valid0[a1]
    mfull, msfull = torch.full((2, nmax), -1, dtype=torch.int64), torch.zeros(2, nmax, dtype=torch.float64)
    mfull[0, ind0], msfull[0, ind0] = torch.where(valid0, ind1[a0], -1), ms0
    mfull[1, ind1], msfull[1, ind1] = torch.where(valid1, ind0[a1], -1), ms1
    rows = torch.nonzero(valid0).flatten()
    return mfull, msfull, torch.stack([ind0[rows], ind1[a0[rows]]], dim=1), ms0[rows], (int(valid0.sum()), int((~mutual0).sum()), int((mutual0 & ~valid0).sum()))


# (m, n, m_orig, n_orig, done): rows-per-thread split above 1024 rows, its transpose, three pruned 130 x 130 pairs: stopped, still running, left without keypoints
FINAL_PAIRS = ((1030, 37, 1032, 40, 5), (37, 1030, 37, 1032, 9), (130, 130, 150, 141, 3), (130, 130, 131, 150, 0), (130, 130, 140, 140, -4))


def finalize_case(lib, out_cap, prune_enabled, bad=False, identity=False, device="cpu", width=256):
    """dim_op_lg_finalize on FINAL_PAIRS (state given directly), twice on 0xff-filled outputs and once more on 0x5a-filled ones (a -1 that was never
    written is then visible).  bad: pair 2 carries ARG_NONE in one row and one column."""
    _bind_head(lib)
    P, nmax = len(FINAL_PAIRS), 1032
    best, arg = torch.full((2 * P, nmax), float("nan")), torch.full((2 * P, nmax), ARG_NONE, dtype=torch.int32)   # dead rows: NaN / an index that must not be followed
    ind, prune = torch.full((2 * P, nmax), ARG_NONE, dtype=torch.int32), torch.full((2 * P, nmax), -77, dtype=torch.int32)
    n_cur, n_orig, done = [], [], []
    exp = []
    for i, (m, n, mo, no, dn) in enumerate(FINAL_PAIRS):
        st = _finalize_pair(m, n, mo, no, identity and i < 2, bad and i == 2, 50 + i)
        ind[2 * i, :m], ind[2 * i + 1, :n], arg[2 * i, :m], arg[2 * i + 1, :n] = st[0].int(), st[1].int(), st[2].int(), st[3].int()
        best[2 * i, :m], best[2 * i + 1, :n], prune[2 * i, :mo], prune[2 * i + 1, :no] = st[4], st[5], st[6].int(), st[7].int()
        n_cur += [m, n]; n_orig += [mo, no]; done.append(dn)
        mfull, msfull, mt, msc, classes = _finalize_reference(m, n, st, nmax, FINAL_THR)
        if dn > 0 and i >= 2:
            assert min(classes) > 0 and classes[0] > 60, classes
        if dn <= 0:   # "no keypoints" exit / still running: no matches
            mfull, msfull, mt, msc = torch.full_like(mfull, -1), torch.zeros_like(msfull), mt[:0], msc[:0]
        po = torch.zeros(2, nmax, dtype=torch.int64)
        po[0, :mo], po[1, :no] = (st[6] if prune_enabled else FINAL_LAYERS), (st[7] if prune_enabled else FINAL_LAYERS)
        exp.append((mfull, msfull, mt, msc, po))
    dev = lambda t, dt=torch.int32: torch.tensor(t, dtype=dt).to(device)
    ins = dict(best=best.to(device), arg=arg.to(device), ind=ind.to(device), prune=prune.to(device), n_cur=dev(n_cur), n_orig=dev(n_orig), done=dev(done))
    raws, ok, unt, fig = [], {k: True for k in ("matches", "n_matches", "mfull", "stop", "prune_out")}, True, 0.0
    for fill in (0xff, 0xff, 0x5a):
        o = dict(matches=_filled(P * out_cap * 2, torch.int64, device, fill), mscores=_filled(P * out_cap, torch.float32, device, fill),
                 n_matches=_filled(P, torch.int32, device, fill), mfull=_filled(2 * P * nmax, torch.int32, device, fill),
                 msfull=_filled(2 * P * nmax, torch.float32, device, fill), stop=_filled(P, torch.int32, device, fill),
                 prune_out=_filled(2 * P * nmax, torch.int32, device, fill))
        hs = _head_state(width, P, nmax, 1030, **ins)
        rc = lib.dim_op_lg_finalize(ctypes.byref(hs), FINAL_LAYERS, prune_enabled, FINAL_THR, out_cap, *(p(o[k]) for k in
                                    ("matches", "mscores", "n_matches", "mfull", "msfull", "stop", "prune_out")), None)
        assert rc == 0, lib.dim_last_error()
        _sync(device)
        c = {k: t.cpu() for k, t in o.items()}
        if fill == 0xff:
            raws.append(tuple(c.values()))
        for k, numel in (("matches", P * out_cap * 2), ("mscores", P * out_cap), ("n_matches", P), ("mfull", 2 * P * nmax), ("msfull", 2 * P * nmax), ("stop", P), ("prune_out", 2 * P * nmax)):
            unt = unt and bool(_is_fill(c[k][numel:], fill).all())
        mt_o, ms_o = c["matches"][:P * out_cap * 2].view(P, out_cap, 2), c["mscores"][:P * out_cap].view(P, out_cap)
        mf_o, msf_o, po_o = (c[k][:2 * P * nmax].view(P, 2, nmax) for k in ("mfull", "msfull", "prune_out"))
        for i, (mfull, msfull, mt, msc, po) in enumerate(exp):
            k = min(mt.shape[0], out_cap)
            ok["n_matches"] = ok["n_matches"] and int(c["n_matches"][i]) == k
            ok["stop"] = ok["stop"] and int(c["stop"][i]) == abs(FINAL_PAIRS[i][4])
            ok["matches"] = ok["matches"] and torch.equal(mt_o[i, :k], mt[:k])
            ok["mfull"] = ok["mfull"] and torch.equal(mf_o[i].long(), mfull)
            ok["prune_out"] = ok["prune_out"] and torch.equal(po_o[i].long(), po)
            unt = unt and bool(_is_fill(mt_o[i, k:].reshape(-1), fill).all()) and bool(_is_fill(ms_o[i, k:].reshape(-1), fill).all())
            ok["mfull"] = ok["mfull"] and torch.equal(msf_o[i] == 0, msfull == 0)   # exact zeros where there is no mutual match
            for got, ref in ((ms_o[i, :k].double(), msc[:k]), (msf_o[i].double(), msfull)):
                nz = ref > 0
                if bool(nz.any()):
                    fig = max(fig, ((got[nz] - ref[nz]).abs() / ref[nz]).max().item())
    return HeadResult({"score": (fig, ULP32)}, ok, unt, _same_bits(raws), dict(mfull=mf_o, msfull=msf_o, n_matches=c["n_matches"][:P], matches=mt_o, exp=exp))


# ---- prune ----
PRUNE_MIN, PRUNE_WIDTH_CONF, PRUNE_THR = 40, 0.99, 0.85
# (rows side 0, rows side 1, done, kind of each side): the scan with two rows per thread (1030), n == pruning_min and + 1, a side that loses nothing,
# a side that loses everything, a stopped pair
PRUNE_PAIRS = ((130, 1030, 0, "nn"), (PRUNE_MIN, PRUNE_MIN + 1, 0, "nn"), (130, 130, 0, "kn"), (130, 64, 0, "an"), (100, 90, 3, "nn"), (1030, 130, 0, "nn"))


def prune_ws_layout(width, n_items, nmax):
    """Byte offsets of tdesc | tenc | tind in the workspace of dim_op_lg_prune (each piece rounded up to 256 bytes) and the total."""
    up = lambda v: (v + 255) // 256 * 256
    rows = n_items * nmax
    tenc = up(rows * width * 4)
    tind = tenc + up(rows * (64 if width == 256 else 96) * 4)
    return 0, tenc, tind, tind + up(rows * 4)


def _prune_scores(n_cur, done, kinds, nmax, seed, exact_rows):
    """conf, mtch [items][nmax] (NaN at or past n): mtch = u^6 (46 % at or below the keep threshold 0.01), conf = u.  kind k: mtch in 0.5 .. 1 (nothing goes);
    a: mtch below 0.005 and conf above 0.9 (everything goes).  exact_rows: item 0 holds mtch == the threshold itself in row 2 (not kept: the compare is >)
    and conf == its threshold in row 4 with a small mtch (kept with the token: the compare is <=)."""
    g = torch.Generator().manual_seed(seed)
    I = len(n_cur)
    conf, mtch = torch.full((I, nmax), float("nan")), torch.full((I, nmax), float("nan"))
    for it in range(I):
        n, kind = int(n_cur[it]), kinds[it]
        u, c = torch.rand(n, generator=g), torch.rand(n, generator=g)
        mtch[it, :n] = u ** 6 if kind == "n" else (0.5 + 0.5 * u if kind == "k" else 0.005 * u)
        conf[it, :n] = c if kind != "a" else 0.9 + 0.1 * c
    if exact_rows and n_cur[0] > 4:
        mtch[0, 2], conf[0, 2] = torch.tensor(1.0 - PRUNE_WIDTH_CONF, dtype=torch.float32), 0.95
        mtch[0, 4], conf[0, 4] = 0.001, torch.tensor(PRUNE_THR, dtype=torch.float32)
    return conf, mtch


def prune_reference(s, conf, mtch, layer, use_token, nmax):
    """One pruning pass (LGN:501-516, 586-591) on the state s (dict of CPU tensors, changed in place): a boolean-mask ordered compaction.
    -> (dest, n_new, per item: did its rows move) with -2 / -2 where nothing is written."""
    keep_thr, thr = torch.tensor(1.0 - PRUNE_WIDTH_CONF, dtype=torch.float32), torch.tensor(PRUNE_THR, dtype=torch.float32)
    I = s["n_cur"].numel()
    dest, n_new, moved = torch.full((I, nmax), -2, dtype=torch.int64), torch.full((I,), -2, dtype=torch.int64), [False] * I
    for it in range(I):
        if int(s["done"][it // 2]) != 0:
            continue
        n = int(s["n_cur"][it])
        n_new[it] = n
        if n <= PRUNE_MIN:
            continue
        keep = mtch[it, :n] > keep_thr
        if use_token:
            keep = keep | (conf[it, :n] <= thr)
        dest[it, :n] = torch.where(keep, torch.cumsum(keep, 0) - 1, -1)
        k = int(keep.sum())
        n_new[it] = k
        s["prune"][it, s["ind"][it, :n][keep].long()] += 1
        if k < n:
            moved[it] = True
            for name in ("desc", "enc", "ind"):
                s[name][it, :k] = s[name][it, :n][keep]
    for pr in range(I // 2):
        if int(s["done"][pr]) == 0:
            s["n_cur"][2 * pr:2 * pr + 2] = n_new[2 * pr:2 * pr + 2].int()
            if int(n_new[2 * pr]) == 0 or int(n_new[2 * pr + 1]) == 0:
                s["done"][pr] = -(layer + 2)
    return dest, n_new, moved


def prune_initial_state(width, pairs, nmax, seed):
    g = torch.Generator().manual_seed(seed)
    I, ew = 2 * len(pairs), 64 if width == 256 else 96
    n_cur = torch.tensor([c for pr in pairs for c in pr[:2]], dtype=torch.int32)
    desc, enc = torch.full((I, nmax, width), float("nan")), torch.full((I, nmax, ew), float("nan"))
    for it in range(I):
        desc[it, :n_cur[it]], enc[it, :n_cur[it]] = torch.randn(int(n_cur[it]), width, generator=g), torch.randn(int(n_cur[it]), ew, generator=g)
    return dict(desc=desc, enc=enc, ind=torch.arange(nmax, dtype=torch.int32).repeat(I, 1), prune=torch.ones(I, nmax, dtype=torch.int32), n_cur=n_cur,
                done=torch.tensor([pr[2] for pr in pairs], dtype=torch.int32))


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))


def prune_round(lib, width, state, kinds, layer, use_token, nmax, nsel, seed, exact_rows=False, device="cpu"):
    """dim_op_lg_prune on `state` (not modified) -> (HeadResult, the reference state after the pass).  Twice on 0xff-filled outputs and workspace and once
    on 0x5a-filled ones (dest holds -1 for a dropped point)."""
    _bind_head(lib)
    I = state["n_cur"].numel()
    conf, mtch = _prune_scores(state["n_cur"], state["done"], kinds, nmax, seed, exact_rows)
    after = {k: t.clone() for k, t in state.items()}
    dest, n_new, moved = prune_reference(after, conf, mtch, layer, use_token, nmax)
    nbytes = int(lib.dim_op_lg_prune_workspace_bytes(width, I, nmax))
    o_desc, o_enc, o_ind, total = prune_ws_layout(width, I, nmax)
    assert nbytes == total
    names = ("desc", "enc", "ind", "prune", "n_cur", "done")
    ok, unt, raws = {k: True for k in names + ("dest", "n_new", "scratch")}, True, []
    confd, mtchd = conf.to(device), mtch.to(device)
    ew = 64 if width == 256 else 96
    for fill in (0xff, 0xff, 0x5a):
        io = {k: _guarded(state[k], device, fill) for k in names}
        o = dict(dest=_filled(I * nmax, torch.int32, device, fill), n_new=_filled(I, torch.int32, device, fill))
        ws = torch.full((nbytes + 16,), fill, dtype=torch.uint8, device=device)
        hs = _head_state(width, I // 2, nmax, nsel, conf=confd, mtch=mtchd, **io, **o)
        rc = lib.dim_op_lg_prune(ctypes.byref(hs), layer, PRUNE_WIDTH_CONF, PRUNE_THR, use_token, PRUNE_MIN, p(ws), None)
        assert rc == 0, lib.dim_last_error()
        _sync(device)
        c = {k: t.cpu() for k, t in {**io, **o}.items()}
        wsc = ws.cpu()
        if fill == 0xff:
            raws.append(tuple(c.values()))
        for k in names:
            numel = state[k].numel()
            ok[k] = ok[k] and _bits_equal(c[k][:numel], after[k])
            unt = unt and bool(_is_fill(c[k][numel:], fill).all())
        d_o, n_o = c["dest"][:I * nmax].view(I, nmax), c["n_new"][:I]
        written = dest != -2
        ok["dest"] = ok["dest"] and torch.equal(d_o.long()[written], dest[written])
        ok["n_new"] = ok["n_new"] and torch.equal(n_o.long()[n_new != -2], n_new[n_new != -2])
        unt = unt and bool(_is_fill(d_o[~written], fill).all()) and bool(_is_fill(n_o[n_new == -2], fill).all())
        unt = unt and bool(_is_fill(c["dest"][I * nmax:], fill).all()) and bool(_is_fill(c["n_new"][I:], fill).all()) and bool((wsc[nbytes:] == fill).all())
        for it in range(I):   # an item whose rows do not move (stopped, at or below pruning_min, nothing pruned) leaves its scratch alone
            if not moved[it]:
                for off, rowb in ((o_desc, width * 4), (o_enc, ew * 4), (o_ind, 4)):
                    ok["scratch"] = ok["scratch"] and bool((wsc[off + it * nmax * rowb:off + (it + 1) * nmax * rowb] == fill).all())
    return HeadResult({}, ok, unt, _same_bits(raws), dict(dest=dest, n_new=n_new, moved=moved, conf=conf, mtch=mtch)), after


def prune_case(lib, width, use_token, pairs=PRUNE_PAIRS, nmax=1032, nsel=1030, device="cpu"):
    """Two pruning rounds in sequence on `pairs` -> (result of round 1, of round 2, state after 1, after 2)."""
    kinds = [k for pr in pairs for k in pr[3]]
    s0 = prune_initial_state(width, pairs, nmax, 900 + width)
    r1, s1 = prune_round(lib, width, s0, kinds, 2, use_token, nmax, nsel, 31, exact_rows=True, device=device)
    r2, s2 = prune_round(lib, width, s1, ["n"] * len(kinds), 3, use_token, nmax, nsel, 32, device=device)
    return r1, r2, s1, s2


def prune_ragged_pairs(n_pairs, nmax, seed):
    return tuple((m, n, 0, "nn") for m, n in head_ragged(2 * n_pairs, nmax, seed))


# ---- confidence and decide ----
CONF_NS, CONF_DONE, CONF_CNT0 = (1, 31, 32, 33, 130, 64, 50, 50), (0, 0, 0, 2), (3, 0, 7, 5)   # around the 32 rows of a workgroup; pair 3 stopped


@functools.lru_cache(maxsize=None)
def _confidence_inputs(width, ns, layer, seed0):
    Wt, Bt, Wm, Bm = head_weights(width)
    keep_thr = 1.0 - PRUNE_WIDTH_CONF
    for seed in range(seed0, seed0 + 100):
        g = torch.Generator().manual_seed(seed)
        desc = [torch.randn(n, width, generator=g) for n in ns]
        ref = [(torch.sigmoid(d.double() @ Wt[layer].double() + Bt[layer].double()), torch.sigmoid(d.double() @ Wm[layer].double() + Bm[layer].double())) for d in desc]
        yard = [0.0, 0.0]
        for s in range(HEAD_PERMS):
            pw = torch.randperm(width, generator=torch.Generator().manual_seed(77 * seed + s)) if s else torch.arange(width)
            for d, (rc_, rm_) in zip(desc, ref):
                yard[0] = max(yard[0], (torch.sigmoid(d[:, pw] @ Wt[layer][pw] + Bt[layer]).double() - rc_).abs().max().item())
                yard[1] = max(yard[1], (torch.sigmoid(d[:, pw] @ Wm[layer][pw] + Bm[layer]).double() - rm_).abs().max().item())
        if all(bool(((rc_ - PRUNE_THR).abs() >= HEAD_MARGIN * HEAD_FACTOR * yard[0]).all()) and bool(((rm_ - keep_thr).abs() >= HEAD_MARGIN * HEAD_FACTOR * yard[1]).all())
               for rc_, rm_ in ref):
            return desc, ref, yard
    raise AssertionError("no seed with the margins")


def confidence_case(lib, width, use_token, ns=CONF_NS, done=CONF_DONE, nmax=132, nsel=130, device="cpu", runs=2, layer=4):
    """dim_op_lg_confidence_f32: conf, mtch and the per-pair count of conf < PRUNE_THR on top of what cnt_lt held."""
    _bind_head(lib)
    I = len(ns)
    descs, ref, yard = _confidence_inputs(width, tuple(ns), layer, 60)
    Wt, Bt, Wm, Bm = head_weights(width)
    desc = torch.full((I, nmax, width), float("nan"))
    for it, d in enumerate(descs):
        desc[it, :ns[it]] = d
    cnt0 = torch.tensor([CONF_CNT0[i % 4] for i in range(I // 2)], dtype=torch.int32)
    descd, nd, dd = desc.to(device), torch.tensor(ns, dtype=torch.int32).to(device), torch.tensor(done, dtype=torch.int32).to(device)
    w = [t.contiguous().to(device) for t in (Wt[layer], Bt[layer:layer + 1], Wm[layer], Bm[layer:layer + 1])]
    raws = []
    for _ in range(runs):
        o = dict(conf=_filled(I * nmax, torch.float32, device), mtch=_filled(I * nmax, torch.float32, device), cnt_lt=_guarded(cnt0, device))
        hs = _head_state(width, I // 2, nmax, nsel, desc=descd, n_cur=nd, done=dd, **o)
        rc = lib.dim_op_lg_confidence_f32(ctypes.byref(hs), p(w[0]), p(w[1]), p(w[2]), p(w[3]), PRUNE_THR, use_token, None)
        assert rc == 0, lib.dim_last_error()
        _sync(device)
        raws.append(tuple(o[k].cpu() for k in ("conf", "mtch", "cnt_lt")))
    conf, mtch, cnt = raws[0]
    live = torch.zeros(I, nmax, dtype=torch.bool)
    fc = fm = 0.0
    cnt_ref = cnt0.clone().long()
    for it in range(I):
        if done[it // 2] != 0:
            continue
        live[it, :ns[it]] = True
        co, mo = conf[:I * nmax].view(I, nmax)[it, :ns[it]].double(), mtch[:I * nmax].view(I, nmax)[it, :ns[it]].double()
        fm = max(fm, (mo - ref[it][1]).abs().max().item())
        if use_token:
            fc = max(fc, (co - ref[it][0]).abs().max().item())
            cnt_ref[it // 2] += int((ref[it][0] < PRUNE_THR).sum())
        else:
            fc = max(fc, co.abs().max().item())   # exact zeros
    unt = all(bool(_is_fill(r[k][I * nmax:]).all()) and bool(_is_fill(r[k][:I * nmax][~live.view(-1)]).all()) for r in raws for k in (0, 1))
    unt = unt and all(bool(_is_fill(r[2][I // 2:]).all()) for r in raws)
    return HeadResult({"conf": (fc, yard[0] if use_token else 0.0), "mtch": (fm, yard[1])}, {"cnt_lt": torch.equal(cnt[:I // 2].long(), cnt_ref)}, unt,
                      _same_bits(raws), dict(cnt_lt=cnt[:I // 2], cnt_ref=cnt_ref))


DECIDE_DONE, DECIDE_NORIG = (0, 0, 0, 4, -2, 0, 0), ((100, 100), (100, 100), (130, 70), (50, 50), (0, 9), (1, 1), (2048, 2048))
DECIDE_CNT, DECIDE_DEPTH_CONF = (3, 40, 11, 6, 0, 0, 200), 0.95   # confident ratios 0.985, 0.8, 0.945, -, -, 1.0, 0.951


def decide_case(lib, early, last, layer=5, device="cpu", runs=2):
    """dim_op_lg_decide: the early-stop decision (LGN:593-604) in the reference's own fp32 form, 1 - count / points > depth_confidence; the counters return
    to 0 for every pair and a stopped pair keeps its layer."""
    _bind_head(lib)
    P = len(DECIDE_DONE)
    done, cnt = torch.tensor(DECIDE_DONE, dtype=torch.int32), torch.tensor(DECIDE_CNT, dtype=torch.int32)
    n_orig = torch.tensor([c for pr in DECIDE_NORIG for c in pr], dtype=torch.int32)
    ratio64 = 1.0 - cnt.double() / n_orig.view(P, 2).sum(1).double()
    assert bool(((ratio64 - DECIDE_DEPTH_CONF).abs() > 1e-4).all()) and bool((ratio64 > DECIDE_DEPTH_CONF).any()) and bool((ratio64 < DECIDE_DEPTH_CONF).any())
    ratio = 1.0 - cnt.float() / n_orig.view(P, 2).sum(1).float()
    stop = torch.full((P,), bool(last)) if last else (ratio > DECIDE_DEPTH_CONF) & bool(early)
    ref = torch.where((done == 0) & stop, torch.full_like(done, layer + 1), done)
    nd = n_orig.to(device)
    raws = []
    for _ in range(runs):
        o = dict(done=_guarded(done, device), cnt_lt=_guarded(cnt, device))
        hs = _head_state(256, P, 8, 8, n_orig=nd, **o)
        rc = lib.dim_op_lg_decide(ctypes.byref(hs), layer, DECIDE_DEPTH_CONF, early, last, None)
        assert rc == 0, lib.dim_last_error()
        _sync(device)
        raws.append(tuple(o[k].cpu() for k in ("done", "cnt_lt")))
    unt = all(bool(_is_fill(r[k][P:]).all()) for r in raws for k in (0, 1))
    return HeadResult({}, {"done": torch.equal(raws[0][0][:P], ref), "cnt_lt": bool((raws[0][1][:P] == 0).all())}, unt, _same_bits(raws), dict(done=raws[0][0][:P], ref=ref))
