"""Reference semantics of the nearest-neighbour matcher (kornia.feature.DescriptorMatcher's nn / mnn / snn / smnn; kornia is not installed,
so its rules are restated here) and the fp64 decision rule the parity tests use.

(a) ``reference_fp32``: the reference's own arithmetic — torch.cdist + torch.topk in fp32.
(b) ``classify_fp64``: exact fp64 squared distances computed BY DIFFERENCES; every candidate (i, j) is classed must / may / must-not from the
    elementary tests (row argmin, column argmin, row ratio, column ratio), each robustly true, robustly false or undecidable when every d^2 may
    move by +-tol.  An implementation passes when must <= output <= must | may (``check_rule``).
``tol`` is measured, not chosen: 4 x max |the reference's fp32 d^2 - the fp64 d^2| on the same inputs (``measured_tol``); the factor 4 covers the
tile-wise accumulation order and the separately summed norms of the library against torch's single matmul."""
from __future__ import annotations

import numpy as np
import torch

MODES = ("nn", "mnn", "snn", "smnn")


def reference_d2_fp32(desc0: torch.Tensor, desc1: torch.Tensor) -> torch.Tensor:
    """What torch.cdist squares-roots at these sizes (its matmul form): clamp_min(|a|^2 + |b|^2 - 2 a.b, 1e-30) in fp32, on the CPU."""
    a, b = desc0.detach().float().cpu(), desc1.detach().float().cpu()
    return ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (a @ b.t())).clamp_min(1e-30)


def reference_fp32(desc0, desc1, mode: str, th: float = 0.8):
    """(matches (S, 2) int64 numpy, idx0-ascending; dists (S,) float32 numpy) by the rules of kornia's match_nn / match_mnn / match_snn /
    match_smnn on dm = torch.cdist(desc0, desc1) in fp32."""
    a, b = torch.as_tensor(desc0).detach().float().cpu(), torch.as_tensor(desc1).detach().float().cpu()
    M, N = a.shape[0], b.shape[0]
    empty = (np.zeros((0, 2), np.int64), np.zeros(0, np.float32))
    if M == 0 or N == 0 or (mode == "snn" and N < 2) or (mode == "smnn" and (M < 2 or N < 2)):
        return empty
    dm = torch.cdist(a, b)
    ar = torch.arange(M)
    if mode in ("nn", "mnn"):
        v, j = dm.min(1)
        keep = torch.ones(M, dtype=torch.bool) if mode == "nn" else dm.min(0).indices[j] == ar
        dist = v
    else:
        v, idx = torch.topk(dm, 2, dim=1, largest=False)
        j, ratio = idx[:, 0], v[:, 0] / v[:, 1]
        keep = ratio <= th                     # a NaN ratio compares false
        dist = ratio
        if mode == "smnn":
            vc, ic = torch.topk(dm.t(), 2, dim=1, largest=False)
            rc = vc[:, 0] / vc[:, 1]
            keep = keep & (rc[j] <= th) & (ic[j, 0] == ar)
            dist = torch.maximum(ratio, rc[j])
    sel = torch.nonzero(keep).reshape(-1)
    return torch.stack([sel, j[sel]], 1).numpy().astype(np.int64), dist[sel].numpy().astype(np.float32)


def d2_fp64(desc0: torch.Tensor, desc1: torch.Tensor, device=None) -> torch.Tensor:
    """Exact-arithmetic stand-in: sum_k (a_k - b_k)^2 in fp64, by differences (no cancellation), chunked; on ``device`` (default: desc0's)."""
    dev = torch.device(device) if device is not None else desc0.device
    a, b = desc0.detach().to(dev, torch.float64), desc1.detach().to(dev, torch.float64)
    M, N, D = a.shape[0], b.shape[0], a.shape[1] if a.ndim == 2 else 0
    out = torch.empty(M, N, dtype=torch.float64, device=dev)
    c = max(1, (1 << 25) // max(1, N * D))     # <= 256 MB of differences per chunk
    for i0 in range(0, M, c):
        out[i0:i0 + c] = ((a[i0:i0 + c, None, :] - b[None, :, :]) ** 2).sum(-1)
    return out


def measured_tol(desc0, desc1, d2: torch.Tensor) -> float:
    """4 x the reference arithmetic's own fp32 error on these inputs."""
    if d2.numel() == 0:
        return 0.0
    ref = reference_d2_fp32(desc0, desc1).to(d2.device, torch.float64)
    return 4.0 * float((ref - d2).abs().max())


def _best2(d2: torch.Tensor):
    """per row: (min, argmin, second-smallest value); a missing second is +inf"""
    M, N = d2.shape
    if N >= 2:
        v, i = torch.topk(d2, 2, dim=1, largest=False)
        return v[:, 0], i[:, 0], v[:, 1]
    v, i = d2.min(1)
    return v, i, torch.full_like(v, float("inf"))


def classify_fp64(desc0, desc1, mode: str, th: float, tol: float, d2: torch.Tensor = None):
    """(must, may): sets of (i, j).  Everything else is must-not."""
    if d2 is None:
        d2 = d2_fp64(torch.as_tensor(desc0), torch.as_tensor(desc1))
    M, N = d2.shape
    if M == 0 or N == 0 or (mode == "snn" and N < 2) or (mode == "smnn" and (M < 2 or N < 2)):
        return set(), set()
    rmin, rarg, rsec = _best2(d2)
    cmin, carg, csec = _best2(d2.t())
    use_col = mode in ("mnn", "smnn")
    # candidates that are not robustly false on the argmin tests: within 2 tol of the row minimum (and of the column minimum)
    cand = d2 <= (rmin[:, None] + 2 * tol)
    if use_col:
        cand &= d2 <= (cmin[None, :] + 2 * tol)
    ii, jj = torch.nonzero(cand, as_tuple=True)
    d = d2[ii, jj]
    r_other = torch.where(rarg[ii] == jj, rsec[ii], rmin[ii])      # the best of the row without j
    c_other = torch.where(carg[jj] == ii, csec[jj], cmin[jj])      # the best of the column without i
    th2 = float(th) ** 2

    def argmin_true(other):
        return d + 2 * tol < other

    def ratio_state(other):      # sqrt(d / other) <= th  <=>  d <= th^2 other, with d and other each moving by +-tol; 0 / 0 is no match
        lo_other = other - tol
        true = (lo_other > 0) & (d + tol <= th2 * lo_other)
        false = (d - tol).clamp_min(0) > th2 * (other + tol)
        return true, false

    must = torch.ones_like(d, dtype=torch.bool)
    never = torch.zeros_like(d, dtype=torch.bool)
    must &= argmin_true(r_other)
    if use_col:
        must &= argmin_true(c_other)
    if mode in ("snn", "smnn"):
        t, f = ratio_state(r_other)
        must &= t
        never |= f
    if mode == "smnn":
        t, f = ratio_state(c_other)
        must &= t
        never |= f
    ii, jj, must, never = ii.cpu().numpy(), jj.cpu().numpy(), must.cpu().numpy(), never.cpu().numpy()
    must_set = {(int(i), int(j)) for i, j in zip(ii[must], jj[must])}
    may = ~must & ~never
    may_set = {(int(i), int(j)) for i, j in zip(ii[may], jj[may])}
    return must_set, may_set


def check_rule(matches: np.ndarray, must: set, may: set, what: str = "") -> None:
    """must <= output <= must | may; rows unique in idx0 and ascending."""
    m = np.asarray(matches).reshape(-1, 2)
    assert np.all(np.diff(m[:, 0]) > 0), f"{what}: idx0 not strictly ascending"
    got = {(int(i), int(j)) for i, j in m}
    missing, extra = must - got, got - must - may
    assert not missing and not extra, f"{what}: {len(missing)} must-matches missing {sorted(missing)[:5]}, {len(extra)} must-not matches present {sorted(extra)[:5]}"


def planted(n: int, dim: int = 256, seed: int = 0, noise: float = 0.12, replaced: float = 0.0, extra1: int = 0):
    """Unit-norm descriptors with planted correspondences: a = normalize(randn), b = normalize(a[perm] + U(0,1) noise randn); a fraction
    ``replaced`` of b's rows is replaced by fresh random directions (their partners in a have no true match: the ratio test rejects them) and
    ``extra1`` unrelated rows are appended to b (M != N)."""
    g = torch.Generator().manual_seed(seed)
    a = torch.nn.functional.normalize(torch.randn(n, dim, generator=g), dim=1)
    perm = torch.randperm(n, generator=g)
    b = a[perm] + torch.rand(n, 1, generator=g) * noise * torch.randn(n, dim, generator=g)
    k = int(round(replaced * n))
    if k:
        b[:k] = torch.randn(k, dim, generator=g)
    if extra1:
        b = torch.cat([b, torch.randn(extra1, dim, generator=g)])
    return a.contiguous(), torch.nn.functional.normalize(b, dim=1).contiguous()
