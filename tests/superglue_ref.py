"""Functional torch-CPU oracle of the SuperGlue network (reference thirdparty/SuperGluePretrainedNetwork/models/superglue.py, SGN), written from
its behaviour: plain tensor algebra on the module's state dict — unfolded BatchNorm, the module's interleaved head layout — in fp32 or fp64, with
taps after the encoder, after every layer, on the scores and on the Sinkhorn potentials.  Rows are keypoints ((N, C) matrices), not channels.
"""
from __future__ import annotations

import math

import torch

BN_EPS = 1e-5


def _lin(sd, name, x):
    w = sd[name + ".weight"]
    return x @ w.reshape(w.shape[0], w.shape[1]).T + sd[name + ".bias"]


def _bn(sd, name, x):
    return (x - sd[name + ".running_mean"]) / torch.sqrt(sd[name + ".running_var"] + BN_EPS) * sd[name + ".weight"] + sd[name + ".bias"]


def normalize_keypoints(kpts, height, width):
    """SGN:64-71: centre at size / 2, scale by 0.7 x the longer side."""
    size = torch.tensor([float(width), float(height)], dtype=kpts.dtype)
    return (kpts - size / 2) / (size.max() * 0.7)


def keypoint_encoder(sd, kpts_n, scores):
    x = torch.cat([kpts_n, scores[:, None]], dim=1)
    for s in range(4):
        x = torch.relu(_bn(sd, f"kenc.encoder.{3 * s + 1}", _lin(sd, f"kenc.encoder.{3 * s}", x)))
    return _lin(sd, "kenc.encoder.12", x)


def propagation(sd, i, x, src):
    """One AttentionalPropagation (SGN:96-128): the residual delta for x attending to src."""
    t = f"gnn.layers.{i}."
    heads = lambda y: y.reshape(y.shape[0], 64, 4).permute(2, 0, 1)   # channel c = d * 4 + h -> [h][n][d]
    q, k, v = heads(_lin(sd, t + "attn.proj.0", x)), heads(_lin(sd, t + "attn.proj.1", src)), heads(_lin(sd, t + "attn.proj.2", src))
    prob = torch.softmax(q @ k.transpose(1, 2) / 8.0, dim=-1)
    msg = (prob @ v).permute(1, 2, 0).reshape(x.shape[0], 256)
    msg = _lin(sd, t + "attn.merge", msg)
    hid = torch.relu(_bn(sd, t + "mlp.1", _lin(sd, t + "mlp.0", torch.cat([x, msg], dim=1))))
    return _lin(sd, t + "mlp.3", hid)


def sinkhorn_potentials(scores, alpha, iters):
    """SGN:152-186 on the (m+1) x (n+1) couplings: returns (u [m+1], v [n+1], norm); Z = couplings + u[:, None] + v[None] - norm."""
    m, n = scores.shape
    dt = scores.dtype
    a = torch.as_tensor(alpha, dtype=dt)
    Z = torch.cat([torch.cat([scores, a.expand(m, 1)], 1), torch.cat([a.expand(1, n), a.expand(1, 1)], 1)], 0)
    norm = -torch.tensor(float(m + n), dtype=dt).log()
    log_mu = torch.cat([norm.expand(m), torch.tensor(float(n), dtype=dt).log()[None] + norm])
    log_nu = torch.cat([norm.expand(n), torch.tensor(float(m), dtype=dt).log()[None] + norm])
    u, v = torch.zeros(m + 1, dtype=dt), torch.zeros(n + 1, dtype=dt)
    for _ in range(iters):
        u = log_mu - torch.logsumexp(Z + v[None, :], dim=1)
        v = log_nu - torch.logsumexp(Z + u[:, None], dim=0)
    return u, v, norm, Z, log_mu, log_nu


def stable_argmax(x, dim):
    """Lowest index among equal maxima (the device rule)."""
    mx = x.max(dim=dim, keepdim=True).values
    idx = torch.arange(x.shape[dim]).reshape([-1 if d == dim else 1 for d in range(x.dim())])
    return torch.where(x == mx, idx, torch.full_like(idx, x.shape[dim])).min(dim=dim).values


def select(scores, u, v, norm, thr):
    """SGN:288-305 on Z = scores + u + v - norm over the real block."""
    m, n = scores.shape
    Z = (scores + u[:m, None]) + v[None, :n] - norm
    i0, i1 = stable_argmax(Z, 1), stable_argmax(Z, 0)
    max0 = Z.gather(1, i0[:, None])[:, 0]
    mutual0 = torch.arange(m) == i1[i0]
    mutual1 = torch.arange(n) == i0[i1]
    ms0 = torch.where(mutual0, max0.exp(), torch.zeros((), dtype=Z.dtype))
    ms1 = torch.where(mutual1, ms0[i1], torch.zeros((), dtype=Z.dtype))
    valid0 = mutual0 & (ms0 > torch.tensor(thr, dtype=Z.dtype))
    valid1 = mutual1 & valid0[i1]
    m0 = torch.where(valid0, i0, torch.full_like(i0, -1))
    m1 = torch.where(valid1, i1, torch.full_like(i1, -1))
    return m0, m1, ms0, ms1, Z


def superglue_forward(kpts0, desc0, scores0, size0, kpts1, desc1, scores1, size1, sd, iters=100, thr=0.2, dtype=torch.float32, taps=True):
    """kpts (N, 2), desc (N, 256), scores (N,), size = (H, W) as the wrapper's image0 / image1 shapes carry it.  Returns matches0 / matches1 (int64,
    -1 = none), matching_scores0 / 1, the compact (S, 2) list and, with taps, enc0/1, layers [(d0, d1)], scores, u, v."""
    c = lambda t: t.detach().to(dtype)
    sd = {k: (c(v) if v.is_floating_point() else v) for k, v in sd.items()}
    kpts0, desc0, scores0, kpts1, desc1, scores1 = map(c, (kpts0, desc0, scores0, kpts1, desc1, scores1))
    m, n = kpts0.shape[0], kpts1.shape[0]
    if m == 0 or n == 0:   # SGN:255-262
        out = {"matches0": torch.full((m,), -1, dtype=torch.int64), "matches1": torch.full((n,), -1, dtype=torch.int64),
               "matching_scores0": torch.zeros(m, dtype=dtype), "matching_scores1": torch.zeros(n, dtype=dtype)}
        out["matches"] = torch.zeros(0, 2, dtype=torch.int64)
        return out
    n_layers = max(int(k.split(".")[2]) for k in sd if k.startswith("gnn.layers.")) + 1
    e0 = keypoint_encoder(sd, normalize_keypoints(kpts0, float(size0[0]), float(size0[1])), scores0)
    e1 = keypoint_encoder(sd, normalize_keypoints(kpts1, float(size1[0]), float(size1[1])), scores1)
    d0, d1 = desc0 + e0, desc1 + e1
    tap = {"enc0": d0, "enc1": d1, "layers": []}
    for i in range(n_layers):
        s0, s1 = (d1, d0) if i % 2 else (d0, d1)
        delta0, delta1 = propagation(sd, i, d0, s0), propagation(sd, i, d1, s1)
        d0, d1 = d0 + delta0, d1 + delta1
        if taps:
            tap["layers"].append((d0, d1))
    md0, md1 = _lin(sd, "final_proj", d0), _lin(sd, "final_proj", d1)
    scores = md0 @ md1.T / math.sqrt(256.0)
    u, v, norm, Zc, _, _ = sinkhorn_potentials(scores, sd["bin_score"], iters)
    m0, m1, ms0, ms1, Z = select(scores, u, v, norm, thr)
    keep = m0 > -1
    out = {"matches0": m0, "matches1": m1, "matching_scores0": ms0, "matching_scores1": ms1,
           "matches": torch.stack([torch.arange(m)[keep], m0[keep]], dim=1)}
    if taps:
        out.update(tap)
        out.update({"desc0": d0, "desc1": d1, "scores": scores, "u": u, "v": v, "Z": Z, "norm": norm})
    return out
