"""Shared by the emulator and the GPU tests of the SuperGlue matcher (tests/test_superglue_emu.py, tests/test_superglue_gpu.py).  Every case takes
(lib, device): the emulator build with "cpu", or the gfx950 library with "cuda".

Weights are seeded synthetic ones (weights.synthetic_superglue_state_dict; superglue_{indoor,outdoor}.pth are not in the reference tree).
tests/golden/sg_<case>.npz hold the outputs of the REFERENCE's SuperGlue module on these weights and inputs (scripts/make_superglue_golden.py),
the asserted decision margins, and the distances of the fp32 oracle (tests/superglue_ref.py) from its fp64 evaluation: the yardsticks of the
comparisons.  Image sizes are (H, W), as the reference's wrapper builds image0 / image1.
"""
from __future__ import annotations

import ctypes
import functools
import importlib
import json
import math
import types
from pathlib import Path

import numpy as np
import torch

from tests import golden_cases as gc
from tests import superglue_ref as ref

sg_mod = importlib.import_module("deep-image-matching_amd.superglue_hip")
capi = importlib.import_module("deep-image-matching_amd.capi")
weights_mod = importlib.import_module("deep-image-matching_amd.weights")

HERE = Path(__file__).parent
GOLD = HERE / "golden"
PARITY = HERE.parent / "profiles" / "superglue_parity.json"
TIE_TOL = 1e-4
MIN_MARGIN = 10 * TIE_TOL   # every decision margin of a golden case in fp64 (asserted by the golden script)

# sizes are (H, W).  conf: what the matcher section passes (keys omitted = the network's 100 / 0.2).  gain: final_proj = gain x orthogonal.
# junk: share of image 1's keypoints replaced by unrelated ones (no counterpart in image 0).  bin: bin_score (2 unless given).
GOLDEN_CASES = {
    "zoo": {"seed": 11, "m": 70, "n": 130, "wseed": 3, "gain": 9.0, "size0": (480.0, 640.0), "size1": (618.0, 640.0),
            "conf": {"sinkhorn_iterations": 100, "match_threshold": 0.3}},
    "yaml": {"seed": 12, "m": 150, "n": 110, "wseed": 4, "gain": 9.0, "size0": (768.0, 1024.0), "size1": (1024.0, 768.0),
             "conf": {"sinkhorn_iterations": 20, "match_threshold": 0.3}},
    "odd": {"seed": 14, "m": 33, "n": 97, "wseed": 3, "gain": 9.0, "size0": (480.0, 640.0), "size1": (618.0, 640.0), "conf": {}},
    "wide": {"seed": 19, "m": 300, "n": 257, "wseed": 5, "gain": 12.0, "size0": (480.0, 640.0), "size1": (618.0, 640.0), "conf": {}},
    "dustbin": {"seed": 16, "m": 90, "n": 120, "wseed": 6, "gain": 9.0, "junk": 0.45, "bin": 38.0, "size0": (480.0, 640.0), "size1": (618.0, 640.0), "conf": {}},
}
# GPU only: decisions against the fp32 oracle (no module golden: the case exists for its size)
BIG_CASE = {"seed": 27, "m": 1100, "n": 900, "wseed": 3, "gain": 12.0, "size0": (768.0, 1024.0), "size1": (1024.0, 768.0),
            "conf": {"sinkhorn_iterations": 20, "match_threshold": 0.3}}
NET = {"sinkhorn_iterations": 100, "match_threshold": 0.2}   # SGN:212-219


def conf_of(case) -> dict:
    return {**NET, **case["conf"]}


def case_weights(case, n_layers=18):
    return weights_mod.synthetic_superglue_state_dict(case["wseed"], n_layers=n_layers, final_gain=case.get("gain", 14.0), bin_score=case.get("bin", 2.0))


def case_inputs(case):
    """Two feature dicts {kpts (N, 2), desc (N, 256), scores (N,), size (H, W)}."""
    f0, f1 = gc.lg_inputs({**case, "input_dim": 256})
    g = torch.Generator().manual_seed(7000 + case["seed"])
    f0["scores"], f1["scores"] = torch.rand(case["m"], generator=g), torch.rand(case["n"], generator=g)
    junk = int(round(case.get("junk", 0.0) * case["n"]))
    if junk:   # the last `junk` keypoints of image 1 become unrelated ones
        h1, w1 = case["size1"]
        f1["kpts"][-junk:] = torch.rand(junk, 2, generator=g) * torch.tensor([w1, h1])
        f1["desc"][-junk:] = torch.nn.functional.normalize(torch.randn(junk, 256, generator=g), dim=-1)
    return f0, f1


def data_of(f0, f1):
    """The dict the reference's wrapper hands to the network (matchers/superglue.py): descriptors (1, D, N), image0 / image1 of shape (1, 1, H, W)."""
    img = lambda f: types.SimpleNamespace(shape=(1, 1, int(f["size"][0]), int(f["size"][1])))   # noqa: E731
    return {"keypoints0": f0["kpts"][None], "descriptors0": f0["desc"].T[None], "scores0": f0["scores"][None], "image0": img(f0),
            "keypoints1": f1["kpts"][None], "descriptors1": f1["desc"].T[None], "scores1": f1["scores"][None], "image1": img(f1)}


def oracle(f0, f1, sd, conf, dtype=torch.float32, taps=True):
    return ref.superglue_forward(f0["kpts"], f0["desc"], f0["scores"], f0["size"], f1["kpts"], f1["desc"], f1["scores"], f1["size"], sd,
                                 iters=int(conf["sinkhorn_iterations"]), thr=float(conf["match_threshold"]), dtype=dtype, taps=taps)


def record(label, **res):
    """Measured figures behind an assertion: profiles/superglue_parity.json, one entry per label (rewritten in place)."""
    try:
        data = json.loads(PARITY.read_text()) if PARITY.exists() else {}
        data[label] = {k: (v if isinstance(v, (int, float, str, bool)) else str(v)) for k, v in res.items()}
        PARITY.write_text(json.dumps(data, indent=1, sort_keys=True) + "\n")
    except OSError:
        pass


def cpu(out):
    return {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in out.items()}


def make_net(lib, device, sd, conf=None, max_pairs=1, max_kpts=256, **kw):
    return sg_mod.SuperGlueHIP(sd, conf, max_pairs=max_pairs, max_kpts=max_kpts, device=device, lib=lib, **kw)


def _diff(a, b):
    return (a.double() - b.double()).abs().max().item() if a.numel() else 0.0


def residuals(o32, o64):
    """fp32 oracle against its fp64 evaluation: the yardsticks stored in the goldens."""
    return {"score_res64": max(_diff(o32["matching_scores0"], o64["matching_scores0"]), _diff(o32["matching_scores1"], o64["matching_scores1"])),
            "uv_res64": max(_diff(o32["u"], o64["u"]), _diff(o32["v"], o64["v"])),
            "desc_res64": max(_diff(o32["desc0"], o64["desc0"]), _diff(o32["desc1"], o64["desc1"])),
            "enc_res64": max(_diff(o32["enc0"], o64["enc0"]), _diff(o32["enc1"], o64["enc1"]))}


def decision_margin(o64, thr):
    """The smallest fp64 margin behind any decision: top-2 gaps of the row and of the column of every mutual pair, and every mutual pair's score
    against the threshold."""
    Z = o64["Z"]
    m, n = Z.shape
    ms0 = o64["matching_scores0"]
    rows = torch.nonzero(ms0 > 0)[:, 0]
    margin = float("inf")
    i0 = ref.stable_argmax(Z, 1)
    for i in rows.tolist():
        j = int(i0[i])
        if n > 1:
            margin = min(margin, float(Z[i, j] - torch.cat([Z[i, :j], Z[i, j + 1:]]).max()))
        if m > 1:
            margin = min(margin, float(Z[i, j] - torch.cat([Z[:i, j], Z[i + 1:, j]]).max()))
        margin = min(margin, abs(float(ms0[i]) - thr))
    # rows that are NOT mutual: their own top-2 gap decides nothing unless the runner-up would be mutual; the mutual test itself is covered from
    # the partner's side — a row's argmax j whose column prefers another row by less than the margin would flip: check every row's argmax column
    i1 = ref.stable_argmax(Z, 0)
    for i in range(m):
        j = int(i0[i])
        if int(i1[j]) != i:
            margin = min(margin, float(Z[int(i1[j]), j] - Z[i, j]))
    for j in range(n):
        i = int(i1[j])
        if int(i0[i]) != j:
            margin = min(margin, float(Z[i, int(i0[i])] - Z[i, j]))
    return margin


@functools.lru_cache(maxsize=None)
def _gold(name):
    g = np.load(GOLD / f"sg_{name}.npz")
    out = {k: torch.from_numpy(np.asarray(g[k])) for k in ("matches0", "matches1", "matching_scores0", "matching_scores1", "matches")}
    return out, {k: float(g[k]) for k in ("score_res64", "uv_res64", "desc_res64", "enc_res64", "min_margin")}


@functools.lru_cache(maxsize=None)
def _refs(name):
    """The fp32 oracle and the fp64 evaluation of a golden case: computed once, shared, never modified."""
    case = GOLDEN_CASES[name]
    sd, (f0, f1) = case_weights(case), case_inputs(case)
    return oracle(f0, f1, sd, conf_of(case)), oracle(f0, f1, sd, conf_of(case), torch.float64)


def compare_decisions(out, want, m, n):
    """matches0 / matches1 and the compact list, integer for integer."""
    assert torch.equal(out["matches0"].reshape(-1).long(), want["matches0"].reshape(-1).long()), "matches0"
    assert torch.equal(out["matches1"].reshape(-1).long(), want["matches1"].reshape(-1).long()), "matches1"
    assert out["matches"].dtype == torch.int64 and torch.equal(out["matches"].reshape(-1, 2), want["matches"].reshape(-1, 2).long()), "compact list"
    assert out["matches0"].shape == (1, m) and out["matches1"].shape == (1, n)


# ---- 1 + 2. goldens and the operator taps against fp64 ---------------------------------------------------------------------------------------
def golden(lib, device, name, arithmetic=None):
    """The module's decisions and the oracle's, integer for integer (the golden script asserted every decision margin >= 1e-3); matching scores,
    the encoder output, the final descriptors after 18 layers and u / v after the last iteration within 2 x the fp32 oracle's own distance from the
    fp64 evaluation (the factor the LighterGlue and XFeat tests use for another summation order at the same precision)."""
    case = GOLDEN_CASES[name]
    sd, (f0, f1) = case_weights(case), case_inputs(case)
    m, n = case["m"], case["n"]
    gold, yard = _gold(name)
    ref32, ref64 = _refs(name)
    net = make_net(lib, device, sd, case["conf"], max_kpts=max(m, n), arithmetic=arithmetic)
    assert net.n_layers == 18
    capi.check(lib, lib.dim_saturation_reset(net._stream()))
    out = cpu(net(data_of(f0, f1)))
    tap = net.taps(m, n)
    total, sites = capi.saturation(lib, net._stream(), reset=True)
    assert total == 0, sites
    compare_decisions(out, gold, m, n)
    compare_decisions(out, ref32, m, n)
    score = max(_diff(out["matching_scores0"][0], ref64["matching_scores0"]), _diff(out["matching_scores1"][0], ref64["matching_scores1"]))
    assert torch.equal(out["scores"], out["matching_scores0"][0][out["matches"][:, 0]])
    desc = max(_diff(tap["desc0"], ref64["desc0"]), _diff(tap["desc1"], ref64["desc1"]))
    uv = max(_diff(tap["u"], ref64["u"]), _diff(tap["v"], ref64["v"]))
    capi.check(lib, lib.dim_sg_debug_layers(net._h, 0))
    net(data_of(f0, f1))
    capi.check(lib, lib.dim_sg_debug_layers(net._h, -1))
    t0 = net.taps(m, n)
    enc = max(_diff(t0["desc0"], ref64["enc0"]), _diff(t0["desc1"], ref64["enc1"]))
    tag = f"sg_{name}_{device}" + (f"_{arithmetic}" if arithmetic else "")
    print(f"superglue {name} {device} {arithmetic or ''}: {out['matches'].shape[0]} matches; scores vs fp64 {score:.3e} (fp32 oracle {yard['score_res64']:.3e}), "
          f"encoder {enc:.3e} ({yard['enc_res64']:.3e}), descriptors {desc:.3e} ({yard['desc_res64']:.3e}), u / v {uv:.3e} ({yard['uv_res64']:.3e})")
    record(tag, matches=int(out["matches"].shape[0]), score_diff64=score, score_yardstick=yard["score_res64"], enc_diff64=enc,
           enc_yardstick=yard["enc_res64"], desc_diff64=desc, desc_yardstick=yard["desc_res64"], uv_diff64=uv, uv_yardstick=yard["uv_res64"],
           min_margin=yard["min_margin"])
    assert score <= 2 * yard["score_res64"], (score, yard["score_res64"])
    assert enc <= 2 * yard["enc_res64"], (enc, yard["enc_res64"])
    assert desc <= 2 * yard["desc_res64"], (desc, yard["desc_res64"])
    assert uv <= 2 * yard["uv_res64"], (uv, yard["uv_res64"])
    return out


# ---- 2b + 3. Sinkhorn alone: potentials and marginals ---------------------------------------------------------------------------------------
SINKHORN_SHAPES = [(1, 1), (1, 65), (64, 64), (65, 257), (129, 31)]
SINKHORN_ITERS = [0, 1, 20, 100]


def _tiny_net(lib, device, max_kpts, max_pairs=1, seed=3):
    """A two-layer handle: the stages behind the score product do not look at the network."""
    return make_net(lib, device, weights_mod.synthetic_superglue_state_dict(seed, n_layers=2), max_pairs=max_pairs, max_kpts=max_kpts)


def _to_device(lib, device, addr, t):
    """Host tensor -> the raw buffer of a handle (hipMemcpy host-to-device on the GPU, a plain copy under the emulator)."""
    t = t.contiguous()
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()
        rc = ctypes.CDLL("libamdhip64.so").hipMemcpy(ctypes.c_void_p(addr), ctypes.c_void_p(t.data_ptr()), ctypes.c_size_t(t.numel() * t.element_size()), 1)
        assert rc == 0, rc
    else:
        ctypes.memmove(addr, t.data_ptr(), t.numel() * t.element_size())


def load_scores(net, S):
    """Puts the m x n block S and its counts into the handle, as the score product of a one-pair call would have left them."""
    m, n = S.shape
    d, nk = net._debug(), net.nk
    buf = torch.zeros(max(m, 1), nk)
    buf[:m, :n] = S
    _to_device(net.lib, net.device, d["scores"], buf)
    _to_device(net.lib, net.device, d["n_cur"], torch.tensor([m, n], dtype=torch.int32))
    _to_device(net.lib, net.device, d["done"], torch.tensor([0 if m and n else -1], dtype=torch.int32))


def run_sinkhorn(net, S, iters):
    m, n = S.shape
    load_scores(net, S)
    with net._ctx():
        capi.check(net.lib, net.lib.dim_sg_sinkhorn(net._h, 1, max(m, n), int(iters), net._stream()))
    d, nk = net._debug(), net.nk
    u = capi.copy_from_device(net.lib, d["u"], (nk + 1,), net.device)[:m + 1]
    v = capi.copy_from_device(net.lib, d["v"], (nk + 1,), net.device)[:n + 1]
    return u, v


def _marginal_error(Zc64, u, v, log_nu64):
    """|LSE_i(Z + u + v) - log_nu| over every column, the dustbin included, evaluated in fp64 on the given potentials."""
    return (torch.logsumexp(Zc64 + u.double()[:, None] + v.double()[None, :], dim=0) - log_nu64).abs().max().item()


N_ORDERS = 8   # fp32 torch evaluations behind a yardstick: the input as it is and seven seeded row / column permutations of it


def _fp32_yardsticks(S, alpha, iters, u64, v64, Zc64, log_nu64):
    """The distance of fp32 torch from fp64 on this input, MEASURED: the largest over N_ORDERS evaluations that differ only in the order in which
    torch.logsumexp meets the terms (rows and columns of S permuted, the potentials permuted back).  One evaluation alone is a noisy yardstick:
    whether a potential of magnitude 45 lands on the float below or above its fp64 value (an ulp is 3.8e-6) depends on the summation order, and the
    device's order is none of torch's."""
    m, n = S.shape
    g = torch.Generator().manual_seed(17 + 1000 * m + n)
    pot, marg = 0.0, 0.0
    for k in range(N_ORDERS):
        pr, pc = (torch.arange(m), torch.arange(n)) if k == 0 else (torch.randperm(m, generator=g), torch.randperm(n, generator=g))
        up, vp, *_ = ref.sinkhorn_potentials(S[pr][:, pc].contiguous(), alpha, iters)
        u32, v32 = torch.empty(m + 1), torch.empty(n + 1)
        u32[pr], v32[pc], u32[m], v32[n] = up[:m], vp[:n], up[m], vp[n]
        pot = max(pot, _diff(u32, u64), _diff(v32, v64))
        marg = max(marg, _marginal_error(Zc64, u32, v32, log_nu64))
    return pot, marg


def sinkhorn_alone(lib, device, shapes=SINKHORN_SHAPES, iters_list=SINKHORN_ITERS, label="sinkhorn"):
    """The two passes on a seeded random score block of magnitude up to +-40 (the running maximum matters) against fp64 torch.logsumexp iterations.
    Bound: 2 x the distance of the fp32 torch evaluation of the same input from fp64 (_fp32_yardsticks: measured, the largest over eight summation
    orders), nothing added.  At 0 iterations u = v = 0 exactly.  After the last column pass the column marginals of exp(Z + u + v) are log_nu on
    every column including the dustbin: bound measured the same way on the fp32 torch potentials."""
    net = _tiny_net(lib, device, max(max(s) for s in shapes))
    alpha = float(weights_mod.synthetic_superglue_state_dict(3, n_layers=2)["bin_score"])
    worst = {}
    for (m, n) in shapes:
        g = torch.Generator().manual_seed(100 * m + n)
        S = (torch.rand(m, n, generator=g) * 2 - 1) * 40.0
        for iters in iters_list:
            u, v = run_sinkhorn(net, S, iters)
            if iters == 0:
                assert float(u.abs().max()) == 0.0 and float(v.abs().max()) == 0.0
                continue
            u64, v64, _, Zc64, _, log_nu64 = ref.sinkhorn_potentials(S.double(), alpha, iters)
            yard, marg_yard = _fp32_yardsticks(S, alpha, iters, u64, v64, Zc64, log_nu64)
            got = max(_diff(u, u64), _diff(v, v64))
            marg = _marginal_error(Zc64, u, v, log_nu64)
            print(f"{label} {device} {m}x{n} iters {iters}: u / v vs fp64 {got:.3e} (fp32 torch {yard:.3e}); column marginals {marg:.3e} (fp32 torch {marg_yard:.3e})")
            worst[f"{m}x{n}_{iters}"] = f"{got:.3e}/{yard:.3e} marg {marg:.3e}/{marg_yard:.3e}"
            assert got <= 2 * yard, (m, n, iters, got, yard)
            assert marg <= 2 * marg_yard, (m, n, iters, marg, marg_yard)
    record(f"{label}_{device}", **worst)


# ---- 4. edge counts --------------------------------------------------------------------------------------------------------------------------
def _pair(seed, m, n, size=((480.0, 640.0), (618.0, 640.0))):
    return case_inputs({"seed": seed, "m": max(m, 1), "n": max(n, 1), "size0": size[0], "size1": size[1]})


def _cut(f, k):
    return {"kpts": f["kpts"][:k].contiguous(), "desc": f["desc"][:k].contiguous(), "scores": f["scores"][:k].contiguous(), "size": f["size"]}


def _check(net, f0, f1, sd, conf):
    """Against the fp32 oracle on the same inputs, every decision equal: the pairs are chosen so that the oracle's fp64 margins are at least 1e-3
    (asserted here, as the golden script does for the goldens); scores within 1e-4."""
    out = cpu(net(data_of(f0, f1)))
    want = oracle(f0, f1, sd, conf)
    m, n = f0["kpts"].shape[0], f1["kpts"].shape[0]
    assert out["matches0"].shape == (1, m) and out["matches1"].shape == (1, n) and out["matches"].dtype == torch.int64
    if m and n:
        thr = float(conf["match_threshold"])
        # (threshold 0: exp(.) > 0 always holds, the threshold decides nothing; 0.999999: every score is below it by construction of the case)
        assert decision_margin(oracle(f0, f1, sd, conf, torch.float64), thr if 0.0 < thr < 0.9 else -1.0) >= MIN_MARGIN, (m, n)
    assert torch.equal(out["matches0"][0], want["matches0"]) and torch.equal(out["matches1"][0], want["matches1"])
    assert _diff(out["matching_scores0"][0], want["matching_scores0"]) <= 1e-4 and _diff(out["matching_scores1"][0], want["matching_scores1"]) <= 1e-4
    assert torch.equal(out["matches"], want["matches"])
    return out


def edge_counts(lib, device):
    """An empty side (both ways, and both), 1 x 1, 1 x n, a pair at exactly max_kpts, thresholds 0 and 0.999999, and all-equal scores (the lowest
    index wins, as in the library's other argmax kernels) — on ONE handle."""
    sd = weights_mod.synthetic_superglue_state_dict(3, n_layers=4, final_gain=12.0)
    net = make_net(lib, device, sd, max_kpts=96)
    f0, f1 = _pair(23, 96, 96)   # (seed and gain: every pair below decides with fp64 margins >= 1e-2)
    for m, n in ((0, 40), (40, 0), (0, 0)):
        out = _check(net, _cut(f0, m), _cut(f1, n), sd, NET)
        assert out["matches"].shape == (0, 2) and bool((out["matches0"] == -1).all()) and bool((out["matches1"] == -1).all())
        assert float(out["matching_scores0"].abs().sum()) == 0.0 and float(out["matching_scores1"].abs().sum()) == 0.0
    for m, n in ((1, 1), (1, 40), (96, 96), (33, 31)):
        out = _check(net, _cut(f0, m), _cut(f1, n), sd, NET)
    assert out["matches"].shape[0] > 5
    net.conf["match_threshold"] = 0.0
    loose = _check(net, _cut(f0, 64), _cut(f1, 96), sd, {**NET, "match_threshold": 0.0})
    mutual = int((loose["matching_scores0"] > 0).sum())
    assert loose["matches"].shape[0] == mutual > 5
    net.conf["match_threshold"] = 0.999999
    strict = _check(net, _cut(f0, 64), _cut(f1, 96), sd, {**NET, "match_threshold": 0.999999})
    assert strict["matches"].shape[0] == 0 and torch.equal(strict["matching_scores0"], loose["matching_scores0"])
    # all-equal scores at 0 iterations: Z is constant over the real block, every argmax is index 0, (0, 0) is the one mutual pair
    for (m, n) in ((5, 7), (70, 33)):
        S = torch.full((m, n), 0.25)
        load_scores(net, S)
        NK = net.nk
        o = {"matches": torch.zeros(1, NK, 2, dtype=torch.int64, device=device), "scores": torch.zeros(1, NK, device=device),
             "n": torch.zeros(1, dtype=torch.int32, device=device), "m01": torch.zeros(1, 2, NK, dtype=torch.int32, device=device),
             "s01": torch.zeros(1, 2, NK, device=device)}
        with net._ctx():
            capi.check(lib, lib.dim_sg_sinkhorn(net._h, 1, max(m, n), 0, net._stream()))
            capi.check(lib, lib.dim_sg_select(net._h, 1, max(m, n), 0.0, capi.ptr(o["matches"]), capi.ptr(o["scores"]), capi.ptr(o["n"]), capi.ptr(o["m01"]),
                                              capi.ptr(o["s01"]), net._stream()))
        z = torch.zeros(max(m, n) + 1)
        norm = -torch.tensor(float(m + n)).log()
        m0, m1, ms0, ms1, _ = ref.select(S, z[:m + 1], z[:n + 1], norm, 0.0)
        assert m0.tolist() == [0] + [-1] * (m - 1) and m1.tolist() == [0] + [-1] * (n - 1)
        assert torch.equal(o["m01"][0, 0, :m].cpu().long(), m0) and torch.equal(o["m01"][0, 1, :n].cpu().long(), m1)
        assert int(o["n"][0]) == 1 and o["matches"][0, 0].tolist() == [0, 0]
        assert _diff(o["s01"][0, 0, :m].cpu(), ms0) <= 1e-5 * float(ms0.max()) and _diff(o["s01"][0, 1, :n].cpu(), ms1) <= 1e-5 * float(ms0.max())


# ---- 5. batch = singles, reused handle ------------------------------------------------------------------------------------------------------
def batch_equals_singles(lib, device):
    """16 pairs of mixed sizes in one call against 16 single calls: matches and scores bit for bit.  One pair is 520 x 513 (five query blocks x 4 heads
    x 32 items = 640 attention workgroups, the largest launch shape), one is 40 x 33, one has an empty side.  A SuperGlue handle never cuts the key
    range of the attention (sg_api.hip), the GEMM blocks accumulate along K in one order whatever block shape a launch picks, and the Sinkhorn /
    selection reductions depend on (m, n) alone.  Single calls run on a fresh handle and on a handle that has just run a larger pair."""
    sd = weights_mod.synthetic_superglue_state_dict(3, n_layers=2, final_gain=9.0)   # one self and one cross layer
    g = torch.Generator().manual_seed(5)
    counts = [520, 513, 40, 33, 300, 257, 0, 129, 64, 96, 1, 200]
    cap, n_img = 520, len(counts)
    base0, _ = _pair(22, cap, cap)
    kt, dt, sc = torch.zeros(n_img, cap, 2), torch.zeros(n_img, cap, 256), torch.zeros(n_img, cap)
    for i in range(n_img):   # every image: image 0's keypoints in the same order, perturbed, so that row k of any two images corresponds
        kt[i] = base0["kpts"] + torch.randn(cap, 2, generator=g)
        dt[i] = torch.nn.functional.normalize(base0["desc"] + 0.02 * torch.randn(cap, 256, generator=g), dim=-1)
        sc[i] = torch.rand(cap, generator=g)
    nt = torch.tensor(counts, dtype=torch.int32)
    hw = [(480.0, 640.0), (618.0, 640.0)]
    st = torch.tensor([[hw[i % 2][1], hw[i % 2][0]] for i in range(n_img)])   # (W, H)
    pairs = torch.tensor([[0, 1], [2, 3], [4, 5], [6, 7], [8, 9], [10, 11], [1, 0], [3, 2], [5, 4], [2, 5], [9, 8], [11, 4], [7, 8], [3, 10], [0, 5], [4, 1]],
                         dtype=torch.int32)
    conf = {"sinkhorn_iterations": 10, "match_threshold": 0.2}
    net = make_net(lib, device, sd, conf, max_pairs=16, max_kpts=cap)
    to = lambda t: t.to(device)   # noqa: E731
    o = cpu(net.match_batch_guarded(to(kt), to(dt), to(sc), to(nt), to(st), pair_idx=to(pairs)))
    fresh = make_net(lib, device, sd, conf, max_pairs=1, max_kpts=cap)
    used = make_net(lib, device, sd, conf, max_pairs=1, max_kpts=cap)

    def one(net_, a, b):
        f = lambda i: {"kpts": kt[i, :counts[i]], "desc": dt[i, :counts[i]], "scores": sc[i, :counts[i]], "size": torch.tensor(hw[i % 2])}   # noqa: E731
        return cpu(net_(data_of(f(a), f(b))))

    total = 0
    for p, (a, b) in enumerate(pairs.tolist()):
        if p in (1, 3, 9):   # the largest pair first (40 x 33, the empty side and a mid-sized pair follow it): nothing of it may reach the next call
            one(used, 0, 1)
        S = int(o["n_matches"][p])
        total += S
        for r in (one(fresh, a, b), one(used, a, b)):
            assert torch.equal(o["matches"][p, :S], r["matches"]), (p, a, b)
            assert torch.equal(o["matches01"][p, 0, :counts[a]].long(), r["matches0"][0]) and torch.equal(o["matches01"][p, 1, :counts[b]].long(), r["matches1"][0])
            assert torch.equal(o["scores"][p, :S], r["scores"]), (p, a, b)
            assert torch.equal(o["mscores01"][p, 0, :counts[a]], r["matching_scores0"][0]) and torch.equal(o["mscores01"][p, 1, :counts[b]], r["matching_scores1"][0])
        if counts[a] == 0 or counts[b] == 0:
            assert S == 0
    assert total > 500, total


# ---- 6. range guard -------------------------------------------------------------------------------------------------------------------------
def guard(lib, device):
    """Layer 15's value projection times 2^14 in one output channel (module channel 29) and the consuming column of merge times 2^-14: the real
    arithmetic is unchanged (powers of two), the stored V leaves +-4094 in a late layer.  The counter fires under fp16x3, and the guarded re-run
    (bf16x6) gives the golden's decisions and scores within the golden's bound."""
    assert capi.get_arithmetic(lib) == 2
    case = GOLDEN_CASES["zoo"]
    sd, (f0, f1) = {k: v.clone() for k, v in case_weights(case).items()}, case_inputs(case)
    s = 2.0 ** 14
    sd["gnn.layers.15.attn.proj.2.weight"][29] *= s
    sd["gnn.layers.15.attn.proj.2.bias"][29] *= s
    sd["gnn.layers.15.attn.merge.weight"][:, 29] /= s
    m, n = case["m"], case["n"]
    net = make_net(lib, device, sd, case["conf"], max_kpts=max(m, n))
    d = data_of(f0, f1)
    capi.check(lib, lib.dim_saturation_reset(net._stream()))
    policy, net.on_saturation = net.on_saturation, "off"
    net(d)
    net.on_saturation = policy
    total, sites = capi.saturation(lib, net._stream(), reset=True)
    assert total > 0 and "lg_qkv" in sites, (total, sites)
    out = cpu(net(d))   # guarded: repeats the call in bf16x6
    gold, yard = _gold("zoo")
    _, ref64 = _refs("zoo")
    compare_decisions(out, gold, m, n)
    score = _diff(out["matching_scores0"][0], ref64["matching_scores0"])
    assert score <= 2 * yard["score_res64"], (score, yard["score_res64"])


# ---- 7. head permutation and BatchNorm fold (host only) ---------------------------------------------------------------------------------------
def folded_forward(prep, n_layers, d0, d1):
    """The network as the DEVICE sees it, in fp64 on prepare_superglue_weights' output: head-major channels (c = h * 64 + d), no BatchNorm."""
    P = {k: v.double() for k, v in prep.items()}
    heads = lambda y: y.reshape(y.shape[0], 4, 64).permute(1, 0, 2)   # noqa: E731
    for i in range(n_layers):
        s0, s1 = (d1, d0) if i % 2 else (d0, d1)
        new = []
        for x, src in ((d0, s0), (d1, s1)):
            q, k, v = heads(x @ P[f"{i}.q_w"].T + P[f"{i}.q_b"]), heads(src @ P[f"{i}.k_w"].T + P[f"{i}.k_b"]), heads(src @ P[f"{i}.v_w"].T + P[f"{i}.v_b"])
            msg = (torch.softmax(q @ k.transpose(1, 2) / 8.0, dim=-1) @ v).permute(1, 0, 2).reshape(x.shape[0], 256)
            msg = msg @ P[f"{i}.merge_w"].T + P[f"{i}.merge_b"]
            hid = torch.relu(torch.cat([x, msg], 1) @ P[f"{i}.mlp0_w"].T + P[f"{i}.mlp0_b"])
            new.append(x + hid @ P[f"{i}.mlp3_w"].T + P[f"{i}.mlp3_b"])
        d0, d1 = new
    return d0, d1


def folded_encoder(prep, x):
    P = {k: v.double() for k, v in prep.items()}
    for s in range(5):
        x = x @ P[f"kenc.{s}.w"].T + P[f"kenc.{s}.b"]
        if s < 4:
            x = torch.relu(x)
    return x


# ---- 8. ABI ---------------------------------------------------------------------------------------------------------------------------------
def abi(lib, device):
    sd = weights_mod.synthetic_superglue_state_dict(3, n_layers=2)
    odd = {k: v for k, v in weights_mod.synthetic_superglue_state_dict(3, n_layers=4).items() if not k.startswith("gnn.layers.3.")}
    for bad_sd, conf, word in ((odd, None, "n_layers 3"), ({k: v for k, v in sd.items() if not k.startswith("gnn.")}, None, "n_layers 0"),
                               (sd, {"descriptor_dim": 128}, "descriptor_dim 128")):
        try:
            make_net(lib, device, bad_sd, conf, max_kpts=64)
        except capi.DimHipError as e:
            assert word in str(e), str(e)
        else:
            raise AssertionError(f"dim_sg_create accepted {word}")
    net = make_net(lib, device, sd, max_kpts=62)
    assert net.nk == 64 and net.n_layers == 2
    f0, f1 = _pair(29, 40, 33)
    try:
        net.match_batch_guarded(*[t.to(device) for t in (torch.zeros(2, 40, 2), torch.zeros(2, 40, 256), torch.zeros(2, 40), torch.tensor([40, 33], dtype=torch.int32),
                                                         torch.ones(2, 2))], n_pairs=1, sinkhorn_iterations=-1)
    except capi.DimHipError as e:
        assert "sinkhorn_iterations -1" in str(e), str(e)
    else:
        raise AssertionError("a negative iteration count was accepted")
    try:
        net.match_batch(*[t.to(device) for t in (torch.zeros(4, 40, 2), torch.zeros(4, 40, 256), torch.zeros(4, 40), torch.tensor([4] * 4, dtype=torch.int32),
                                                 torch.ones(4, 2))], n_pairs=2)
    except capi.DimHipError as e:
        assert "n_pairs 2" in str(e), str(e)
    else:
        raise AssertionError("more pairs than the handle holds were accepted")
    # create / destroy give the device memory back: ten handles of ~70 MB each, one alive at a time (the emulator has no device memory to ask about:
    # there the ten rounds check only that create / destroy run)
    free0 = torch.cuda.mem_get_info()[0] if torch.device(device).type == "cuda" else None
    for _ in range(10):
        h = make_net(lib, device, sd, max_kpts=2048)
        assert h.nk == 2048
        del h
    if free0 is not None:
        torch.cuda.synchronize()
        assert free0 - torch.cuda.mem_get_info()[0] < 32 << 20
    out = cpu(net(data_of(f0, f1)))
    assert out["matches0"].shape == (1, 40)


# ---- 10. GPU only ---------------------------------------------------------------------------------------------------------------------------
def big_pair_against_fp32_oracle(lib, device):
    """1100 x 900 (nine query blocks, ragged key tiles, several Sinkhorn column tiles per row group): decisions equal to the fp32 oracle's — the case's
    fp64 margins are >= 1e-3 (asserted here on the fp64 evaluation, as the golden script does for the module goldens)."""
    case = BIG_CASE
    sd, (f0, f1) = case_weights(case), case_inputs(case)
    conf = conf_of(case)
    o32, o64 = oracle(f0, f1, sd, conf), oracle(f0, f1, sd, conf, torch.float64)
    assert torch.equal(o32["matches0"], o64["matches0"]) and decision_margin(o64, conf["match_threshold"]) >= MIN_MARGIN
    net = make_net(lib, device, sd, case["conf"], max_kpts=1100)
    out = cpu(net(data_of(f0, f1)))
    compare_decisions(out, o32, case["m"], case["n"])
    score = _diff(out["matching_scores0"][0], o64["matching_scores0"])
    yard = residuals(o32, o64)["score_res64"]
    print(f"superglue 1100x900 {device}: {out['matches'].shape[0]} matches, scores vs fp64 {score:.3e} (fp32 oracle {yard:.3e})")
    record(f"sg_big_{device}", matches=int(out["matches"].shape[0]), score_diff64=score, score_yardstick=yard)
    assert out["matches"].shape[0] > 300 and score <= 2 * yard


def shipped_yaml_size(lib, device):
    """One pair at 8000 x 8000 keypoints, 20 iterations (config/superpoint+superglue.yaml's count): no CPU oracle.  The column marginals of
    exp(Z + u + v) are log_nu on every column including the dustbin (fp64 torch on the device, from the handle's S, u, v; bound: 2 x the same figure for
    the last column pass redone in fp32 torch on the device's u), matches0 / matches1 are mutually consistent, and the range guard stays silent."""
    m = n = 8000
    case = {"seed": 33, "m": m, "n": n, "size0": (3000.0, 4000.0), "size1": (3000.0, 4000.0)}
    f0, f1 = case_inputs(case)
    sd = weights_mod.synthetic_superglue_state_dict(3, final_gain=12.0)
    net = make_net(lib, device, sd, {"sinkhorn_iterations": 20, "match_threshold": 0.3}, max_kpts=8000)
    capi.check(lib, lib.dim_saturation_reset(net._stream()))
    policy, net.on_saturation = net.on_saturation, "off"
    out = net(data_of(f0, f1))
    net.on_saturation = policy
    total, sites = capi.saturation(lib, net._stream(), reset=True)
    assert total == 0, sites
    m0, m1 = out["matches0"][0], out["matches1"][0]
    idx = torch.nonzero(m0 > -1)[:, 0]
    assert idx.numel() > 2000 and torch.equal(m1[m0[idx]], idx)
    jdx = torch.nonzero(m1 > -1)[:, 0]
    assert jdx.numel() == idx.numel() and torch.equal(m0[m1[jdx]], jdx)
    assert torch.equal(out["matches"][:, 0], idx) and torch.equal(out["matches"][:, 1], m0[idx])
    # marginals on the device in fp64 from the handle's own buffers
    d, nk = net._debug(), net.nk
    alpha = float(sd["bin_score"])
    S = torch.empty(nk * nk, dtype=torch.float32, device=device)
    u = torch.empty(nk + 1, dtype=torch.float32, device=device)
    v = torch.empty(nk + 1, dtype=torch.float32, device=device)
    hip = ctypes.CDLL("libamdhip64.so")
    torch.cuda.synchronize()
    for dst, src in ((S, d["scores"]), (u, d["u"]), (v, d["v"])):
        assert hip.hipMemcpy(ctypes.c_void_p(dst.data_ptr()), ctypes.c_void_p(src), ctypes.c_size_t(dst.numel() * 4), 3) == 0
    S = S.reshape(nk, nk)[:m, :n]
    norm = -torch.log(torch.tensor(float(m + n), dtype=torch.float64))
    log_nu = torch.cat([norm.expand(n), (torch.log(torch.tensor(float(m), dtype=torch.float64)) + norm)[None]]).to(device)
    worst, yard = 0.0, 0.0
    ud, vd = u[:m + 1].double(), v[:n + 1].double()
    u32 = u[:m + 1]
    for j0 in range(0, n + 1, 1024):   # column slabs: the fp64 coupling matrix is never whole in memory
        j1 = min(n + 1, j0 + 1024)
        Z = torch.full((m + 1, j1 - j0), alpha, dtype=torch.float64, device=device)
        jr = min(j1, n)
        if jr > j0:
            Z[:m, :jr - j0] = S[:, j0:jr].double()
        lse = torch.logsumexp(Z + ud[:, None] + vd[None, j0:j1], dim=0)
        worst = max(worst, float((lse - log_nu[j0:j1]).abs().max()))
        # the yardstick, measured: the same last column pass in fp32 torch on the device's u, and ITS marginals in fp64
        v32 = log_nu[j0:j1].float() - torch.logsumexp(Z.float() + u32[:, None], dim=0)
        yard = max(yard, float((torch.logsumexp(Z + ud[:, None] + v32.double()[None, :], dim=0) - log_nu[j0:j1]).abs().max()))
    bound = 2 * yard
    print(f"superglue 8000x8000 {device}: {idx.numel()} matches, column marginals off by {worst:.3e} (fp32 torch {yard:.3e})")
    record(f"sg_8000_{device}", matches=int(idx.numel()), marginal_error=worst, fp32_torch=yard)
    assert worst <= bound, (worst, bound)
