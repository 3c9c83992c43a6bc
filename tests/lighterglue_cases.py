"""Shared by the emulator and the GPU tests of the LighterGlue matcher (tests/test_lighterglue_emu.py, tests/test_lighterglue_gpu.py).  Every case
takes (lib, device): the emulator build with "cpu", or the gfx950 library with "cuda".

Weights are seeded synthetic ones at LighterGlue's shape (weights.synthetic_lighterglue_state_dict; the trained xfeat-lighterglue.pt is not in the
reference tree).  tests/golden/lgl_<case>.npz hold the outputs of the REFERENCE's vendored LightGlue module built at LighterGlue's configuration
(scripts/make_lighterglue_golden.py: kornia's class, which the reference's LighterGlue wraps, is a copy of it and kornia is not installed), the
asserted decision margins, and the residual of the fp64 log-assignment against the fp32 one: the yardstick of the dense comparison.
Image sizes are fed as the reference's matcher feeds them: (W, H).
"""
from __future__ import annotations

import ctypes
import functools
import importlib
import json
from pathlib import Path

import numpy as np
import torch

from oracle import lightglue_ref
from tests import golden_cases as gc
from tests.parity import compare_lightglue

lgl_mod = importlib.import_module("deep-image-matching_amd.lighterglue_hip")
lg_mod = importlib.import_module("deep-image-matching_amd.lightglue_hip")
capi = importlib.import_module("deep-image-matching_amd.capi")
weights_mod = importlib.import_module("deep-image-matching_amd.weights")

HERE = Path(__file__).parent
GOLD = HERE / "golden"
PARITY = HERE.parent / "profiles" / "lighterglue_parity.json"
TIE_TOL = 1e-4            # compare_lightglue's near-tie bar; the goldens assert every decision margin >= 10 x this
MIN_MARGIN = 10 * TIE_TOL
PRUNE_BAR = 1 - 0.95      # matchability above this keeps a keypoint (width_confidence 0.95, LGN:586-591)
NET = {"n_layers": 6, "num_heads": 1, "depth_confidence": -1, "width_confidence": 0.95, "filter_threshold": 0.1}   # modules/lighterglue.py:12-27

# sizes are (H, W) as features.h5 holds them; lg_inputs draws keypoints inside them.  mw / mb: the matchability rows are replaced by
# randn(1, 96) * mw with bias mb (pruning becomes real); otherwise the matching weights' "matchable" heads (bias 5) keep every keypoint.
GOLDEN_CASES = {
    "fixed": {"seed": 11, "m": 70, "n": 130, "wseed": 3, "size0": (480.0, 640.0), "size1": (618.0, 640.0), "conf": {"width_confidence": -1}},
    "prune": {"seed": 12, "m": 150, "n": 110, "wseed": 6, "mw": 3.5, "mb": 2.5, "size0": (768.0, 1024.0), "size1": (1024.0, 768.0), "conf": {}},
    "odd": {"seed": 14, "m": 33, "n": 97, "wseed": 3, "size0": (480.0, 640.0), "size1": (618.0, 640.0), "conf": {}},
    "prune_to_empty": {"seed": 12, "m": 150, "n": 110, "wseed": 5, "mw": 3.5, "mb": -14.0, "size0": (768.0, 1024.0), "size1": (1024.0, 768.0), "conf": {}},
    "wide": {"seed": 19, "m": 300, "n": 257, "wseed": 4, "size0": (480.0, 640.0), "size1": (618.0, 640.0), "conf": {}},
}


def conf_of(case) -> dict:
    return {**NET, **case["conf"]}


def case_weights(case):
    sd = weights_mod.synthetic_lighterglue_state_dict(case["wseed"])
    if "mw" in case:
        g = torch.Generator().manual_seed(1000 + case["wseed"])
        for i in range(NET["n_layers"]):
            sd[f"log_assignment.{i}.matchability.weight"] = torch.randn(1, 96, generator=g) * case["mw"]
            sd[f"log_assignment.{i}.matchability.bias"] = torch.full((1,), float(case["mb"]))
    return sd


def case_inputs(case):
    """Two feature dicts {kpts, desc (N, 64), size}: size is (W, H), what the network is fed."""
    f0, f1 = gc.lg_inputs({**case, "input_dim": 64})
    for f in (f0, f1):
        f["size"] = f["size"].flip(0).contiguous()
    return f0, f1


def data_of(f0, f1):
    return {"image0": {"keypoints": f0["kpts"][None], "descriptors": f0["desc"][None], "image_size": f0["size"][None]},
            "image1": {"keypoints": f1["kpts"][None], "descriptors": f1["desc"][None], "image_size": f1["size"][None]}}


def oracle(f0, f1, sd, conf, dtype=torch.float32, taps=True):
    c = dict(conf)
    if dtype == torch.float64:
        sd = {k: v.double() for k, v in sd.items()}
        c["dtype"] = torch.float64
    return lightglue_ref.lightglue_forward(f0["kpts"], f0["desc"], f0["size"], f1["kpts"], f1["desc"], f1["size"], sd, c, taps=taps)


def record(label, **res):
    """Measured figures behind an assertion: profiles/lighterglue_parity.json, one entry per label (rewritten in place)."""
    try:
        data = json.loads(PARITY.read_text()) if PARITY.exists() else {}
        data[label] = {k: (v if isinstance(v, (int, float, str, bool)) else str(v)) for k, v in res.items()}
        PARITY.write_text(json.dumps(data, indent=1, sort_keys=True) + "\n")
    except OSError:
        pass


def cpu(out):
    return {k: ([t.cpu() for t in v] if isinstance(v, list) else (v.cpu() if torch.is_tensor(v) else v)) for k, v in out.items()}


def make_net(lib, device, sd, conf=None, max_pairs=1, max_kpts=256, **kw):
    return lgl_mod.LighterGlueHIP(sd, conf, max_pairs=max_pairs, max_kpts=max_kpts, device=device, lib=lib, **kw)


def final_desc(net):
    """dim_lg_debug_desc after a one-pair call: the live rows of the final descriptors ([n_cur0, 96], [n_cur1, 96]) and their original indices."""
    lib = net.lib
    d, nc, ind = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    capi.check(lib, lib.dim_lg_debug_desc(net._h, ctypes.byref(d), ctypes.byref(nc), ctypes.byref(ind)))
    nk = net.nk
    desc = capi.copy_from_device(lib, d.value, (2, nk, net.descriptor_dim), net.device)
    cnt = capi.copy_from_device(lib, nc.value, (2,), net.device).view(torch.int32)
    idx = capi.copy_from_device(lib, ind.value, (2, nk), net.device).view(torch.int32)
    c0, c1 = int(cnt[0]), int(cnt[1])
    return desc[0, :c0], desc[1, :c1], idx[0, :c0].long(), idx[1, :c1].long()


@functools.lru_cache(maxsize=None)
def _gold(name):
    g = np.load(GOLD / f"lgl_{name}.npz")
    out = {k: torch.from_numpy(np.asarray(g[k])) for k in ("matches0", "matches1", "matching_scores0", "matching_scores1", "matches", "scores",
                                                           "prune0", "prune1")}
    out["stop"] = int(g["stop"])
    return out, {k: float(g[k]) for k in ("dense_res64", "desc_res64", "min_margin")}


@functools.lru_cache(maxsize=None)
def _refs(name):
    """The fp32 oracle (integer decisions, taps) and the fp64 evaluation of a golden case: computed once, shared, never modified."""
    case = GOLDEN_CASES[name]
    sd, (f0, f1) = case_weights(case), case_inputs(case)
    return oracle(f0, f1, sd, conf_of(case)), oracle(f0, f1, sd, conf_of(case), torch.float64)


# ---- 1 + 2. goldens, dense log-assignment and final descriptors against fp64 ------------------------------------------------------------
def golden(lib, device, name):
    """The module's outputs and the oracle's, integer for integer (max_ties = 0: the golden script asserted every decision margin >= 1e-3); the dense
    log-assignment and the final descriptors within 2 x the fp32 oracle's own distance from the fp64 evaluation (the factor the XFeat tests use for
    another summation order at the same precision)."""
    case = GOLDEN_CASES[name]
    sd, (f0, f1) = case_weights(case), case_inputs(case)
    gold, yard = _gold(name)
    ref32, ref64 = _refs(name)
    net = make_net(lib, device, sd, case["conf"], max_kpts=max(case["m"], case["n"]))
    capi.check(lib, lib.dim_saturation_reset(net._stream()))
    out = cpu(net(data_of(f0, f1), dense=True))
    compare_lightglue(out, gold, max_ties=0)
    compare_lightglue(out, ref32, max_ties=0)
    res = {"stop": out["stop"], "matches": int(out["matches"][0].shape[0])}
    if ref32["stop"] == NET["n_layers"] and "log_assignment" in ref32:
        la64 = ref64["log_assignment"]
        mm, nn = la64.shape[0] - 1, la64.shape[1] - 1
        dense = (out["dense"][:mm, :nn].double() - la64[:mm, :nn]).abs().max().item()
        d0, d1, i0, i1 = final_desc(net)
        assert torch.equal(i0, ref64["ind0"]) and torch.equal(i1, ref64["ind1"]), "surviving keypoints"
        t0, t1 = ref64["layers"][-1][0], ref64["layers"][-1][1]
        desc = max((d0.double() - t0).abs().max().item(), (d1.double() - t1).abs().max().item())
        res.update(dense_diff64=dense, dense_yardstick=yard["dense_res64"], desc_diff64=desc, desc_yardstick=yard["desc_res64"])
        print(f"lighterglue {name} {device}: log-assignment vs fp64 {dense:.3e} (fp32 oracle {yard['dense_res64']:.3e}), descriptors {desc:.3e} "
              f"(fp32 oracle {yard['desc_res64']:.3e}), {res['matches']} matches")
        record(f"lgl_{name}_{device}", **res)
        assert dense <= 2 * yard["dense_res64"], (dense, yard["dense_res64"])
        assert desc <= 2 * yard["desc_res64"], (desc, yard["desc_res64"])
    else:   # the empty exit: nothing dense to compare
        assert out["stop"] < NET["n_layers"] and out["matches"][0].shape[0] == 0 and float(out["matching_scores0"].abs().max()) == 0.0
        record(f"lgl_{name}_{device}", **res)
    return out


# ---- 3. edge counts ----------------------------------------------------------------------------------------------------------------------
def _pair(seed, m, n, size=((480.0, 640.0), (618.0, 640.0))):
    return case_inputs({"seed": seed, "m": max(m, 1), "n": max(n, 1), "size0": size[0], "size1": size[1]})


def _cut(f, k):
    return {"kpts": f["kpts"][:k].contiguous(), "desc": f["desc"][:k].contiguous(), "size": f["size"]}


def _check(net, f0, f1, sd, conf):
    out = cpu(net(data_of(f0, f1), dense=True))
    ref = oracle(f0, f1, sd, conf)
    compare_lightglue(out, ref, dense_ref=ref.get("log_assignment"), dense_out=out["dense"], dense_tol=2e-2, ind0=ref.get("ind0"), ind1=ref.get("ind1"))
    return out


def edge_counts(lib, device):
    """0 keypoints on one side and on both, 1 x 40, exact tile multiples, and the 31 / 32 / 33-key sweep on ONE handle (the tile tail of the V image and of the
    masked softmax).  Against the oracle on the same inputs, near ties allowed by compare_lightglue's default rule (these are not golden cases)."""
    sd = weights_mod.synthetic_lighterglue_state_dict(3)
    conf = dict(NET)
    net = make_net(lib, device, sd, max_kpts=96)
    f0, f1 = _pair(21, 64, 96)
    for m, n in ((0, 40), (40, 0), (0, 0)):
        out = _check(net, _cut(f0, m), _cut(f1, n), sd, conf)
        assert out["stop"] == 1 and out["matches"][0].shape[0] == 0 and out["matches0"].shape[1] == m
    for m, n in ((1, 40), (32, 32), (64, 96)):
        out = _check(net, _cut(f0, m), _cut(f1, n), sd, conf)
        assert out["stop"] == NET["n_layers"]
    counts = []
    for k in (31, 32, 33, 31):
        out = _check(net, _cut(f0, 40), _cut(f1, k), sd, conf)
        counts.append(out["matches"][0].shape[0])
    assert counts[0] == counts[3] and min(counts) > 5, counts


# ---- 4. batch = singles, reused handle --------------------------------------------------------------------------------------------------
def _attention_splits(cap, items):
    """launch_lgl_attention's choice (csrc/lg_attn_d96.hip) for a call whose feature table has `cap` rows per image, on a handle whose key-split scratch
    covers the call (at most 8 items)."""
    wgs = -(-((cap + 3) & ~3) // 128) * items
    return 1 if wgs >= 512 else (2 if wgs >= 256 else 4)


def batch_equals_singles(lib, device):
    sd = weights_mod.synthetic_lighterglue_state_dict(3)
    g = torch.Generator().manual_seed(3)
    n_img, cap = 4, 300
    counts = [300, 0, 123, 257]
    f0, f1 = _pair(22, 300, 300)
    # images 0 / 2 / 3: image 0's keypoints perturbed (so that pairs of them match), ragged counts
    kt = torch.zeros(n_img, cap, 2); dt = torch.zeros(n_img, cap, 64)
    kt[0], dt[0] = f0["kpts"], f0["desc"]
    kt[2], dt[2] = f1["kpts"], f1["desc"]
    kt[3] = f0["kpts"] + torch.randn(cap, 2, generator=g)
    dt[3] = torch.nn.functional.normalize(f0["desc"] + 0.05 * torch.randn(cap, 64, generator=g), dim=-1)
    nt = torch.tensor(counts, dtype=torch.int32)
    st = torch.tensor([[640.0, 480.0]] * n_img)
    pairs = torch.tensor([[0, 2], [2, 3], [0, 1], [3, 0]], dtype=torch.int32)
    net = make_net(lib, device, sd, max_pairs=4, max_kpts=cap)
    o = {k: v.cpu() for k, v in net.match_batch_guarded(kt.to(device), dt.to(device), nt.to(device), st.to(device), pair_idx=pairs.to(device)).items()}
    single = make_net(lib, device, sd, max_pairs=1, max_kpts=cap)

    def one(net_, a, b):
        data = {"image0": {"keypoints": kt[a, :counts[a]][None], "descriptors": dt[a, :counts[a]][None], "image_size": st[a][None]},
                "image1": {"keypoints": kt[b, :counts[b]][None], "descriptors": dt[b, :counts[b]][None], "image_size": st[b][None]}}
        return cpu(net_(data))

    total = 0
    for p, (a, b) in enumerate(pairs.tolist()):
        r = one(single, a, b)
        S = int(o["n_matches"][p])
        total += S
        assert int(o["stop"][p]) == r["stop"]
        assert torch.equal(o["matches"][p, :S], r["matches"][0])
        assert torch.equal(o["matches01"][p, 0, :counts[a]].long(), r["matches0"][0]) and torch.equal(o["prune01"][p, 0, :counts[a]].long(), r["prune0"][0].long())
        # same launch shape -> bit-equal scores: a 2-item and an 8-item launch of 3 query blocks per item both stay below 256 attention workgroups, so both
        # cut the key range in 4 (launch_lgl_attention) with the same share per part, and the GEMM blocks a launch picks accumulate in the same order.
        # (rtol 1e-3 would be the bound for a pair whose key split differs between the two launches; there is none here.)
        assert _attention_splits(300, 8) == _attention_splits(max(counts[a], counts[b], 1), 2) == 4
        assert torch.equal(o["scores"][p, :S], r["scores"][0])
        assert torch.equal(o["mscores01"][p, 0, :counts[a]], r["matching_scores0"][0]) and torch.equal(o["mscores01"][p, 1, :counts[b]], r["matching_scores1"][0])
        if counts[a] == 0 or counts[b] == 0:
            assert S == 0 and r["stop"] == 1
    assert total > 100, total
    # a reused handle (large pair, small pair, large pair) equals fresh handles
    first, mid, again = one(single, 0, 3), one(single, 2, 3), one(single, 0, 3)
    fresh_small = one(make_net(lib, device, sd, max_pairs=1, max_kpts=cap), 2, 3)
    for x, y in ((first, again), (mid, fresh_small)):
        assert x["stop"] == y["stop"] and torch.equal(x["matches"][0], y["matches"][0]) and torch.equal(x["scores"][0], y["scores"][0])
        assert torch.equal(x["matches0"], y["matches0"]) and torch.equal(x["prune1"], y["prune1"])


# ---- 5. range guard ---------------------------------------------------------------------------------------------------------------------
def guard(lib, device):
    """One to_v output channel times 2^16 and its consumer column of to_out times 2^-16: the real arithmetic is unchanged, the stored V leaves +-4094.
    The guard fires under fp16x3 and the guarded re-run (bf16x6) equals the golden."""
    assert capi.get_arithmetic(lib) == 2
    case = GOLDEN_CASES["fixed"]
    sd, (f0, f1) = {k: v.clone() for k, v in case_weights(case).items()}, case_inputs(case)
    s = 2.0 ** 16
    sd["transformers.2.cross_attn.to_v.weight"][7] *= s
    sd["transformers.2.cross_attn.to_v.bias"][7] *= s
    sd["transformers.2.cross_attn.to_out.weight"][:, 7] /= s
    net = make_net(lib, device, sd, case["conf"], max_kpts=max(case["m"], case["n"]))
    kt = torch.zeros(2, 130, 2); dt = torch.zeros(2, 130, 64)
    kt[0, :70], kt[1], dt[0, :70], dt[1] = f0["kpts"], f1["kpts"], f0["desc"], f1["desc"]
    nt, st = torch.tensor([70, 130], dtype=torch.int32), torch.stack([f0["size"], f1["size"]])
    capi.check(lib, lib.dim_saturation_reset(net._stream()))
    net.match_batch(kt.to(device), dt.to(device), nt.to(device), st.to(device), n_pairs=1)
    total, sites = capi.saturation(lib, net._stream(), reset=True)
    assert total > 0 and "lg_qkv" in sites, (total, sites)
    out = cpu(net(data_of(f0, f1)))   # guarded: repeats the call in bf16x6
    compare_lightglue(out, _gold("fixed")[0], max_ties=0)


# ---- 5b. attention undamped, adaptive depth ------------------------------------------------------------------------------------------------
def _dense_weights(seed):
    """nn.Linear-style weights with gain 2 at LighterGlue's shape: the blocks are NOT near-identity (the matching weights scale ffn.3 by 0.003, which damps
    an error of the attention ~300-fold), so what self and cross attention compute reaches the outputs undamped."""
    return weights_mod.synthetic_lighterglue_state_dict(seed, matching=False, gain=2.0)


@functools.lru_cache(maxsize=None)
def _undamped_refs():
    sd, (f0, f1) = _dense_weights(7), _pair(23, 70, 130)
    conf = {**NET, "width_confidence": -1, "filter_threshold": 0.0}
    return sd, f0, f1, conf, oracle(f0, f1, sd, conf), oracle(f0, f1, sd, conf, torch.float64)


def attention_undamped(lib, device):
    """Six layers of self and cross attention at d = 96 with nothing damping them, 70 x 130 keypoints (both off the 32-key tile), against the fp64 evaluation:
    the final descriptors and the log-assignment within 2 x the fp32 oracle's own distance from fp64 (the goldens' yardstick and factor).  A softmax scale
    off by 1e-5 relative — 96^-0.25 mistyped in its sixth digit — misses this bound several times over."""
    sd, f0, f1, conf, ref32, ref64 = _undamped_refs()
    net = make_net(lib, device, sd, {"width_confidence": -1, "filter_threshold": 0.0}, max_kpts=130)
    out = cpu(net(data_of(f0, f1), dense=True))
    d0, d1, _, _ = final_desc(net)
    t32, t64 = ref32["layers"][-1], ref64["layers"][-1]
    yard_desc = max((t32[0].double() - t64[0]).abs().max().item(), (t32[1].double() - t64[1]).abs().max().item())
    desc = max((d0.double() - t64[0]).abs().max().item(), (d1.double() - t64[1]).abs().max().item())
    la64 = ref64["log_assignment"][:-1, :-1]
    yard_la = (ref32["log_assignment"][:-1, :-1].double() - la64).abs().max().item()
    la = (out["dense"][:70, :130].double() - la64).abs().max().item()
    scale = max(t64[0].abs().max().item(), t64[1].abs().max().item())
    print(f"lighterglue undamped {device}: descriptors vs fp64 {desc:.3e} (fp32 oracle {yard_desc:.3e}, max |x| {scale:.2f}), log-assignment {la:.3e} (fp32 oracle {yard_la:.3e})")
    record(f"lgl_undamped_{device}", desc_diff64=desc, desc_yardstick=yard_desc, dense_diff64=la, dense_yardstick=yard_la, max_abs_desc=scale)
    assert desc <= 2 * yard_desc, (desc, yard_desc)
    assert la <= 2 * yard_la, (la, yard_la)


def adaptive_depth(lib, device):
    """A positive depth_confidence on a 96-wide handle (the network's default is -1; a caller's conf may set it): the gated per-layer assignment of
    lgl_match.  Token-confidence biases of -6 in layers 0 and 1 and +6 from layer 2 on stop the pair after its third layer; against the oracle with the same
    conf, default near-tie rule."""
    sd, (f0, f1) = _dense_weights(11), _pair(24, 90, 75)
    for i in range(NET["n_layers"] - 1):
        sd[f"token_confidence.{i}.token.0.bias"] = torch.full((1,), -6.0 if i < 2 else 6.0)
    conf = {**NET, "depth_confidence": 0.5, "filter_threshold": 0.0}
    ref = oracle(f0, f1, sd, conf)
    assert ref["stop"] == 3, ref["stop"]
    net = make_net(lib, device, sd, {"depth_confidence": 0.5, "filter_threshold": 0.0}, max_kpts=90)
    out = cpu(net(data_of(f0, f1), dense=True))
    compare_lightglue(out, ref, dense_ref=ref.get("log_assignment"), dense_out=out["dense"], ind0=ref.get("ind0"), ind1=ref.get("ind1"))
    # ... and another pair on the same handle afterwards (the stop flags of the previous call must not leak)
    g0, g1 = _pair(25, 40, 33)
    ref2 = oracle(g0, g1, sd, conf)
    out2 = cpu(net(data_of(g0, g1), dense=True))
    compare_lightglue(out2, ref2, dense_ref=ref2.get("log_assignment"), dense_out=out2["dense"], ind0=ref2.get("ind0"), ind1=ref2.get("ind1"))


# ---- 6. ABI -----------------------------------------------------------------------------------------------------------------------------
def abi(lib, device):
    sd = weights_mod.synthetic_lighterglue_state_dict(3)
    for dim, heads in ((128, 2), (96, 2), (64, 1)):
        try:
            make_net(lib, device, sd, max_kpts=64, descriptor_dim=dim, num_heads=heads)
        except capi.DimHipError as e:
            assert "descriptor_dim" in str(e) and str(dim) in str(e), str(e)
        else:
            raise AssertionError(f"dim_lgl_create accepted ({dim}, {heads})")
    net = make_net(lib, device, sd, max_kpts=64)
    assert net.input_dim == 64 and net.descriptor_dim == 96 and net.num_heads == 1
    bad = torch.zeros(2, 64, 128, device=device)
    try:
        net.match_batch(torch.zeros(2, 64, 2, device=device), bad, torch.tensor([8, 8], dtype=torch.int32, device=device), torch.ones(2, 2, device=device))
    except AssertionError:
        pass
    else:
        raise AssertionError("a feature table of another input_dim was accepted")
    # a 256-wide handle through the old entry still passes an existing golden case
    case = gc.LG_CASES["fixed"]
    sd256 = gc.lg_weights(case)
    g0, g1 = gc.lg_inputs(case)
    old = lg_mod.LightGlueHIP(sd256, case["conf"], max_pairs=1, max_kpts=max(case["m"], case["n"]), device=device, lib=lib)
    out = cpu(old(data_of(g0, g1)))
    g = np.load(GOLD / "lg_fixed.npz")
    gold = {k: torch.from_numpy(np.asarray(g[k])) for k in ("matches0", "matches1", "matching_scores0", "matching_scores1", "matches", "scores", "prune0", "prune1")}
    gold["stop"] = int(g["stop"])
    compare_lightglue(out, gold)


# ---- 7. the plugin's size table -------------------------------------------------------------------------------------------------------------
def plugin_feats(f, hw, dtype=np.float32, dn=False):
    """A feature dict as features.h5 holds it: image_size (H, W), descriptors (N, 64) or (64, N)."""
    d = f["desc"].numpy().astype(dtype)
    return {"keypoints": f["kpts"].numpy().astype(dtype), "descriptors": np.ascontiguousarray(d.T) if dn else d, "image_size": np.array(hw)}


def plugin_size_table(monkeypatch, conf):
    """LighterGlueMatcher._match_pairs on a non-square pair whose features carry (H, W): the size table that reaches the library (match_batch's, which
    both the host path and the staged one-upload path of a GPU go through) holds (W, H), and the matches are the oracle's.  The oracle called both ways
    cannot tell the two orders apart: keypoints are normalised by (k - size / 2) / (max(size) / 2), so swapping the size only TRANSLATES them, and
    LightGlue sees positions through rotary self-attention alone, which depends on position differences.  Returns (matcher, matches, f0, f1, hw0, hw1)."""
    plugins = importlib.import_module("deep-image-matching_amd.plugins")
    seen, call = [], lgl_mod.LighterGlueHIP.match_batch

    def spy(self, kpts_tab, desc_tab, n_tab, size_tab, *a, **k):
        seen.append(size_tab.detach().cpu().clone())
        return call(self, kpts_tab, desc_tab, n_tab, size_tab, *a, **k)
    monkeypatch.setattr(lgl_mod.LighterGlueHIP, "match_batch", spy)
    sizes = plugins.LighterGlueMatcher._size_as_the_network_sees_it
    assert sizes({"image_size": np.array((300, 640))}).tolist() == [640.0, 300.0] and sizes({"image_size": [torch.tensor([300.7, 640.2])]}).tolist() == [640.0, 300.0]
    case = {"seed": 31, "m": 90, "n": 75, "size0": (300.0, 640.0), "size1": (640.0, 300.0)}
    f0, f1 = case_inputs(case)                      # sizes (W, H)
    hw0, hw1 = (300, 640), (640, 300)
    mt = plugins.LighterGlueMatcher({"general": {}, "matcher": conf}, local_features="xfeat")
    got = mt._match_pairs(plugin_feats(f0, hw0), plugin_feats(f1, hw1))
    assert seen and seen[-1].reshape(2, 2).tolist() == [[640.0, 300.0], [300.0, 640.0]], seen
    right = oracle(f0, f1, mt._sd, NET, taps=False)["matches"].numpy()
    swapped = oracle({**f0, "size": f0["size"].flip(0)}, {**f1, "size": f1["size"].flip(0)}, mt._sd, NET, taps=False)["matches"].numpy()
    assert np.array_equal(got, right) and np.array_equal(swapped, right)
    return mt, got, f0, f1, hw0, hw1


# ---- 8. chain ---------------------------------------------------------------------------------------------------------------------------
def chain(lib, device):
    """tests/xfeat_cases.chain's two shifted crops -> XFeatHIP -> LighterGlueHIP with the matching synthetic weights centred on the pair's mean
    descriptor (and whitened); the same chain through xfeat_ref + the oracle.  Equal match lists up to compare_lightglue's default near-tie rule (at most 2 ties,
    each recorded); the share of matches at the true shift is reported for both."""
    from tests import xfeat_cases, xfeat_ref
    a, b = xfeat_cases.photo()[100:292, 200:456].astype(np.float32), xfeat_cases.photo()[116:308, 224:480].astype(np.float32)
    ra, rb = (xfeat_ref.xfeat_forward(i, xfeat_cases.weights(), top_k=256, taps=True) for i in (a, b))
    # the matching synthetic weights compare the 96-wide states, which input_proj makes of the 64-wide rows: centre (and whiten: the seeded XFeat's
    # descriptors share most of their direction, centred norm 0.34) the INPUT — input_proj(A (x - c)) — which is the same map, folded into its weights
    center, whiten = weights_mod.descriptor_whitening(torch.cat([ra["descriptors"], rb["descriptors"]]))
    sd = weights_mod.synthetic_lighterglue_state_dict(3)
    sd["input_proj.weight"] = (sd["input_proj.weight"] @ (0.5 * whiten)).contiguous()
    sd["input_proj.bias"] = sd["input_proj.bias"] - sd["input_proj.weight"] @ center
    xnet = xfeat_cases.make_net(lib, device, (192, 256), top_k=256, max_batch=2)
    x = torch.stack([torch.from_numpy(a), torch.from_numpy(b)]).contiguous().to(device)
    kp, sc, de, n = xnet.extract_batch(x)
    n0, n1 = int(n[0].item()), int(n[1].item())
    assert n0 > 100 and n1 > 100
    net = make_net(lib, device, sd, max_kpts=256)
    st = torch.tensor([[256.0, 192.0]] * 2, device=device)
    o = net.match_batch_guarded(kp[:, :256].contiguous(), de[:, :256, :64].contiguous(), n, st, n_pairs=1, dense=True)
    S = int(o["n_matches"][0].item())
    out = {"matches0": o["matches01"][0, 0, :n0].cpu(), "matches1": o["matches01"][0, 1, :n1].cpu(), "matching_scores0": o["mscores01"][0, 0, :n0].cpu(),
           "matching_scores1": o["mscores01"][0, 1, :n1].cpu(), "stop": int(o["stop"][0]), "matches": o["matches"][0, :S].cpu(), "scores": o["scores"][0, :S].cpu(),
           "prune0": o["prune01"][0, 0, :n0].cpu(), "prune1": o["prune01"][0, 1, :n1].cpu()}
    f0 = {"kpts": ra["keypoints"].float(), "desc": ra["descriptors"], "size": st[0].cpu()}
    f1 = {"kpts": rb["keypoints"].float(), "desc": rb["descriptors"], "size": st[1].cpu()}
    assert n0 == f0["kpts"].shape[0] and n1 == f1["kpts"].shape[0], "the extractor chain selected another keypoint count than its reference"
    ref = oracle(f0, f1, sd, NET)
    # (the log-assignment is handed over for the near-tie rule only: the two chains' DESCRIPTORS differ by the extractor's own tolerance, which whitening
    # and the sharp final_proj multiply by ~1e4 in the logits — the dense comparison belongs to the goldens, whose inputs are shared)
    res = compare_lightglue(out, ref, dense_ref=ref.get("log_assignment"), dense_out=o["dense"][0].cpu(), dense_tol=float("inf"), max_ties=2,
                            filter_threshold=NET["filter_threshold"], ind0=ref.get("ind0"), ind1=ref.get("ind1"))
    shift = np.array([24.0, 16.0])
    share_of = lambda k0, k1, m: float(np.mean(np.abs(k0[m[:, 0]] - k1[m[:, 1]] - shift).max(axis=1) < 0.5)) if len(m) else 0.0   # noqa: E731
    share = share_of(kp[0].cpu().numpy(), kp[1].cpu().numpy(), out["matches"].numpy())
    ref_share = share_of(f0["kpts"].numpy(), f1["kpts"].numpy(), ref["matches"].numpy())
    ties = res.get("explained_near_ties", [])
    print(f"lighterglue chain {device}: {S} matches, share at the true shift {share:.4f}, reference {ref_share:.4f} ({ref['matches'].shape[0]}), near ties {ties}")
    record(f"lgl_chain_{device}", matches=S, share=share, reference_matches=int(ref["matches"].shape[0]), reference_share=ref_share, near_ties=str(ties))
    assert S > 30 and abs(S - int(ref["matches"].shape[0])) <= 2
    assert abs(share - ref_share) <= 2.0 / max(1, S)
