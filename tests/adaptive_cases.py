"""Shared by the adaptive-LightGlue tests (emulator and GPU): calls cut out of workloads.adaptive_lightglue_workload, the oracle per pair,
and the comparison of one row of a match_batch result with it."""
from __future__ import annotations

import importlib

import numpy as np
import torch

from oracle import lightglue_ref
from tests.parity import compare_lightglue

CONF = {"n_layers": 9, "depth_confidence": 0.95, "width_confidence": 0.99, "filter_threshold": 0.1, "pruning_min_kpts": -1}
STOPS = (3, 4, 5, 6, 7, 8, 9)
# the ragged counts of the full-size batch (image 0, image 1)
RAGGED_2048 = ((2048, 1777), (1500, 2048), (1024, 2048), (61, 130), (2047, 2045), (1, 2048))

_WORKLOADS = {}


def workload(n_pairs, n_kpts, stops=STOPS):
    """(state_dict, kpts [2P, N, 2], desc [2P, N, 256], sizes [2P, 2], designed stop layers [P]) — cached; read only."""
    key = (n_pairs, n_kpts, tuple(stops))
    if key not in _WORKLOADS:
        wl = importlib.import_module("deep-image-matching_amd.workloads")
        sd, kp, de, _, sz, expect = wl.adaptive_lightglue_workload(n_pairs, n_kpts=n_kpts, stops=tuple(stops))
        _WORKLOADS[key] = (sd, kp, de, sz, expect)
    return _WORKLOADS[key]


def call_of(wl, pairs, cap, counts=None):
    """One dim_lg_match call: the feature table of `pairs` (workload pair numbers) cut to `cap` rows per image, items 2q / 2q + 1 = pairs[q], with
    `counts` [(m, n) per pair] live keypoints (default: cap, cap).  Returns (kpts, desc, counts int32, sizes) — contiguous CPU tensors."""
    _, kp, de, sz, _ = wl
    items = [i for p in pairs for i in (2 * p, 2 * p + 1)]
    counts = [(cap, cap)] * len(pairs) if counts is None else counts
    assert all(0 <= c <= cap for mn in counts for c in mn)
    nt = torch.tensor([c for mn in counts for c in mn], dtype=torch.int32)
    return kp[items, :cap].contiguous(), de[items, :cap].contiguous(), nt, sz[items].contiguous()


def oracle_of(sd, call, a, b, conf=CONF):
    """The oracle on items a, b of a call (their live rows)."""
    kt, dt, nt, st = call
    na, nb = int(nt[a]), int(nt[b])
    return lightglue_ref.lightglue_forward(kt[a, :na], dt[a, :na], st[a], kt[b, :nb], dt[b, :nb], st[b], sd, conf, taps=True)


def row_of(o, p, m, n):
    """Row p of a match_batch result (CPU tensors or device tensors) as the reference-style dict compare_lightglue takes; the tables are only
    defined up to the live counts."""
    o = {k: v.cpu() for k, v in o.items()}
    S = int(o["n_matches"][p])
    res = {"stop": int(o["stop"][p]), "matches0": o["matches01"][p, 0, :m].long(), "matches1": o["matches01"][p, 1, :n].long(),
           "matching_scores0": o["mscores01"][p, 0, :m], "matching_scores1": o["mscores01"][p, 1, :n],
           "prune0": o["prune01"][p, 0, :m], "prune1": o["prune01"][p, 1, :n],
           "matches": [o["matches"][p, :S].clone()], "scores": [o["scores"][p, :S].clone()]}
    if "dense" in o:
        res["dense"] = o["dense"][p]
    return res


def check_row(row, ref, **kw):
    """compare_lightglue at its default tolerances with everything the oracle knows: dense log-assignment and the surviving indices."""
    return compare_lightglue(row, ref, dense_ref=ref.get("log_assignment"), dense_out=row.get("dense"), ind0=ref.get("ind0"), ind1=ref.get("ind1"),
                             filter_threshold=CONF["filter_threshold"], **kw)


def assert_rows_bit_equal(a, b, what=""):
    """Two reference-style rows (row_of) of the same call: every output bit for bit, the dense log-assignment included."""
    assert a["stop"] == b["stop"], (what, a["stop"], b["stop"])
    for k in ("matches0", "matches1", "matching_scores0", "matching_scores1", "prune0", "prune1", "dense"):
        if k in a or k in b:
            assert torch.equal(a[k], b[k]), (what, k)
    assert torch.equal(a["matches"][0], b["matches"][0]) and torch.equal(a["scores"][0], b["scores"][0]), (what, "compact list")


def h5_features(kpts, desc, size):
    """One image's features as features.h5 holds them: float16, descriptors (D, N), image_size (H, W) — and the same values back in float32 as
    the oracle's inputs (the fp16 -> fp32 conversion is exact)."""
    k16, d16 = kpts.numpy().astype(np.float16), np.ascontiguousarray(desc.numpy().T.astype(np.float16))
    feats = {"keypoints": k16, "descriptors": d16, "image_size": np.asarray(size.tolist(), np.int32)}
    return feats, torch.from_numpy(k16.astype(np.float32)), torch.from_numpy(np.ascontiguousarray(d16.T).astype(np.float32))
