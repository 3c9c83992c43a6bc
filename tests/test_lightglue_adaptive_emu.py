"""CPU: adaptive LightGlue (the reference's default depth / width confidences, the mode of the plugin hook) on REUSED handles, against the oracle.

A handle keeps every buffer of its state from call to call: K | V tile images, the similarity matrix (row stride = the handle's capacity), the
partial attention records, live counts / index tables / prune counters / stop flags and the page-locked stop-flag mirrors.  The emulator poisons
fresh device memory with NaNs, so a read of never-written memory trips the range guard — but what an earlier, LARGER call left behind is finite and
plausible.  Every sequence below therefore runs calls of different sizes and stop layers on ONE handle (the plugin keeps one handle and calls it
with the table size of every pair) and checks each call against the oracle, and against the same call on a fresh handle.

Inputs: workloads.adaptive_lightglue_workload — pairs designed to stop after 3 .. 9 layers with ~25 % of their keypoints prunable; ragged calls
are cut out of it by truncating table and counts.  The oracle's smallest top-2 margin of a reported match on these inputs is 5e-2 (500 x the
near-tie tolerance): integer outputs are expected to be identical.  All tolerances are compare_lightglue's defaults.

N_KPTS is odd, above 128 (one pair per call: the attention launches cut the keys in 4 parts, a part then holds more than one 32-key tile) and
smaller than the handles' 256 rows (strides follow the handle, launch shapes the table)."""
import importlib

import numpy as np
import pytest
import torch

from oracle import lightglue_ref
from tests import adaptive_cases as ac

lg_mod = importlib.import_module("deep-image-matching_amd.lightglue_hip")
capi = importlib.import_module("deep-image-matching_amd.capi")

N_KPTS, NMAX = 163, 256
P3, P4, P5, P8, P9 = 0, 1, 2, 5, 6          # workload pair numbers by designed stop layer

_ORACLE, _SINGLE = {}, {}


def _key(pairs, cap, counts):
    return (tuple(pairs), cap, None if counts is None else tuple(map(tuple, counts)))


def _oracles(pairs, cap, counts=None):
    """[oracle result per pair of the call] (cached: it does not depend on the library, the handle or a kernel selection)."""
    k = _key(pairs, cap, counts)
    if k not in _ORACLE:
        wl = ac.workload(7, N_KPTS)
        call = ac.call_of(wl, pairs, cap, counts)
        _ORACLE[k] = [ac.oracle_of(wl[0], call, 2 * q, 2 * q + 1) for q in range(len(pairs))]
    return _ORACLE[k]


def _run(net, pairs, cap, counts=None, n_pairs=None):
    wl = ac.workload(7, N_KPTS)
    kt, dt, nt, st = ac.call_of(wl, pairs, cap, counts)
    o = net.match_batch(kt, dt, nt, st, n_pairs=n_pairs, dense=True)
    return [ac.row_of(o, q, int(nt[2 * q]), int(nt[2 * q + 1])) for q in range(len(pairs) if n_pairs is None else n_pairs)]


def _fresh_single(lib, pair, cap, counts=None):
    """The call on a FRESH one-pair handle of NMAX rows, checked against the oracle (cached per call)."""
    k = _key([pair], cap, counts)
    if k not in _SINGLE:
        net = lg_mod.LightGlueHIP(ac.workload(7, N_KPTS)[0], ac.CONF, max_pairs=1, max_kpts=NMAX, device="cpu", lib=lib)
        row = _run(net, [pair], cap, counts)[0]
        ac.check_row(row, _oracles([pair], cap, counts)[0])
        _SINGLE[k] = row
    return _SINGLE[k]


def _no_saturation(lib):
    total, sites = capi.saturation(lib, None, reset=False)
    assert total == 0, sites


# (workload pair, table rows per image, live counts) — in this order on one handle
SEQUENCE_1 = [
    (P9, N_KPTS, (N_KPTS, N_KPTS)),     # all 9 layers at the largest size: fills every tile image and every layer's stop-flag mirror
    (P3, 61, (61, 57)),                 # odd table (launch shapes for 64 rows); the followed loop leaves early, later mirrors are stale
    (P5, 130, (113, 130)),
    (P3, 61, (61, 57)),
    (P4, 77, (0, 77)),                  # an image without keypoints: the "no keypoints" exit
    (P8, 1, (1, 1)),
    (P4, N_KPTS, (N_KPTS, N_KPTS)),
]


def test_one_pair_handle_reused_across_sizes_and_stop_layers(emu_lib):
    """The plugin's pattern: ONE one-pair handle whose capacity (256) is larger than every table, called with tables of 163 / 61 / 130 / 61 / 77 / 1 / 163
    rows whose pairs stop after 9 / 3 / 5 / 3 / 1 / ? / 4 layers, with the host following the stop flags (dim_tune_set key 18 = 1) and not (0).  Every call
    equals the same call on a fresh handle bit for bit — which equals the oracle — and equals the oracle itself; the range guard stays silent."""
    sd, *_, expect = ac.workload(7, N_KPTS)
    fresh = [_fresh_single(emu_lib, p, cap, [cnt]) for p, cap, cnt in SEQUENCE_1]
    for (p, cap, cnt), row in zip(SEQUENCE_1, fresh):
        if min(cnt) >= 57:      # (the designed stop layer holds for truncated tables; the degenerate ones follow the oracle alone)
            assert row["stop"] == int(expect[p]), (p, cap, row["stop"])
    assert fresh[4]["stop"] == 1 and fresh[4]["matches"][0].shape[0] == 0
    assert min(fresh[i]["matches"][0].shape[0] for i in (0, 1, 2, 6)) > 0
    capi.saturation(emu_lib, None, reset=True)
    try:
        for follow in (1, 0):
            assert emu_lib.dim_tune_set(18, follow) == 0
            net = lg_mod.LightGlueHIP(sd, ac.CONF, max_pairs=1, max_kpts=NMAX, device="cpu", lib=emu_lib)
            assert net.nk == NMAX
            for step, (p, cap, cnt) in enumerate(SEQUENCE_1):
                row = _run(net, [p], cap, [cnt])[0]
                ac.assert_rows_bit_equal(row, fresh[step], (follow, step))
                ac.check_row(row, _oracles([p], cap, [cnt])[0])
                _no_saturation(emu_lib)
    finally:
        emu_lib.dim_tune_set(18, 1)


def test_two_pair_handle_followed_with_a_slot_left_over(emu_lib):
    """Handles of up to two pairs follow the stop flags too: the loop may only leave when EVERY pair of the call has stopped.  Pairs that stop after 3 and
    9 layers in one call; then a one-pair call (slot 1 keeps the state — stop flag, counts, mirrors — of the call before); then the two pairs with
    swapped slots.  Every pair equals the oracle and its own run on a fresh one-pair handle (same integers, scores to fp32 rounding: a two-pair launch
    takes other block shapes)."""
    sd = ac.workload(7, N_KPTS)[0]
    net = lg_mod.LightGlueHIP(sd, ac.CONF, max_pairs=2, max_kpts=NMAX, device="cpu", lib=emu_lib)
    capi.saturation(emu_lib, None, reset=True)
    assert emu_lib.dim_tune_set(18, 1) == 0
    calls = [([P3, P9], N_KPTS, None, None), ([P5], 130, [(113, 130)], 1), ([P9, P3], N_KPTS, None, None)]
    for step, (pairs, cap, counts, n_pairs) in enumerate(calls):
        rows = _run(net, pairs, cap, counts, n_pairs)
        refs = _oracles(pairs, cap, counts)
        for q, p in enumerate(pairs):
            ac.check_row(rows[q], refs[q])
            one = _fresh_single(emu_lib, p, cap, None if counts is None else [counts[q]])
            a, b = rows[q], one
            assert a["stop"] == b["stop"], (step, q)
            for k in ("matches0", "matches1", "prune0", "prune1"):
                assert torch.equal(a[k], b[k]), (step, q, k)
            assert torch.equal(a["matches"][0], b["matches"][0]), (step, q)
            assert a["matches"][0].shape[0] > 0 and (a["scores"][0] - b["scores"][0]).abs().max().item() < 1e-5, (step, q)
        _no_saturation(emu_lib)
    assert [r["stop"] for r in _oracles([P3, P9], N_KPTS)] == [3, 9]


@pytest.mark.parametrize("kv_from_gemm", [2, 1], ids=["large_batch_kernels_forced", "unforced"])
def test_batched_handle_reused_with_fewer_pairs_and_a_smaller_table(emu_lib, kv_from_gemm):
    """A four-pair handle (no host-side following): a ragged four-pair call at 163 rows, then TWO pairs at 90 rows through pair_idx that reuse image rows
    (a pair and its swap; slots 2, 3 keep their state), then four other pairs — with the large-batch kernels (K | V tile images written by the
    projection GEMM) forced as the golden tests do (dim_tune_set(6, 2)) and unforced.  Every pair of every call equals the oracle."""
    wl = ac.workload(7, N_KPTS)
    sd, expect = wl[0], wl[4]
    calls = [([P3, P4, P5, P9], N_KPTS, [(N_KPTS, 150), (121, N_KPTS), (N_KPTS, N_KPTS), (157, N_KPTS)]),
             None,
             ([P9, 3, P3, P4], N_KPTS, [(N_KPTS, N_KPTS), (140, N_KPTS), (N_KPTS, 101), (N_KPTS, N_KPTS)])]
    try:
        assert emu_lib.dim_tune_set(6, kv_from_gemm) == 0
        net = lg_mod.LightGlueHIP(sd, ac.CONF, max_pairs=4, max_kpts=NMAX, device="cpu", lib=emu_lib)
        capi.saturation(emu_lib, None, reset=True)
        for step, c in enumerate(calls):
            if c is not None:
                pairs, cap, counts = c
                rows, refs = _run(net, pairs, cap, counts), _oracles(pairs, cap, counts)
                for q, p in enumerate(pairs):
                    assert refs[q]["stop"] == int(expect[p]) and refs[q]["matches"].shape[0] > 0
                    ac.check_row(rows[q], refs[q])
            else:
                kt, dt, nt, st = ac.call_of(wl, [3], 90, [(90, 83)])       # the two images of the pair designed to stop after 6 layers
                pi = torch.tensor([[0, 1], [1, 0]], dtype=torch.int32)
                o = net.match_batch(kt, dt, nt, st, pair_idx=pi, dense=True)
                k = ("pair_idx", 3, 90, (90, 83))
                if k not in _ORACLE:
                    _ORACLE[k] = [ac.oracle_of(sd, (kt, dt, nt, st), a, b) for a, b in pi.tolist()]
                for q, (a, b) in enumerate(pi.tolist()):
                    assert _ORACLE[k][q]["stop"] == 6 and _ORACLE[k][q]["matches"].shape[0] > 0
                    ac.check_row(ac.row_of(o, q, int(nt[a]), int(nt[b])), _ORACLE[k][q])
            _no_saturation(emu_lib)
    finally:
        emu_lib.dim_tune_set(6, 1)


def test_plugin_matcher_keeps_its_handle_across_pair_sizes(emu_install, tmp_path):
    """LightGlueMatcher._match_pairs as the reference's loop calls it: features as features.h5 holds them (float16, descriptors (D, N)), ONE matcher for
    pairs of 203 -> 61 -> 130 -> 300 -> 61 keypoints.  On a CPU device the first handle has 256 rows; 300 keypoints rebuild it with 512; the last pair
    runs on the rebuilt one.  Every (S, 2) result equals the oracle's match list on the same fp16-rounded inputs.  (The oracle always prunes: the
    matcher must be told pruning_min_kpts -1; the range guard raises instead of falling back.)"""
    plugins = importlib.import_module("deep-image-matching_amd.plugins")
    sd = ac.workload(1, 61, stops=(3,))[0]
    torch.save(sd, tmp_path / "lg.pth")
    m = plugins.LightGlueMatcher({"general": {}, "matcher": {"name": "lightglue", "depth_confidence": 0.95, "width_confidence": 0.99, "filter_threshold": 0.1,
                                                             "pruning_min_kpts": -1, "weights_path": str(tmp_path / "lg.pth"), "on_saturation": "raise"}})
    assert m._conf["n_layers"] == 9 and m._conf["pruning_min_kpts"] == -1
    handles, refs = [], {}
    for n, drop, stop in ((203, 0, 9), (61, 4, 3), (130, 0, 5), (300, 20, 4), (61, 4, 3)):
        sd_n, kp, de, sz, _ = ac.workload(1, n, stops=(stop,))
        assert all(torch.equal(sd_n[k], sd[k]) for k in sd)        # one set of weights whatever the size
        f0, k0, d0 = ac.h5_features(kp[0], de[0], sz[0])
        f1, k1, d1 = ac.h5_features(kp[1, :n - drop], de[1, :n - drop], sz[1])
        assert f0["descriptors"].shape == (256, n) and f0["descriptors"].dtype == np.float16
        got = m._match_pairs(f0, f1)
        if (n, stop) not in refs:
            refs[(n, stop)] = lightglue_ref.lightglue_forward(k0, d0, sz[0], k1, d1, sz[1], sd, ac.CONF)
        ref = refs[(n, stop)]
        assert ref["stop"] == stop and ref["matches"].shape[0] > 0.5 * (n - drop), (n, ref["stop"], ref["matches"].shape)
        assert got.dtype == np.int64 and np.array_equal(got, ref["matches"].numpy()), (n, got.shape, ref["matches"].shape)
        handles.append((m._net, m._net_n))
    assert [h[1] for h in handles] == [256, 256, 256, 512, 512]
    assert handles[0][0] is handles[2][0] and handles[3][0] is handles[4][0] and handles[3][0] is not handles[0][0]


def test_adaptive_workload_batch_vs_oracle(emu_lib):
    """The flagship adaptive batch (bench.py's, pinned at full size on hardware by tests/test_lightglue_adaptive_gpu.py) at 128 keypoints as ONE seven-pair
    call: stop layers 3 .. 9 as designed, prune counters, match lists, scores and the dense log-assignment of every pair equal to the oracle."""
    wl = ac.workload(7, 128)
    sd, expect = wl[0], wl[4]
    call = ac.call_of(wl, range(7), 128)
    net = lg_mod.LightGlueHIP(sd, ac.CONF, max_pairs=7, max_kpts=128, device="cpu", lib=emu_lib)
    capi.saturation(emu_lib, None, reset=True)
    o = net.match_batch(*call, dense=True)
    _no_saturation(emu_lib)
    assert expect.tolist() == list(ac.STOPS)
    for p in range(7):
        ref = ac.oracle_of(sd, call, 2 * p, 2 * p + 1)
        assert ref["stop"] == int(expect[p])
        pruned = [float((ref[k] < ref["prune0"].max()).float().mean()) for k in ("prune0", "prune1")]
        assert all(0.15 < f < 0.35 for f in pruned) and ref["matches"].shape[0] > 64, (p, pruned, ref["matches"].shape)
        ac.check_row(ac.row_of(o, p, 128, 128), ref)
