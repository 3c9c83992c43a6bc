"""CPU (emulator): the nearest-neighbour descriptor matcher (csrc/nn_match.hip, dim_nn_*) against the fp64 decision rule of tests/nn_ref.py.

Inputs are planted unit-norm sets (nn_ref.planted) with replaced rows, so every mode accepts some rows and rejects others; the may-set stays
within 1 % of the must-set on each of them (asserted).  ``tol`` is measured per input from the reference's fp32 arithmetic (nn_ref.measured_tol)."""
import importlib

import numpy as np
import pytest
import torch

from tests import nn_ref

nn = importlib.import_module("deep-image-matching_amd.nn_hip")
capi = importlib.import_module("deep-image-matching_amd.capi")

TH = 0.9


def _table(sets, cap=None):
    """[(a, b), ...] -> (desc_tab [2P][cap][D], n_tab [2P])"""
    cap = cap or max(max(a.shape[0], b.shape[0]) for a, b in sets)
    D = sets[0][0].shape[1]
    tab = torch.zeros(2 * len(sets), max(cap, 1), D)
    nt = torch.zeros(2 * len(sets), dtype=torch.int32)
    for p, (a, b) in enumerate(sets):
        tab[2 * p, : a.shape[0]], tab[2 * p + 1, : b.shape[0]] = a, b
        nt[2 * p], nt[2 * p + 1] = a.shape[0], b.shape[0]
    return tab.contiguous(), nt


def _lists(o, P):
    n = o["n_matches"].numpy()
    return [o["matches"][p, : int(n[p])].numpy().copy() for p in range(P)], [o["scores"][p, : int(n[p])].numpy().copy() for p in range(P)]


def _net(lib, mode, D, max_pairs=1, max_kpts=256, th=TH, **k):
    return nn.NearestNeighborHIP(mode, th, dim=D, max_pairs=max_pairs, max_kpts=max_kpts, device="cpu", lib=lib, **k)


def _sets(M, N, D, seed):
    """planted pair cut to (M, N): 20 % of image 1's rows replaced by noise"""
    a, b = nn_ref.planted(max(M, N), D, seed=seed, replaced=0.2)
    return a[:M].contiguous(), b[:N].contiguous()


_REF = {}


def _ref(M, N, D, seed):
    """fp64 distances + measured tol + fp32 reference lists of one input, computed once and shared"""
    key = (M, N, D, seed)
    if key not in _REF:
        a, b = _sets(M, N, D, seed)
        d2 = nn_ref.d2_fp64(a, b)
        _REF[key] = (a, b, d2, nn_ref.measured_tol(a, b, d2))
    return _REF[key]


# M != N, sizes that are no multiple of the 128-wide tile (one tile, 2 x 2 tiles, 1 x 3 tiles), every descriptor width
SHAPES = [(203, 130, 64), (61, 150, 128), (130, 203, 256), (100, 300, 128)]


@pytest.mark.parametrize("mode", nn_ref.MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_modes_follow_the_fp64_rule(emu_lib, mode, shape):
    M, N, D = shape
    a, b, d2, tol = _ref(M, N, D, seed=3)
    must, may = nn_ref.classify_fp64(a, b, mode, TH, tol, d2)
    assert len(must) >= 20 and len(may) <= 0.01 * len(must), (len(must), len(may))
    ref_m, ref_d = nn_ref.reference_fp32(a, b, mode, TH)
    nn_ref.check_rule(ref_m, must, may, "fp32 reference")          # guards the rule itself
    if mode != "nn":
        assert len(ref_m) < M                                       # the mode rejects some rows on this input
    tab, nt = _table([(a, b)])
    o = _net(emu_lib, mode, D, max_kpts=max(M, N)).match_batch(None, tab, nt, None, n_pairs=1)      # (row stride 204 / 152 / 300: no tile multiple either)
    (m,), (d,) = _lists(o, 1)
    nn_ref.check_rule(m, must, may, f"{mode} {shape}")
    _check_dists(m, d, d2, mode, tol)


def _check_dists(m, d, d2, mode, tol):
    """The reported dists against fp64: cdist values (nn / mnn) or best / second ratios (snn / smnn), compared as squares — a d^2 within tol of the
    exact one moves a squared ratio b / s by at most tol (1 + b / s) / (s - tol) to first order; 1e-5 relative for the fp32 sqrt / division."""
    if len(m) == 0:
        return
    i, j = torch.from_numpy(m[:, 0]), torch.from_numpy(m[:, 1])
    g2 = torch.from_numpy(d).double() ** 2
    best = d2[i, j]
    if mode in ("nn", "mnn"):
        assert bool(((g2 - best).abs() <= tol + 1e-5 * best).all())
        return

    def other(dd, ii, jj):
        v, a = torch.topk(dd, 2, dim=1, largest=False)
        return torch.where(a[ii, 0] == jj, v[ii, 1], v[ii, 0])

    so = other(d2, i, j)
    want, slack = best / so, tol * (1 + best / so) / (so - tol).clamp_min(1e-300)
    if mode == "smnn":
        sc = other(d2.t(), j, i)
        want, slack = torch.maximum(want, best / sc), torch.maximum(slack, tol * (1 + best / sc) / (sc - tol).clamp_min(1e-300))
    assert bool(((g2 - want).abs() <= 2 * slack + 1e-5 * want).all())


def test_taps_agree_with_fp64_within_tol(emu_lib):
    M, N, D = 203, 130, 64
    a, b, d2, tol = _ref(M, N, D, seed=3)
    tab, nt = _table([(a, b)])
    o = _net(emu_lib, "smnn", D).match_batch(None, tab, nt, None, n_pairs=1, taps=True)
    for stats, dd, cnt in ((o["row_stats"][0], d2, M), (o["col_stats"][0], d2.t(), N)):
        v, _ = torch.topk(dd, 2, dim=1, largest=False)
        idx = stats[0, :cnt].view(torch.int32).long()
        assert float((stats[1, :cnt].double() - v[:, 0]).abs().max()) <= tol
        assert float((stats[2, :cnt].double() - v[:, 1]).abs().max()) <= tol
        # the chosen index is a minimum to within the tolerance
        assert float((dd[torch.arange(cnt), idx] - v[:, 0]).max()) <= 2 * tol


@pytest.mark.parametrize("arith", ["bf16x6", "fp32"])
def test_other_arithmetics_follow_the_rule(emu_lib, arith):
    M, N, D = 130, 203, 256
    a, b, d2, tol = _ref(M, N, D, seed=3)
    tab, nt = _table([(a, b)])
    for mode in ("mnn", "smnn"):
        must, may = nn_ref.classify_fp64(a, b, mode, TH, tol, d2)
        o = _net(emu_lib, mode, D, arithmetic=arith).match_batch(None, tab, nt, None, n_pairs=1)
        nn_ref.check_rule(_lists(o, 1)[0][0], must, may, f"{arith} {mode}")


@pytest.mark.parametrize("mode", nn_ref.MODES)
@pytest.mark.parametrize("mn", [(0, 0), (0, 5), (5, 0), (5, 1), (1, 5), (1, 1)])
def test_too_few_descriptors_give_an_empty_list(emu_lib, mode, mn):
    M, N = mn
    g = torch.Generator().manual_seed(7)
    a, b = torch.randn(M, 64, generator=g), torch.randn(N, 64, generator=g)
    tab, nt = _table([(a, b)], cap=8)
    o = _net(emu_lib, mode, 64).match_batch(None, tab, nt, None, n_pairs=1)
    (m,), _ = _lists(o, 1)
    ref_m, _ = nn_ref.reference_fp32(a, b, mode, TH)
    assert m.shape == (len(ref_m), 2)
    assert {tuple(r) for r in m.tolist()} == {tuple(r) for r in ref_m.tolist()}
    if M == 0 or N == 0 or (mode == "snn" and N < 2) or (mode == "smnn" and min(M, N) < 2):
        assert m.shape == (0, 2)


def test_exact_duplicates_tie_to_the_lowest_index_and_zero_over_zero_is_no_match(emu_lib):
    g = torch.Generator().manual_seed(11)
    D = 64
    a = torch.nn.functional.normalize(torch.randn(140, D, generator=g), dim=1)
    b = a.clone()
    b[5], b[133] = a[9], a[9]        # row 9 of image 0 appears three times in image 1 (columns 5, 9, 133: two tiles): tie -> column 5
    a[70] = a[20]                    # column 20 of image 1 has two exact copies in image 0 (rows 20, 70): tie -> row 20
    tab, nt = _table([(a, b)])
    o = _net(emu_lib, "nn", D).match_batch(None, tab, nt, None, n_pairs=1, taps=True)
    (m,), (d,) = _lists(o, 1)
    assert m[9].tolist() == [9, 5] and m[70].tolist() == [70, 20] and m[20].tolist() == [20, 20]
    rows, cols = o["row_stats"][0], o["col_stats"][0]
    assert float(rows[1, 9]) == 0.0 and float(rows[2, 9]) == 0.0          # best and second-best are both the exact duplicate
    assert int(cols[0, 20].view(torch.int32)) == 20 and float(cols[2, 20]) == 0.0
    (m2,), _ = _lists(_net(emu_lib, "mnn", D).match_batch(None, tab, nt, None, n_pairs=1), 1)
    got = {tuple(r) for r in m2.tolist()}
    assert (20, 20) in got and (70, 20) not in got and (9, 5) in got and (9, 9) not in got      # b[5] = a[9]: (9, 5) is mutual, (9, 9) lost the tie
    for mode in ("snn", "smnn"):
        (ms,), _ = _lists(_net(emu_lib, mode, D, th=0.95).match_batch(None, tab, nt, None, n_pairs=1), 1)
        got = {tuple(r) for r in ms.tolist()}
        assert not any(i == 9 for i, _ in got)           # d_best = d_second = 0: the ratio is 0 / 0
        assert (3, 3) in got                             # an undisturbed exact copy: ratio 0 / d_second = 0 <= th
        if mode == "smnn":
            assert not any(j == 20 for _, j in got)      # column 20's ratio is 0 / 0


def test_batch_through_pair_idx_equals_single_pairs_and_shares_norms(emu_lib):
    D = 128
    imgs = [_sets(150, 150, D, seed=s)[0][: n] for s, n in ((1, 150), (2, 97), (3, 131))]
    imgs.append(_sets(150, 150, D, seed=1)[1][:140])                # image 3 is the planted partner of image 0
    cap = 150
    tab = torch.zeros(4, cap, D)
    nt = torch.tensor([x.shape[0] for x in imgs], dtype=torch.int32)
    for i, x in enumerate(imgs):
        tab[i, : x.shape[0]] = x
    pairs = [(0, 3), (3, 0), (1, 2), (0, 0), (2, 3)]
    pidx = torch.tensor(pairs, dtype=torch.int32)
    net = _net(emu_lib, "mnn", D, max_pairs=8)
    lists, _ = _lists(net.match_batch(None, tab, nt, None, pair_idx=pidx), len(pairs))
    one = _net(emu_lib, "mnn", D)
    for p, (i, j) in enumerate(pairs):
        t2, n2 = _table([(imgs[i], imgs[j])])
        (m,), _ = _lists(one.match_batch(None, t2, n2, None, n_pairs=1), 1)
        assert np.array_equal(lists[p], m), p
    assert len(lists[0]) > 50 and np.array_equal(lists[3], np.stack([np.arange(150)] * 2, 1))      # (0, 0): every row is its own mutual neighbour
    # fewer pairs than the handle holds, through the same handle
    lists2, _ = _lists(net.match_batch(None, tab, nt, None, pair_idx=pidx[2:4].contiguous()), 2)
    assert np.array_equal(lists2[0], lists[2]) and np.array_equal(lists2[1], lists[3])


def test_one_handle_reused_with_shrinking_and_growing_cap_equals_fresh_handles(emu_lib):
    """The stale-state scenario: 203 -> 61 -> 130 -> 61 rows per image on one 256-row handle; every call bit-identical to a fresh handle's."""
    D = 64
    net = _net(emu_lib, "smnn", D)
    for k, cap in enumerate((203, 61, 130, 61)):
        a, b = _sets(cap, max(cap - 7, 2), D, seed=20 + k)
        tab, nt = _table([(a, b)], cap=cap)
        got = net.match_batch(None, tab, nt, None, n_pairs=1, taps=True)
        want = _net(emu_lib, "smnn", D).match_batch(None, tab, nt, None, n_pairs=1, taps=True)
        S = int(want["n_matches"][0])
        assert int(got["n_matches"][0]) == S and S > 10
        assert torch.equal(got["matches"][0, :S], want["matches"][0, :S]) and torch.equal(got["scores"][0, :S], want["scores"][0, :S])
        assert torch.equal(got["row_stats"].view(torch.int32), want["row_stats"].view(torch.int32))
        assert torch.equal(got["col_stats"].view(torch.int32), want["col_stats"].view(torch.int32))


def test_launch_shapes_follow_the_table_not_the_handle(emu_lib):
    """A 300-row table (3 x 3 tiles) on a 640-row handle (5 tiles per side) and with counts above the handle's 140 rows (truncated)."""
    a, b, d2, tol = _ref(290, 300, 64, seed=9)
    tab, nt = _table([(a, b)])
    must, may = nn_ref.classify_fp64(a, b, "smnn", TH, tol, d2)
    big = _net(emu_lib, "smnn", 64, max_kpts=640).match_batch(None, tab, nt, None, n_pairs=1)
    fit = _net(emu_lib, "smnn", 64, max_kpts=300).match_batch(None, tab, nt, None, n_pairs=1)
    (m,), _ = _lists(big, 1)
    nn_ref.check_rule(m, must, may, "oversized handle")
    assert len(m) > 150 and np.array_equal(m, _lists(fit, 1)[0][0])
    small = _net(emu_lib, "mnn", 64, max_kpts=140)
    (mt,), _ = _lists(small.match_batch(None, tab, nt, None, n_pairs=1), 1)
    t2, n2 = _table([(a[:140].contiguous(), b[:140].contiguous())])
    assert small.nk == 140 and np.array_equal(mt, _lists(small.match_batch(None, t2, n2, None, n_pairs=1), 1)[0][0])


def test_two_runs_are_bit_identical(emu_lib):
    a, b, _, _ = _ref(203, 130, 64, seed=3)
    tab, nt = _table([(a, b)])
    net = _net(emu_lib, "smnn", 64)
    o1 = {k: v.clone() for k, v in net.match_batch(None, tab, nt, None, n_pairs=1, taps=True).items()}
    o2 = net.match_batch(None, tab, nt, None, n_pairs=1, taps=True)
    S = int(o1["n_matches"][0])
    assert int(o2["n_matches"][0]) == S
    assert torch.equal(o1["matches"][0, :S], o2["matches"][0, :S]) and torch.equal(o1["scores"][0, :S].view(torch.int32), o2["scores"][0, :S].view(torch.int32))
    assert torch.equal(o1["row_stats"].view(torch.int32), o2["row_stats"].view(torch.int32))


@pytest.mark.parametrize("D", [64, 256])
def test_fp16_exact_fast_path_equals_the_three_term_path_bit_for_bit(emu_lib, D):
    a, b = _sets(203, 130, D, seed=5)
    a, b = a.half().float(), b.half().float()            # what features.h5 holds
    tab, nt = _table([(a, b)])
    net = _net(emu_lib, "smnn", D)
    three = net.match_batch(None, tab, nt, None, n_pairs=1, taps=True, f16_exact=False)
    one = net.match_batch(None, tab, nt, None, n_pairs=1, taps=True, f16_exact=True)
    S = int(three["n_matches"][0])
    assert S > 30 and int(one["n_matches"][0]) == S
    assert torch.equal(one["matches"][0, :S], three["matches"][0, :S]) and torch.equal(one["scores"][0, :S].view(torch.int32), three["scores"][0, :S].view(torch.int32))
    assert torch.equal(one["row_stats"].view(torch.int32), three["row_stats"].view(torch.int32))
    assert torch.equal(one["col_stats"].view(torch.int32), three["col_stats"].view(torch.int32))


def test_range_guard_counts_inputs_beyond_the_fp16_range_and_the_guarded_call_reruns(emu_lib):
    a, b = _sets(140, 90, 64, seed=6)
    a, b = a * 50000.0, b * 50000.0                      # elements up to ~2e4 > 4094
    d2 = nn_ref.d2_fp64(a, b)
    tol = nn_ref.measured_tol(a, b, d2)
    must, may = nn_ref.classify_fp64(a, b, "smnn", TH, tol, d2)
    tab, nt = _table([(a, b)])
    net = _net(emu_lib, "smnn", 64)
    capi.check(emu_lib, emu_lib.dim_saturation_reset(None))
    net.match_batch(None, tab, nt, None, n_pairs=1)
    total, sites = capi.saturation(emu_lib, None)
    assert total > 0 and set(sites) == {"op"}
    o = net.match_batch_guarded(None, tab, nt, None, n_pairs=1)      # re-runs in bf16x6
    nn_ref.check_rule(_lists(o, 1)[0][0], must, may, "guarded")
    assert capi.saturation(emu_lib, None)[0] == 0
    strict = _net(emu_lib, "smnn", 64, on_saturation="raise")
    with pytest.raises(capi.SaturationError):
        strict.match_batch_guarded(None, tab, nt, None, n_pairs=1)


def test_workspace_holds_no_m_by_n_buffer_and_bad_arguments_are_rejected(emu_lib):
    net = _net(emu_lib, "smnn", 256, max_pairs=4, max_kpts=2048)
    assert net.nk == 2048 and 0 < net.workspace_bytes() < 4 * 2048 * 2048 * 4 // 8
    with pytest.raises(ValueError, match="nn.*mnn.*snn.*smnn"):
        _net(emu_lib, "fginn", 64)
    with pytest.raises(capi.DimHipError):
        _net(emu_lib, "nn", 48)
    tab, nt = _table([_sets(10, 10, 64, seed=1)] * 2)
    with pytest.raises(capi.DimHipError):
        _net(emu_lib, "nn", 64, max_pairs=1).match_batch(None, tab, nt, None, n_pairs=2)
