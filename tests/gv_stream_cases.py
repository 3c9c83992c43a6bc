"""Shared inputs of the streaming geometric-verification tests (CPU emulator and GPU): the four oracle-pinned pairs, the
two edge pairs, the non-identity match tables, and the oracle results (computed once per process and never modified)."""
import functools

import numpy as np
import torch

from oracle import geom_ref

ITERS, SEED, THRESHOLD = 256, 5, 1.5
# (n_inliers, n_outliers, scene seed): 4096 = the LDS limit, 4097 = one point into the second chunk, 8193 = one point into
# the third chunk of 4096 (fifth of 2048), 100 = a single short chunk; pair index = position in this list
SCENES = [(3000, 1096, 21), (2500, 1597, 22), (5000, 3193, 23), (60, 40, 24)]
ORACLE_INLIERS = {"sampson": [3004, 2504, 5014, 60], "symmetric_epipolar": [3001, 2500, 5006, 60]}     # as the issue lists them
ERR = {"sampson": 0, "symmetric_epipolar": 1}


@functools.lru_cache(maxsize=None)
def scene(i):
    ni, no, seed = SCENES[i]
    x0, x1, _, _ = geom_ref.synthetic_two_view(ni, no, seed=seed, noise_px=0.3)
    x0.setflags(write=False); x1.setflags(write=False)
    return x0, x1


@functools.lru_cache(maxsize=None)
def oracle(i, err, pair):
    """(F, mask, count) of scene i verified as pair `pair` of a call"""
    x0, x1 = scene(i)
    F, mask, cnt, _ = geom_ref.fundamental_ransac(x0, x1, THRESHOLD, iters=ITERS, err_type=ERR[err], seed=SEED, pair=pair)
    mask.setflags(write=False); F.setflags(write=False)
    return F, mask, cnt


def tables(cases, nk, cap=None):
    """cases: list of (x0, x1) -> (kpts_tab [2P, cap, 2], matches [P, nk, 2], n [P]); matches are not the identity
    (idx1 = perm[idx0], as tests/test_geom_verify_emu.py builds them)."""
    P = len(cases)
    cap = cap or max(8, max(len(c[0]) for c in cases))
    kt = torch.zeros(2 * P, cap, 2)
    mt = torch.zeros(P, nk, 2, dtype=torch.int64)
    n = torch.zeros(P, dtype=torch.int32)
    for p, (x0, x1) in enumerate(cases):
        s = len(x0)
        perm = np.random.default_rng(p).permutation(s)
        kt[2 * p, :s] = torch.from_numpy(np.array(x0))
        kt[2 * p + 1, perm] = torch.from_numpy(np.array(x1))
        mt[p, :s, 0] = torch.arange(s)
        mt[p, :s, 1] = torch.from_numpy(perm)
        n[p] = s
    return kt.contiguous(), mt.contiguous(), n


def unit(F):
    return np.asarray(F, np.float64) / np.linalg.norm(F)


def f_distance(Fa, Fb):
    """largest element difference of two fundamental matrices after Frobenius normalisation, up to sign"""
    a, b = unit(Fa), unit(Fb)
    return float(min(np.abs(a - b).max(), np.abs(a + b).max()))


def check_against_oracle(out, err, mask_places, count_places):
    """The per-pair assertions of the six-pair call (four scenes, a 5-match pair, an empty pair) against the oracle."""
    mask_all, ninl, Fs = out["mask"].cpu().numpy().astype(bool), out["n_inliers"].cpu().numpy(), out["F"].cpu().numpy()
    for p in range(len(SCENES)):
        x0, _ = scene(p)
        s = len(x0)
        F, mask, cnt = oracle(p, err, p)
        assert cnt == ORACLE_INLIERS[err][p]
        got = mask_all[p, :s]
        print(f"pair {p} ({err}): n {s} device inliers {int(ninl[p])} oracle {cnt} mask differences {int((got != mask).sum())} "
              f"F distance {f_distance(Fs[p], F):.3e}")
        assert int(ninl[p]) == int(got.sum())
        assert not mask_all[p, s:].any()
        assert (got != mask).sum() <= mask_places and abs(int(ninl[p]) - cnt) <= count_places
        assert f_distance(Fs[p], F) <= 1e-6
        assert abs(np.linalg.det(unit(Fs[p]))) < 1e-9                                        # rank 2
    # fewer than 8 matches: every match is an inlier, F = 0; the empty pair
    assert int(ninl[4]) == 5 and mask_all[4, :5].all() and not mask_all[4, 5:].any() and float(np.abs(Fs[4]).sum()) == 0.0
    assert int(ninl[5]) == 0 and not mask_all[5].any()


def six_pair_cases():
    x0, x1 = scene(3)
    return [scene(i) for i in range(len(SCENES))] + [(x0[:5], x1[:5]), (x0[:0], x1[:0])]
