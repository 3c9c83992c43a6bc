"""CPU (emulator): per-tile geometric verification (``geometric_verification_per_tile``, matchers/matcher_base.py:427-440) in the batched
tile matcher — tile pairs through verify.DeviceVerifier and dim_op_filter_matches — against the numpy oracle followed by the
fewer-than-15-inliers rule, for the host-table function, the device-table function and the matcher's own ``_match_by_tile``."""
import importlib

import numpy as np
import torch

from tests import tile_verify_cases as tc

plugins = importlib.import_module("deep-image-matching_amd.plugins")
tm = importlib.import_module("deep-image-matching_amd.tile_matching")
verify = importlib.import_module("deep-image-matching_amd.verify")

GENERAL = {"tile_size": (64, 64), "tile_overlap": 0, "geom_verification": "MAGSAC", "gv_threshold_in_tiles_matching": 4}


def _matcher(general):
    return plugins.KorniaMatcher({"general": general, "matcher": {"name": "kornia_matcher", "match_mode": "mnn", "th": 0.8}})


def _verifier(lib):
    return verify.DeviceVerifier(threshold=tc.THRESHOLD, iters=tc.ITERS, error_type="sampson", seed=tc.SEED, device="cpu", lib=lib)


def test_tile_pairs_are_verified_like_the_reference_loop(emu_install):
    f0, f1, expected, unverified = tc.case()
    m = _matcher(GENERAL)
    v = _verifier(emu_install)
    got = tm.match_tile_pairs_batched(m._ensure_pairs, f0, f1, tc.TILE_PAIRS, "cpu", verifier=v)
    assert got.dtype == np.int64 and np.array_equal(got, expected)
    d0, d1 = tc.device_features(f0, "cpu"), tc.device_features(f1, "cpu")
    got_dev = tm.match_tile_pairs_batched_device(m._ensure_pairs, d0, d1, tc.TILE_PAIRS, verifier=v)
    assert got_dev.dtype == torch.int64 and np.array_equal(got_dev.numpy(), expected)
    # without a verifier both functions return what they returned before: every match of every tile pair
    assert np.array_equal(tm.match_tile_pairs_batched(m._ensure_pairs, f0, f1, tc.TILE_PAIRS, "cpu"), unverified)
    assert np.array_equal(tm.match_tile_pairs_batched_device(m._ensure_pairs, d0, d1, tc.TILE_PAIRS).numpy(), unverified)
    # geom_verification NONE: all-ones masks, then the 15 rule — the 10-match tile pair goes, the other two stay whole
    none = tm.match_tile_pairs_batched(m._ensure_pairs, f0, f1, tc.TILE_PAIRS, "cpu", verifier=verify.AllInliersVerifier(lib=emu_install))
    t0_of = {int(i): int(t) for i, t in enumerate(f0["tile_idx"])}
    assert np.array_equal(none, unverified[[t0_of[int(r[0])] != 1 for r in unverified]])
    # a chunk boundary inside the list: pair positions restart, results are still lists of verified rows
    split = tm.match_tile_pairs_batched(m._ensure_pairs, f0, f1, tc.TILE_PAIRS, "cpu", pair_batch=2, verifier=v)
    assert split.shape[1] == 2 and set(map(tuple, split)) <= set(map(tuple, unverified))


def test_match_by_tile_with_geometric_verification_per_tile(emu_install, tmp_path):
    """The matcher's hook with the option set: no cv2, no per-tile-pair call — the batched path with a DeviceVerifier built from the
    configuration (raw gv_threshold_in_tiles_matching, Sampson, 2048 hypotheses, seed 0)."""
    from PIL import Image

    f0, f1, expected, unverified = tc.case()
    paths = []
    for k in range(2):
        p = tmp_path / f"im{k}.png"
        Image.fromarray(np.zeros(tc.HW, np.uint8)).save(p)
        paths.append(p)
    m = _matcher({**GENERAL, "geometric_verification_per_tile": True})
    got = m._match_by_tile(paths[0], paths[1], f0, f1, method="GRID")
    assert np.array_equal(got, expected)
    v = m._tile_verifier()
    assert isinstance(v, verify.DeviceVerifier) and (v.threshold, v.iters, v.seed, v.error_type) == (4.0, 2048, 0, 0) and m._tile_verifier() is v
    plain = _matcher(GENERAL)._match_by_tile(paths[0], paths[1], f0, f1, method="GRID")
    assert np.array_equal(plain, unverified)
    none = _matcher({**GENERAL, "geom_verification": "NONE", "geometric_verification_per_tile": True})
    assert isinstance(none._tile_verifier(), verify.AllInliersVerifier)
