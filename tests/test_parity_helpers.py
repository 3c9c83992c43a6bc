"""CPU: the comparators themselves — the near-tie rule accepts only what the oracle's own log-assignment margins explain."""
import pytest
import torch

from tests.parity import compare_lightglue


def _side(m0, n):
    m0 = torch.tensor(m0)
    m1 = torch.full((n,), -1)
    for i, j in enumerate(m0.tolist()):
        if j >= 0:
            m1[j] = i
    pairs = torch.tensor([[i, j] for i, j in enumerate(m0.tolist()) if j >= 0])
    return {"stop": 3, "prune0": torch.zeros(len(m0)), "prune1": torch.zeros(n), "matches0": m0, "matches1": m1,
            "matching_scores0": torch.where(m0 >= 0, torch.tensor(0.36), torch.tensor(0.0)),
            "matching_scores1": torch.where(m1 >= 0, torch.tensor(0.36), torch.tensor(0.0)),
            "matches": [pairs], "scores": [torch.full((len(pairs),), 0.36)]}


def test_near_tie_rule_of_compare_lightglue():
    m, n = 6, 5
    la = torch.full((m + 1, n + 1), -20.0)
    for i, j in ((0, 1), (2, 3), (4, 0)):
        la[i, j] = -1.0
    la[2, 4] = -1.00005                                   # row 2: two candidates 5e-5 apart in the ORACLE's own scores
    ref, tie, real = _side([1, -1, 3, -1, 0, -1], n), _side([1, -1, 4, -1, 0, -1], n), _side([1, -1, 2, -1, 0, -1], n)
    assert compare_lightglue(ref, ref)["n_matches0_mismatch"] == 0
    res = compare_lightglue(tie, ref, dense_ref=la, dense_out=la)
    assert res["n_matches0_mismatch"] == 1 and len(res["explained_near_ties"]) == 2
    with pytest.raises(AssertionError, match="unexplained match difference"):
        compare_lightglue(real, ref, dense_ref=la, dense_out=la)       # (2, 2) scores -20 in the oracle: not a tie
    with pytest.raises(AssertionError, match="no log-assignment"):
        compare_lightglue(tie, ref)                                     # without the oracle's scores nothing is excused
    la[2, 4] = -1.01                                                    # 1e-2 apart: a real disagreement
    with pytest.raises(AssertionError, match="unexplained match difference"):
        compare_lightglue(tie, ref, dense_ref=la, dense_out=la)


def test_near_tie_rule_with_point_pruning_needs_the_surviving_indices():
    """With point pruning the oracle's log-assignment is indexed by the SURVIVING keypoints (ind0 / ind1: ascending, nothing reordered, some indices
    skipped).  A 5e-5 tie there is explained only when compare_lightglue is given ind0 / ind1; without them the match is looked up at the wrong row
    and column and rejected; a match on a keypoint the oracle pruned is never explained."""
    m, n = 6, 5
    ind0, ind1 = torch.tensor([0, 2, 4, 5]), torch.tensor([0, 1, 3, 4])          # keypoints 1, 3 of image 0 and 2 of image 1 were pruned
    la = torch.full((len(ind0) + 1, len(ind1) + 1), -20.0)                       # pruned space: 4 x 4 (+ the dustbin row / column)
    for i, j in ((0, 1), (1, 2), (2, 0)):                                        # = (0, 1), (2, 3), (4, 0) in keypoint indices
        la[i, j] = -1.0
    la[1, 3] = -1.00005                                                          # keypoint 2 of image 0: candidates 3 and 4 are 5e-5 apart
    ref, tie, gone = _side([1, -1, 3, -1, 0, -1], n), _side([1, -1, 4, -1, 0, -1], n), _side([1, 2, 3, -1, 0, -1], n)
    for d in (ref, tie, gone):
        d["prune0"], d["prune1"] = torch.tensor([3, 1, 3, 1, 3, 3]), torch.tensor([3, 3, 1, 3, 3])
    assert compare_lightglue(ref, ref, dense_ref=la, dense_out=la, ind0=ind0, ind1=ind1)["n_matches0_mismatch"] == 0
    res = compare_lightglue(tie, ref, dense_ref=la, dense_out=la, ind0=ind0, ind1=ind1)
    assert res["n_matches0_mismatch"] == 1 and sorted(t["match"] for t in res["explained_near_ties"]) == [(2, 3), (2, 4)]
    assert all(t["row_top2_margin"] < 1e-4 for t in res["explained_near_ties"])
    with pytest.raises(AssertionError, match="unexplained match difference"):
        compare_lightglue(tie, ref, dense_ref=la, dense_out=la)                 # keypoint indices used as pruned-space indices: (2, 3) scores -20 there
    with pytest.raises(AssertionError, match="match on a keypoint the oracle pruned"):
        compare_lightglue(gone, ref, dense_ref=la, dense_out=la, ind0=ind0, ind1=ind1)   # (1, 2): both keypoints were pruned
    la[1, 3] = -1.01                                                            # 1e-2 apart: a real disagreement, with or without the index maps
    with pytest.raises(AssertionError, match="unexplained match difference"):
        compare_lightglue(tie, ref, dense_ref=la, dense_out=la, ind0=ind0, ind1=ind1)
