"""Device NMS (mvg_pose_nms / ops.pose_nms), the part that needs no GPU: the numpy restatement of its contract
(tests/nms_ref.py) is pinned to the reference's golden vectors and to the host functions, the generated scenes take every
branch of the greedy pass, and the C ABI rejects bad arguments before it launches anything."""
import ctypes
import os

import numpy as np
import pytest
import torch

from mvgformer_amd import _lib
from mvgformer_amd import evaluate as E
from oracle import eval_ref as O
from tests import nms_cases, nms_ref
from tests.golden.eval_cases import NMS_CASES, panoptic_scene

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "eval.npz"))
MVG_E_BADARG = 10001


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", sorted(NMS_CASES))
def test_restatement_matches_reference_golden(name):
    spec = NMS_CASES[name]
    preds, _, _ = panoptic_scene(spec["seed"], frames=spec["frames"])
    for f, p in enumerate(preds):
        keep = nms_ref.nearby_joints_nms(p, spec["dist_thr"], spec["num_nearby"], max_dets=spec.get("max_dets", -1))
        assert keep == GOLD["nms_%s_f%d" % (name, f)].tolist(), (name, f)


@pytest.mark.parametrize("name", ["n1", "n63", "n64", "n65", "n130", "n130_flagged", "n65_j14", "n130_maxdets", "n1024"])
def test_restatement_matches_host_nms_on_generated_scenes(name):
    """distinct scores: the stable visiting order is the reference's order, so the product's host NMS (and, at the sizes its
    Python loops allow, the oracle's) must give the restatement's keep list on the classification-filtered rows"""
    pred, kw, (keep, count, dets, stats) = nms_cases.generated(name)
    rows = np.flatnonzero(pred[:, 0, 3] >= 0)
    cand = pred[rows]
    args = (0.3, kw.get("num_nearby_joints_thr", 7), kw.get("max_dets", -1))
    assert [int(rows[k]) for k in E.nearby_joints_nms(cand, *args)] == keep
    if len(cand) <= 65:
        assert [int(rows[k]) for k in O.nearby_joints_nms(cand, *args)] == keep
    assert count == [len(keep), 0] and np.array_equal(dets, pred[keep])
    assert len(set(keep)) == len(keep) and all(pred[k, 0, 3] >= 0 for k in keep)
    if "max_dets" not in kw and len(pred) <= 130:
        # filter_and_nms: the same rows, row for row
        assert np.array_equal(E.filter_and_nms(torch.from_numpy(np.array(pred)), 0.3, args[1]).numpy(), dets)


@pytest.mark.parametrize("name", [k for k, v in nms_cases.GENERATED.items() if v[0] >= 63])
def test_generated_scenes_take_every_branch(name):
    """so that the GPU comparison cannot pass on scenes that never leave the trivial branch: `close` is not symmetric, some visit
    hands its slot to another pose, some visit finds its best already ignored -- and poses are both kept and suppressed"""
    pred, kw, (keep, count, dets, stats) = nms_cases.generated(name)
    print(name, "kept", count[0], stats)
    assert stats["asymmetric"] > 0 and stats["best_is_other"] > 0 and stats["best_ignored"] > 0, stats
    assert 0 < count[0] < int((pred[:, 0, 3] >= 0).sum())


def test_max_dets_selects_the_best_scored_kept_poses():
    pred, kw, (keep, count, dets, stats) = nms_cases.generated("n130_maxdets")
    full = nms_cases.generated("n130")[2][0]
    assert len(full) > 7 and len(keep) == 7
    assert keep == sorted(full, key=lambda k: -pred[k, 0, 4])[:7]


# ------------------------------------------------------------------------------------------------ degenerate inputs
def test_ties_up_to_16_rows_follow_the_host_functions():
    """Tied scores in a scene of at most 16 rows, ties inside one neighbourhood included.  The host functions visit tied rows in
    whatever order np.argsort's default sort leaves them: an insertion sort (= the documented rule) only in numpy builds without
    the vectorised sort; numpy 2.2 on an AVX-512 CPU orders [.7, .7, .3, .7] differently.  So the case ties only repeated poses,
    for which every visiting order gives one result, and the restatement must give exactly that."""
    pred, kw, (keep, count, dets, stats) = nms_cases.degenerate_reference("ties_small")
    assert len(pred) <= 16 and len(np.unique(pred[:, 0, 4])) < len(pred)
    assert pred[0, 0, 4] == pred[1, 0, 4] and np.array_equal(pred[0, :, :3], pred[1, :, :3])     # a tie inside a neighbourhood
    pred = np.array(pred)
    assert E.nearby_joints_nms(pred, 0.3, 7) == keep == O.nearby_joints_nms(pred, 0.3, 7)
    assert 0 in keep and 1 not in keep                                                            # np.argmax: the lower row
    for md in (1, 2, 3):
        assert E.nearby_joints_nms(pred, 0.3, 7, max_dets=md) == nms_ref.pose_nms(pred, 0.3, 7, max_dets=md)[0]


def test_tied_scores_beyond_16_rows_are_deterministic():
    for name in ("ties_large", "ties_large_maxdets"):
        pred, kw, (keep, count, dets, stats) = nms_cases.degenerate_reference(name)
        assert len(pred) > 16 and len(np.unique(pred[:, 0, 4])) <= 4 and 0 < count[0] < len(pred)
        assert nms_ref.pose_nms(np.array(pred), **kw)[0] == keep
        assert stats["best_is_other"] > 0 and stats["best_ignored"] > 0


def test_empty_neighbourhoods_are_counted_and_ignored():
    for name, row in (("zero_extent", 4), ("nan_coordinate", 2)):
        pred, kw, (keep, count, dets, stats) = nms_cases.degenerate_reference(name)
        assert count[1] == 1 and row not in keep, name
        # neither kept nor suppressing: the other rows come out as if the row were not a candidate
        without = np.array(pred)
        without[row, :, 3] = -1.0
        assert nms_ref.pose_nms(without, **kw)[0] == keep
        with pytest.raises(ValueError):                                 # the reference's behaviour: np.argmax of an empty sequence
            E.nearby_joints_nms(np.array(pred), 0.3, 7)


def test_no_candidate_and_one_candidate():
    pred, kw, (keep, count, dets, stats) = nms_cases.degenerate_reference("all_flagged")
    assert keep == [] and count == [0, 0] and dets.shape == (0, 15, 5)
    pred, kw, (keep, count, dets, stats) = nms_cases.degenerate_reference("one_candidate")
    assert keep == [13] and count == [1, 0]
    pred, kw, (keep, count, dets, stats) = nms_cases.generated("n1")
    assert keep == [0] and count == [1, 0]


# ------------------------------------------------------------------------------------------------ C ABI, host side
def test_symbols_are_exported_and_in_the_ctypes_table():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in ("mvg_pose_nms_workspace", "mvg_pose_nms"):
        assert hasattr(lib, s) and s in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["mvg_pose_nms"]) == 14 and _lib.SIGNATURES["mvg_pose_nms"][4] is ctypes.c_double


def test_workspace_size_is_monotone_in_n():
    lib = _lib.load()
    sizes = [lib.mvg_pose_nms_workspace(1, n, 15) for n in range(1, 2049)]
    assert all(s > 0 and s % 8 == 0 for s in sizes) and all(b >= a for a, b in zip(sizes, sizes[1:]))
    assert lib.mvg_pose_nms_workspace(3, 1024, 15) == 3 * sizes[1023]
    # the closeness bit matrix alone: N rows of ceil(N / 64) 64-bit words
    assert sizes[2047] >= 2048 * 32 * 8 and sizes[63] >= 64 * 8
    assert lib.mvg_pose_nms_workspace(1, 2049, 15) == 0 and lib.mvg_pose_nms_workspace(0, 8, 15) == 0
    assert lib.mvg_pose_nms_workspace(1, 8, 33) == 0


@pytest.mark.parametrize("B,N,J,dist_thr,nn", [
    (1, 8, 15, 0.0, 7), (1, 8, 15, -1.0, 7), (1, 8, 15, float("nan"), 7),      # dist_thr <= 0
    (1, 8, 15, 0.3, 15), (1, 8, 15, 0.3, -1),                                  # num_nearby_joints_thr >= J or < 0
    (1, 8, 33, 0.3, 7),                                                         # J > 32
    (1, 2049, 15, 0.3, 7), (1, 1 << 20, 15, 0.3, 7),                            # N above the maximum
    (0, 8, 15, 0.3, 7), (1, 0, 15, 0.3, 7),                                     # B or N == 0
    (1, 8, 15, 0.3, 7),                                                         # valid shape, NULL pointers
])
def test_bad_arguments_are_rejected_before_any_launch(B, N, J, dist_thr, nn):
    """no GPU is needed: a call that got as far as a launch would return a HIP error, not MVG_E_BADARG"""
    lib = _lib.load()
    assert lib.mvg_pose_nms(None, B, N, J, dist_thr, nn, -1, None, 0, None, None, None, N, None) == MVG_E_BADARG


def test_python_wrapper_argument_errors_and_cpu_tensors():
    from mvgformer_amd import ops
    pred = torch.from_numpy(np.array(nms_cases.generated("n63")[0]))[None]
    with pytest.raises(AssertionError, match="`dist_thr` must be greater than 0."):
        ops.pose_nms(pred, dist_thr=0.0)
    with pytest.raises(AssertionError, match="`num_nearby_joints_thr` must be less than the number of joints."):
        ops.pose_nms(pred, num_nearby_joints_thr=15)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.pose_nms(pred)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        E.filter_and_nms_device(pred[0])
    with pytest.raises(RuntimeError, match=r"\(B, N, J, 5\) float32"):
        ops.pose_nms(pred.double())
