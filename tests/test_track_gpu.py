"""Person identities on the device (csrc/track.hip -> ops.linear_assignment / ops.track_update -> tracking.PoseTracker) against the
numpy fp64 restatement of tests/track_ref.py.

The solver: col_of_row equal and total bit-equal on one B = 6 call with the live sizes (1,1), (5,9), (64,64), (64,3), (0,7),
(7,0), for random float costs, integer costs in 0..3 (many ties: the lowest-index rule), all-equal costs and costs with NaN, +inf
and 1e300 entries (the call must return).  The tracker: frame by frame, ids, slots, every state buffer and every counter equal
(the poses and scores are fp32 copies: bit-equal), on the sequences of tests/track_cases.py, whose preconditions (no near tie,
no cost near the gate) tests/test_track_ref_cpu.py checks."""
import functools

import numpy as np
import pytest
import torch

from mvgformer_amd import _lib, ops
from mvgformer_amd.tracking import PoseTracker
from tests import track_cases as TC
from tests import track_ref as TR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ------------------------------------------------------------------------------------------------------------------------ solver
@functools.lru_cache(maxsize=None)
def _solver_reference(name):
    cost, n, m = TC.solver_matrices()[name]
    want = [TR.solve(cost[b], n[b], m[b]) for b in range(len(n))]
    return np.stack([w[0] for w in want]), np.array([w[1] for w in want], np.float64)


@pytest.mark.parametrize("name", ["random", "ties", "equal", "odd"])
def test_solver_equals_the_restatement(name):
    cost, n, m = TC.solver_matrices()[name]
    want_col, want_total = _solver_reference(name)
    col, total = ops.linear_assignment(torch.from_numpy(cost).to(DEV), torch.from_numpy(n).to(DEV), torch.from_numpy(m).to(DEV))
    torch.cuda.synchronize()
    col, total = col.cpu().numpy(), total.cpu().numpy()
    assert col.dtype == np.int32 and total.dtype == np.float64
    for b, (nb, mb) in enumerate(TC.SOLVER_SIZES):
        assert col[b].tolist() == want_col[b].tolist(), (name, nb, mb)
        assert total[b].tobytes() == want_total[b].tobytes(), (name, nb, mb, total[b], want_total[b])
        live = [c for c in col[b, :nb] if c >= 0]
        assert len(live) == min(nb, mb) and len(set(live)) == len(live)
    print(name, "totals", total.tolist())


def test_solver_without_live_sizes_and_the_crossing_example():
    cost = np.zeros((2, 2, 2))
    cost[0] = [[100.0, 110.0], [105.0, 300.0]]            # greedy takes (0, 0) and pays 400; the optimum is 215
    cost[1] = [[1.0, 2.0], [3.0, 1.5]]
    col, total = ops.linear_assignment(torch.from_numpy(cost).to(DEV))
    assert col.cpu().tolist() == [[1, 0], [0, 1]] and total.cpu().tolist() == [215.0, 2.5]
    rect = np.random.default_rng(3).uniform(0.0, 10.0, size=(1, 5, 9))
    col, total = ops.linear_assignment(torch.from_numpy(rect).to(DEV))
    want_col, want_total = TR.solve(rect[0])
    assert col.cpu().numpy()[0].tolist() == want_col.tolist() and float(total[0]) == want_total


def test_solver_refusals():
    ok = torch.zeros((1, 4, 4), dtype=torch.float64, device=DEV)
    with pytest.raises(_lib.MvgError):
        ops.linear_assignment(torch.zeros((1, 65, 4), dtype=torch.float64, device=DEV))
    with pytest.raises(_lib.MvgError):
        ops.linear_assignment(torch.zeros((1, 4, 65), dtype=torch.float64, device=DEV))
    with pytest.raises(RuntimeError, match="float64"):
        ops.linear_assignment(ok.float())
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.linear_assignment(torch.zeros((1, 4, 8), dtype=torch.float64, device=DEV)[:, :, ::2])
    with pytest.raises(RuntimeError, match="int32"):
        ops.linear_assignment(ok, torch.zeros((1,), dtype=torch.int64, device=DEV))


# ----------------------------------------------------------------------------------------------------------------------- tracker
STATE_KEYS = ("id", "hits", "misses", "born", "score", "pose", "next_id", "state", "ids", "slots")


def _live_only(buf):
    """the buffers with the pose / score / hits / misses / born of FREE slots blanked: they are whatever the last owner left"""
    out = {k: np.array(v, copy=True) for k, v in buf.items()}
    free = out["id"] < 0
    for k in ("hits", "misses", "born", "score"):
        out[k][free] = 0
    out["pose"][free] = 0
    return out


@functools.lru_cache(maxsize=None)
def _reference_run(name):
    """the restatement over the sequence, computed once: per frame a copy of every buffer"""
    seq = TC.float_sequences()[name]
    B, R, J = seq["frames"][0][0].shape[:3]
    buf = TR.new_buffers(B, seq["T"], J, R)
    snaps = []
    for dets, count in seq["frames"]:
        TR.update(dets, count, buf, seq["max_dist"], seq["max_misses"], seq["min_hits"])
        snaps.append(_live_only(buf))
    return snaps


def _device_run(name):
    seq = TC.float_sequences()[name]
    B, R, J = seq["frames"][0][0].shape[:3]
    tracker = PoseTracker(batch=B, rows=R, num_joints=J, max_tracks=seq["T"], max_dist=seq["max_dist"],
                          max_misses=seq["max_misses"], min_hits=seq["min_hits"], device=DEV)
    snaps = []
    for dets, count in seq["frames"]:
        ids, slots = tracker.update(torch.from_numpy(dets).to(DEV), None if count is None else torch.from_numpy(count).to(DEV))
        assert ids is tracker.buffers["ids"] and slots is tracker.buffers["slots"]
        snaps.append(_live_only({k: t.cpu().numpy() for k, t in tracker.buffers.items()}))
    return snaps, tracker


@pytest.mark.parametrize("name", sorted(TC.float_sequences()))
def test_tracker_equals_the_restatement_frame_by_frame(name):
    want = _reference_run(name)
    got, tracker = _device_run(name)
    for f, (g, w) in enumerate(zip(got, want)):
        for k in STATE_KEYS:
            assert g[k].dtype == w[k].dtype and g[k].shape == w[k].shape, (name, f, k)
            assert g[k].tobytes() == w[k].tobytes(), (name, f, k, g[k], w[k])
    st = tracker.state()
    assert st == dict(zip(TR.STATE, want[-1]["state"].tolist())) and st["reserved"] == 0
    assert st["active"] == int((want[-1]["id"] >= 0).sum()) == sum(len(t) for t in tracker.tracks())
    print(name, st)


def test_ids_follow_the_persons():
    """what the sequences are for, read from the device's ids: constant ids on the walk, the optimum where greedy differs, the
    occlusion rule, the overflow, the gate on both sides, the NaN pose, min_hits, the dropped detections"""
    def ids_per_person(name):
        seq = TC.float_sequences()[name]
        got, tracker = _device_run(name)
        return [[{int(w): int(i) for w, i in zip(who[b], g["ids"][b]) if w >= 0} for b in range(who.shape[0])]
                for g, who in zip(got, seq["persons"])], tracker
    hist, tracker = ids_per_person("walk")
    assert all(h[0] == hist[0][0] for h in hist) and sorted(hist[0][0].values()) == [0, 1, 2, 3]
    assert [t.hits for t in tracker.tracks()[0]] == [12] * 4 and [t.born for t in tracker.tracks()[0]] == [0] * 4
    hist, _ = ids_per_person("cross")
    assert hist[0][0] == hist[1][0] == {0: 0, 1: 1}
    hist, tracker = ids_per_person("occlusion")
    assert hist[-1][0][0] == hist[0][0][0] and hist[-1][0][1] == 3 and tracker.state()["deaths"] == 1
    hist, tracker = ids_per_person("overflow")
    assert sorted(hist[0][0].values()) == [-1, -1, 0, 1, 2, 3] and tracker.state()["overflow"] == 6
    assert ids_per_person("gate_on")[0][1][0] == {0: 0} and ids_per_person("gate_off")[0][1][0] == {0: 1}
    hist, tracker = ids_per_person("nan_pose")
    assert hist[2][0][1] == 2 and hist[3][0] == hist[0][0] and tracker.state()["deaths"] == 1 and len(tracker.tracks()[0]) == 2
    hist, _ = ids_per_person("min_hits")
    assert set(hist[0][0].values()) == set(hist[1][0].values()) == {-1} and sorted(hist[2][0].values()) == [0, 1, 2, 3]
    hist, tracker = ids_per_person("two_streams")
    assert hist[-1][0] == hist[0][0] and hist[-1][1] == {0: 0, 1: 1} and [len(t) for t in tracker.tracks()] == [3, 2]
    hist, tracker = ids_per_person("crowd")
    assert tracker.state()["dropped"] == 12 and hist[1][0] == {k: (k if k < 64 else -1) for k in range(70)}


def test_two_runs_give_the_same_bits_and_reset_starts_over():
    a, tracker = _device_run("walk")
    b, _ = _device_run("walk")
    assert all(x[k].tobytes() == y[k].tobytes() for x, y in zip(a, b) for k in STATE_KEYS)
    tracker.reset()
    fresh = ops.track_buffers(1, 8, 15, 8, DEV)
    assert all(torch.equal(tracker.buffers[k], fresh[k]) for k in fresh)
    seq = TC.float_sequences()["walk"]
    dets, count = seq["frames"][0]
    tracker.update(torch.from_numpy(dets).to(DEV), torch.from_numpy(count).to(DEV))
    assert all(_live_only({k: t.cpu().numpy() for k, t in tracker.buffers.items()})[k].tobytes() == a[0][k].tobytes() for k in STATE_KEYS)


def test_update_is_capturable_and_synchronisation_free():
    """the update in a HIP graph of its own: three replays on new static inputs equal three eager updates"""
    seq = TC.float_sequences()["walk"]
    want = _reference_run("walk")
    tracker = PoseTracker(batch=1, rows=8, num_joints=15, max_tracks=8, max_misses=2, device=DEV)
    dets = torch.from_numpy(seq["frames"][0][0]).to(DEV)
    count = torch.from_numpy(seq["frames"][0][1]).to(DEV)
    saved = tracker.snapshot()
    tracker.update(dets, count)                               # warm-up outside the capture
    tracker.restore(saved)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tracker.update(dets, count)
    assert tracker.state() == dict.fromkeys(ops.TRACK_STATE, 0)            # a capture runs nothing
    for f in range(3):
        dets.copy_(torch.from_numpy(seq["frames"][f][0]))
        count.copy_(torch.from_numpy(seq["frames"][f][1]))
        graph.replay()
        torch.cuda.synchronize()
        got = _live_only({k: t.cpu().numpy() for k, t in tracker.buffers.items()})
        assert all(got[k].tobytes() == want[f][k].tobytes() for k in STATE_KEYS), f


def test_tracker_refusals():
    with pytest.raises(_lib.MvgError):
        PoseTracker(batch=1, rows=8, max_tracks=65, device=DEV)
    with pytest.raises(_lib.MvgError):
        PoseTracker(batch=1, rows=8, num_joints=33, device=DEV)
    tracker = PoseTracker(batch=1, rows=8, device=DEV)
    dets = torch.zeros((1, 8, 15, 5), device=DEV)
    with pytest.raises(RuntimeError, match="float32"):
        tracker.update(dets.double())
    with pytest.raises(RuntimeError, match="contiguous"):
        tracker.update(torch.zeros((1, 8, 15, 10), device=DEV)[..., ::2])
    with pytest.raises(RuntimeError, match="track_buffers"):
        tracker.update(torch.zeros((1, 9, 15, 5), device=DEV))
    with pytest.raises(RuntimeError, match="count"):
        tracker.update(dets, torch.zeros((1, 2), dtype=torch.int64, device=DEV))
    with pytest.raises(_lib.MvgError):
        ops.track_update(dets, None, tracker.buffers, max_dist=float("nan"))
    with pytest.raises(_lib.MvgError):
        ops.track_update(dets, None, tracker.buffers, max_dist=-1.0)
    assert tracker.state()["frames"] == 0                                   # nothing was launched
