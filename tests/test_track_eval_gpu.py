"""mvg_track_eval on the device (csrc/track.hip -> ops.track_eval -> tracking.TrackEvaluator) against the plain-Python restatement
of tests/trackeval_ref.py, on the sequences of tests/trackeval_cases.py: ops.pose_nms-shaped inputs -> ops.track_update ->
ops.track_eval, frame by frame, the restatement driven by the DEVICE's own ids (and filtered poses, with the motion model).  Every
integer of the state equal -- last_track, counters, seen, covered, overlap -- and dist_sum bit-equal."""
import functools

import numpy as np
import pytest
import torch

from mvgformer_amd import _lib, ops
from mvgformer_amd.tracking import PoseTracker, TrackEvaluator
from tests import trackeval_cases as EC
from tests import trackeval_ref as ER

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("last_track", "counters", "dist_sum", "seen", "covered", "overlap")
BADARG = 10001                                 # MVG_E_BADARG


@functools.lru_cache(maxsize=None)
def _case(name):
    if name == "crowd":
        return EC.crowd()
    if name in ("moving_plain", "moving_motion"):
        return EC.moving(name == "moving_motion")
    return EC.cases()[name]


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _objects(case):
    B, R, J = case["frames"][0][0].shape[:3]
    tracker = PoseTracker(batch=B, rows=R, num_joints=J, max_tracks=case["T"], max_dist=case["max_dist"],
                          max_misses=case["max_misses"], min_hits=case["min_hits"], motion=True if case["motion"] else None,
                          device=DEV)
    scorer = TrackEvaluator(batch=B, max_persons=case["P"], max_ids=case["K"], dist_thr=case["dist_thr"], device=DEV)
    return tracker, scorer


def _device_run(name):
    """-> (per frame the scorer's buffers, per frame the tracker's ids, per frame its row_poses or None, the scorer)"""
    case = _case(name)
    tracker, scorer = _objects(case)
    snaps, ids, poses = [], [], []
    for f, ((dets, count), (j3d, vis, num, pid)) in enumerate(zip(case["frames"], case["truth"])):
        if f in case["clear_last"]:
            scorer.buffers["last_track"].fill_(-1)
        dets, count = _dev(dets), _dev(count)
        tracker.update(dets, count)
        scorer.update(tracker, dets, count, _dev(j3d), _dev(vis), _dev(num), _dev(pid))
        snaps.append({k: t.cpu().numpy() for k, t in scorer.buffers.items()})
        ids.append(tracker.buffers["ids"].cpu().numpy())
        poses.append(None if tracker.row_poses is None else tracker.row_poses.cpu().numpy())
    return snaps, ids, (poses if case["motion"] else None), scorer


def _assert_equal(got, want, what):
    for f, (g, w) in enumerate(zip(got, want)):
        for k in KEYS:
            assert g[k].dtype == w[k].dtype and g[k].shape == w[k].shape, (what, f, k)
            assert g[k].tobytes() == w[k].tobytes(), (what, f, k, g[k], w[k])


NAMES = sorted(EC.cases()) + ["moving_plain", "moving_motion", "crowd"]


@pytest.mark.parametrize("name", NAMES)
def test_scores_equal_the_restatement_frame_by_frame(name):
    """every case, B = 2 with uneven streams, count = None, row_pose from the motion tracker and the full size among them"""
    got, ids, poses, scorer = _device_run(name)
    want = ER.run(_case(name), ids, poses)
    _assert_equal(got, want, name)
    st = scorer.state()
    assert st == ER.counters(want[-1]) and st["reserved"] == 0
    print(name, st, "dist_sum", got[-1]["dist_sum"].tolist())


def test_what_the_cases_are_for():
    """the known answers of tests/test_track_eval_cpu.py, read from the device through TrackEvaluator.report"""
    rep = _device_run("perfect")[3].report()["total"]
    assert (rep["matches"], rep["kept"], rep["misses"], rep["false_pos"], rep["switches"]) == (24, 21, 0, 0, 0)
    assert rep["mota"] == 1.0 and rep["idf1"] == 1.0 and (rep["mostly_tracked"], rep["mostly_lost"]) == (3, 0)
    rep = _device_run("occlusion")[3].report()["total"]
    assert (rep["misses"], rep["switches"], rep["false_pos"], rep["idtp"]) == (5, 1, 0, 18)
    assert rep["mota"] == 0.75 and rep["idf1"] == 36.0 / 43.0
    rep = _device_run("min_hits")[3].report()["total"]
    assert (rep["unreported"], rep["misses"], rep["false_pos"]) == (6, 6, 0) and rep["idf1"] == 36.0 / 42.0
    rep = _device_run("ghost")[3].report()["total"]
    assert rep["false_pos"] == 3 and rep["idf1"] == 48.0 / 51.0
    assert _device_run("kept_pairs")[3].report()["total"]["switches"] == 0
    assert _device_run("kept_pairs")[0][1]["last_track"][0].tolist() == [0, 1]
    assert _device_run("kept_pairs_cleared")[0][1]["last_track"][0].tolist() == [1, 0]
    assert _device_run("contested")[0][2]["last_track"][0].tolist() == [0, 1]
    on, off = _device_run("threshold_on")[3].report()["total"], _device_run("threshold_off")[3].report()["total"]
    assert (on["matches"], on["dist_sum"]) == (1, 512.0) and (off["misses"], off["false_pos"]) == (1, 1)
    small = _device_run("small_table")[3].report()
    assert small["total"]["idf1"] is None and small["max_ids_needed"] == 4 and small["total"]["mota"] == 0.75
    crowd = _device_run("crowd")[3].report()["total"]
    assert (crowd["gt"], crowd["hyp"], crowd["matches"], crowd["kept"], crowd["idtp"]) == (128, 128, 128, 64, 128)
    two = _device_run("two_streams")[3].report()
    assert [s["frames"] for s in two["streams"]] == [5, 4] and two["total"]["frames"] == 9


def test_two_runs_give_the_same_bits_and_reset_starts_over():
    a, _, _, scorer = _device_run("occlusion")
    b = _device_run("occlusion")[0]
    _assert_equal(a, b, "twice")
    saved = scorer.snapshot()
    scorer.reset()
    fresh = ops.track_eval_buffers(1, 4, 16, DEV)
    assert all(torch.equal(scorer.buffers[k], fresh[k]) for k in fresh)
    scorer.restore(saved)
    assert all(scorer.buffers[k].cpu().numpy().tobytes() == a[-1][k].tobytes() for k in KEYS)


def test_the_three_op_chain_is_capturable():
    """ops.pose_nms -> track_update -> track_eval in one HIP graph, on the case whose person_id changes from frame to frame:
    the frames go in as packed predictions (the persons stand 1.5 m apart and come in descending score, so the NMS keeps every
    row where it is), the ground truth and person_id as static tensors; the replays over the sequence equal the eager run"""
    case = _case("identities")
    want = _device_run("identities")[0]
    tracker, scorer = _objects(case)
    pred = _dev(case["frames"][0][0])
    nms = ops.pose_nms_buffers(*pred.shape[:3], None, DEV)
    dets, count = nms["dets"], nms["count"]
    truth = [_dev(x) for x in case["truth"][0]]

    def forward():
        ops.pose_nms(pred, 0.3, 7, out=nms)
        tracker.update(dets, count)
        scorer.update(tracker, dets, count, *truth[:3], person_id=truth[3])

    t_saved, s_saved = tracker.snapshot(), scorer.snapshot()
    forward()                                                                   # warm-up outside the capture
    tracker.restore(t_saved)
    scorer.restore(s_saved)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        forward()
    assert scorer.state() == dict.fromkeys(ops.TRACK_EVAL_STATE, 0)             # a capture runs nothing
    for f, ((d, c), gt) in enumerate(zip(case["frames"], case["truth"])):
        pred.copy_(torch.from_numpy(d))
        for dst, src in zip(truth, gt):
            dst.copy_(torch.from_numpy(src))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(dets.cpu(), torch.from_numpy(d)) and torch.equal(count.cpu(), torch.from_numpy(c)), f
        got = {k: t.cpu().numpy() for k, t in scorer.buffers.items()}
        assert all(got[k].tobytes() == want[f][k].tobytes() for k in KEYS), f


def test_refusals():
    B, R, Jn, G = 1, 8, 15, 4
    dets = torch.zeros((B, R, Jn, 5), device=DEV)
    ids = torch.zeros((B, R), dtype=torch.int32, device=DEV)
    j3d, vis = torch.zeros((B, G, Jn, 3), device=DEV), torch.zeros((B, G, Jn), device=DEV)
    num = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    buf = ops.track_eval_buffers(B, G, 16, DEV)
    for P, K in ((65, 16), (4, 4097), (0, 16), (4, 0)):
        with pytest.raises(_lib.MvgError):
            ops.track_eval_buffers(B, P, K, DEV)
    with pytest.raises(_lib.MvgError):                                          # G = 4 > P = 2
        ops.track_eval(dets, None, ids, j3d, vis, num, ops.track_eval_buffers(B, 2, 16, DEV))
    with pytest.raises(_lib.MvgError):
        ops.track_eval(dets, None, ids, j3d, vis, num, buf, dist_thr=float("nan"))
    with pytest.raises(_lib.MvgError):
        ops.track_eval(dets, None, ids, j3d, vis, num, buf, dist_thr=-1.0)
    with pytest.raises(RuntimeError, match="ids"):
        ops.track_eval(dets, None, ids.long(), j3d, vis, num, buf)
    with pytest.raises(RuntimeError, match="row_pose"):
        ops.track_eval(dets, None, ids, j3d, vis, num, buf, row_pose=torch.zeros((B, R, Jn, 5), device=DEV))
    with pytest.raises(RuntimeError, match="person_id"):
        ops.track_eval(dets, None, ids, j3d, vis, num, buf, person_id=torch.zeros((B, G), dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError, match="track_eval_buffers"):
        ops.track_eval(torch.zeros((2, R, Jn, 5), device=DEV), None, ids.repeat(2, 1), j3d.repeat(2, 1, 1, 1), vis.repeat(2, 1, 1),
                       num.repeat(2), buf)
    with pytest.raises(ValueError, match="person slots"):
        TrackEvaluator(batch=1, max_persons=2, device=DEV).update(PoseTracker(batch=1, rows=R, device=DEV), dets, None, j3d, vis, num)
    # the C entry itself: shape limits -> MVG_E_BADARG, nothing launched
    lib = _lib.load()
    ptrs = [_lib.ptr(t) for t in (dets, None, ids, None, j3d, vis, num, None)]
    state = [_lib.ptr(buf[k]) for k in ("last_track", "counters", "dist_sum", "seen", "covered", "overlap")]
    for shape in ((1, R, Jn, G, 65, 16), (1, R, Jn, G, 2, 16), (1, R, Jn, G, G, 4097), (1, R, 33, G, G, 16), (0, R, Jn, G, G, 16)):
        assert lib.mvg_track_eval(*ptrs, *shape, 500.0, *state, None) == BADARG, shape
    torch.cuda.synchronize()
    assert int(buf["counters"].sum()) == 0
    ops.track_eval(dets, None, ids, j3d, vis, num, buf)                         # num_person = -1: launched, nothing counted
    torch.cuda.synchronize()
    assert int(buf["counters"].sum()) == 0 and int(buf["last_track"].max()) == -1
