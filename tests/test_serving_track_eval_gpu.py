"""serving.GraphedDecoder(tracking=..., track_evaluation=...): the scoring of the track ids right behind the tracker inside the
captured graph.  mini5, 2 layers, valid_fraction 0.5, bf16, threshold 0.02: the smallest runner shape of
tests/test_serving_track_gpu.py.  The ground truth is the first frame's own kept poses, so that there is something to match."""
import pytest
import torch

from mvgformer_amd import ops
from mvgformer_amd.synthetic import build_case
from mvgformer_amd.tracking import TrackEvaluator

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THRESHOLD = 0.02
TRACKING = dict(max_tracks=8, max_dist=500.0, max_misses=1, min_hits=1)
SCORING = dict(dist_thr=500.0, max_persons=4, max_ids=64)


def _feed(run, c, truth=None):
    run.set_cameras(c.meta)
    run.load(src_views=c.src_views, tgt=c.tgt, query_pos=c.query_pos, reference_points=c.reference_points, ground_truth=truth)


def test_track_evaluation_in_the_graph_equals_eager_and_changes_nothing_else():
    """five replays with alternating maps, one of them without annotation: decoder outputs, detections and track ids bit-equal to
    a runner without track_evaluation; the capture's warm-up forwards count no frame; the same frames through eager() give the
    same report"""
    from mvgformer_amd.factory import build_decoder_for_case, case_to_device
    from mvgformer_amd.serving import GraphedDecoder
    from tests.test_serving_nms_gpu import _clone, _eq
    cases = [case_to_device(build_case("mini5", seed=s, layers=2, valid_fraction=0.5), DEV) for s in (4, 3)]
    dec = build_decoder_for_case(cases[0], DEV, dtype=torch.bfloat16)
    c = cases[0]
    args = (dec, c.meta, c.spatial_shapes, c.level_start_index)
    pp = dict(dist_thr=0.3, num_nearby_joints_thr=7)
    plain = GraphedDecoder(*args, batch=1, num_queries=c.NQ, threshold=THRESHOLD, postprocess=pp, tracking=TRACKING)
    runner = GraphedDecoder(*args, batch=1, num_queries=c.NQ, threshold=THRESHOLD, postprocess=pp, tracking=TRACKING,
                            track_evaluation=SCORING)
    assert plain.track_evaluator is None and plain.person_id is None
    assert isinstance(runner.track_evaluator, TrackEvaluator) and runner.track_evaluator.max_ids == 64
    assert tuple(runner.ground_truth[0].shape) == (1, 4, 15, 3) and runner.person_id.tolist() == [[0, 1, 2, 3]]
    with pytest.raises(ValueError, match="ground_truth needs"):               # neither evaluation nor track_evaluation
        plain.load(ground_truth=runner.ground_truth)
    # the ground truth: the kept poses of the first frame
    _feed(plain, c)
    plain.capture().replay()
    torch.cuda.synchronize()
    G = min(int(plain.detections[1][0, 0]), 3)
    assert G >= 2
    j3d = plain.detections[0][:, :G, :, :3].clone()
    vis = torch.ones((1, G, 15), device=DEV)
    plain.tracker.reset()

    def truth(i):
        return j3d, vis, torch.tensor([-1 if i == 3 else G], dtype=torch.int32, device=DEV)

    frames = (cases * 3)[:5]
    for i, c in enumerate(frames):
        _feed(plain, c)
        _feed(runner, c, truth(i))
        if runner.graph is None:
            runner.capture()
            torch.cuda.synchronize()
            assert runner.track_evaluator.state() == dict.fromkeys(ops.TRACK_EVAL_STATE, 0)      # the warm-up counted no frame
            assert int(runner.track_evaluator.buffers["last_track"].max()) == -1
            assert runner.tracker.state() == dict.fromkeys(ops.TRACK_STATE, 0)
        want_out = _clone(plain.replay())
        got_out = runner.replay()
        torch.cuda.synchronize()
        assert _eq(got_out, want_out), i
        assert all(torch.equal(a, b) for a, b in zip(runner.detections, plain.detections)), i
        assert all(torch.equal(a, b) for a, b in zip(runner.track_ids, plain.track_ids)), i
    pinned = [p.data_ptr() for p in runner._pinned]
    assert all(t.data_ptr() in pinned for t in runner.track_evaluator.buffers.values()) and runner.person_id.data_ptr() in pinned
    replayed = runner.track_evaluator.report()
    total = replayed["total"]
    print(total)
    assert total["frames"] == 4 and total["gt"] == 4 * G                       # frame 3 has no annotation
    assert total["matches"] >= 2 * G and total["matches"] + total["misses"] == total["gt"]
    assert total["matches"] + total["false_pos"] == total["hyp"] and total["idtp"] <= total["matches"]
    assert runner.tracker.state() == plain.tracker.state()
    # eager() takes the same path as the capture
    runner.tracker.reset()
    runner.track_evaluator.reset()
    for i, c in enumerate(frames):
        _feed(runner, c, truth(i))
        runner.eager()
    assert runner.track_evaluator.report() == replayed


def test_track_evaluation_needs_tracking_and_known_keys():
    from mvgformer_amd.factory import build_decoder_for_case, case_to_device
    from mvgformer_amd.serving import GraphedDecoder
    c = case_to_device(build_case("mini5", seed=4, layers=2, with_features=False), DEV)
    dec = build_decoder_for_case(c, DEV, dtype=torch.bfloat16)
    args = (dec, c.meta, c.spatial_shapes, c.level_start_index, 1, c.NQ, 0.1)
    with pytest.raises(ValueError, match="requires tracking"):
        GraphedDecoder(*args, postprocess=dict(), track_evaluation=dict())
    with pytest.raises(TypeError, match="unknown track_evaluation keys"):
        GraphedDecoder(*args, postprocess=dict(), tracking=dict(), track_evaluation=dict(metric="hota"))
    with pytest.raises(ValueError, match="below the 10 person slots"):
        GraphedDecoder(*args, postprocess=dict(), tracking=dict(), evaluation=dict(kind="panoptic", capacity=64),
                       track_evaluation=dict(max_persons=4))
    both = GraphedDecoder(*args, postprocess=dict(), tracking=dict(), evaluation=dict(kind="panoptic", capacity=64),
                          track_evaluation=dict())
    assert both.track_evaluator.max_persons == 10 and tuple(both.person_id.shape) == (1, 10)     # one set of buffers for both
    with pytest.raises(ValueError, match="person_id needs"):
        GraphedDecoder(*args, postprocess=dict(), evaluation=dict(kind="panoptic", capacity=64)).load(
            ground_truth=(*both.ground_truth, both.person_id))
    runner = GraphedDecoder(*args, postprocess=dict(), tracking=dict(), track_evaluation=dict())
    assert runner.track_evaluator.max_persons == 10 and runner.track_evaluator.dist_thr == 500.0
    ids = torch.tensor([[3, 1]], dtype=torch.int32, device=DEV)
    runner.load(ground_truth=(both.ground_truth[0][:, :2], both.ground_truth[1][:, :2], both.ground_truth[2], ids))
    assert runner.person_id[0, :3].tolist() == [3, 1, 2]
    runner.load(ground_truth=both.ground_truth)
    assert runner.person_id[0].tolist() == list(range(10))


def test_validate_reports_the_tracking_scores(tmp_path_factory):
    """--device-track-eval 1 on the small Panoptic rig of tests/test_eval_device_gpu.py (two frames, ground truth = the first kept
    poses moved by 15 mm noise, the last person without a visible joint in frame 1): every person is matched, and the replayed
    graph and the eager launches report the same"""
    from mvgformer_amd import validate
    from tests.test_eval_device_gpu import _validate_rig
    args, _ = _validate_rig("panoptic", str(tmp_path_factory.getbasetemp() / "track_eval_panoptic"))
    rows = []
    for graph in (1, 0):
        rep = validate.main(args + ["--device-nms", "1", "--device-track", "1", "--device-track-eval", "1", "--graph", str(graph)])
        assert rep["device_track_eval"] is True and rep["results"][0]["hip_graph"] is bool(graph)
        rows.append(rep["results"][0]["device_track_eval"])
    print(rows[0])
    assert rows[0] == rows[1]
    s = rows[0]
    G = (s["gt"] + 1) // 2
    assert s["frames"] == 2 and s["gt"] in (3, 5) and s["bad_id"] == 0
    assert s["matches"] >= G and s["matches"] + s["misses"] == s["gt"]          # frame 0 has no pair to keep: all G are matched
    assert s["matches"] + s["false_pos"] == s["hyp"] and s["idtp"] <= s["matches"] and 0.0 < s["motp"] <= 500.0
    assert s["identities"] == (s["gt"] + 1) // 2 and s["mostly_lost"] == 0
    import numpy as np
    arrays = dict(np.load(args[3]))
    arrays["joints_3d"], arrays["joints_3d_vis"] = arrays["joints_3d"][:, :, :14], arrays["joints_3d_vis"][:, :, :14]
    short = str(tmp_path_factory.mktemp("track_eval_short") / "frames14.npz")
    np.savez(short, **arrays)
    with pytest.raises(SystemExit, match="14. joints, the kept poses 15"):      # ground truth of another joint format
        validate.main([args[0], args[1], args[2], short, *args[4:], "--device-nms", "1", "--device-track", "1",
                       "--device-track-eval", "1"])
    with pytest.raises(SystemExit, match="no frame has joints_3d"):             # synthetic frames carry no ground truth
        validate.main(["--cfg", args[1], "--frames", "2", "--device-nms", "1", "--device-track", "1", "--device-track-eval", "1"])
