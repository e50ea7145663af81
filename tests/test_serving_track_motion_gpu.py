"""serving.GraphedDecoder(tracking=dict(..., motion=...)) and validate --device-track-motion: predict, update and correct behind the
NMS inside the captured graph.  mini5, 2 layers, valid_fraction 0.5, bf16, threshold 0.02 as in tests/test_serving_track_gpu.py."""
import pytest
import torch

from mvgformer_amd import ops
from mvgformer_amd.synthetic import build_case
from mvgformer_amd.tracking import PoseTracker

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THRESHOLD = 0.02
PANOPTIC = "configs/panoptic/knn5-lr4-q1024-g8.yaml"
MOTION = dict(dt=1.0, q=16.0, r=900.0)
TRACKING = dict(max_tracks=8, max_dist=500.0, max_misses=1, min_hits=2)


def _state(tracker):
    return {**tracker.buffers, **tracker.motion_buffers}


def _bits(t):
    """floating-point tensors as integers of their width: the comparison is of bits"""
    return t.view(torch.int64) if t.dtype == torch.float64 else t.view(torch.int32) if t.dtype == torch.float32 else t


def test_motion_in_the_graph_equals_an_eager_tracker():
    """five replays with new maps: track_ids, track_poses and every state buffer bit-equal to a second, eager
    PoseTracker(motion=...) fed clones of runner.detections after every replay; one graph; decoder outputs and detections
    bit-equal to a runner without motion; the capture's warm-up forwards leave the motion state as it was"""
    from mvgformer_amd.factory import build_decoder_for_case, case_to_device
    from mvgformer_amd.serving import GraphedDecoder
    from tests.test_serving_nms_gpu import _clone, _eq
    cases = [case_to_device(build_case("mini5", seed=s, layers=2, valid_fraction=0.5), DEV) for s in (4, 3)]
    dec = build_decoder_for_case(cases[0], DEV, dtype=torch.bfloat16)
    c = cases[0]
    args = (dec, c.meta, c.spatial_shapes, c.level_start_index)
    pp = dict(dist_thr=0.3, num_nearby_joints_thr=7)
    plain = GraphedDecoder(*args, batch=1, num_queries=c.NQ, threshold=THRESHOLD, postprocess=pp, tracking=TRACKING)
    runner = GraphedDecoder(*args, batch=1, num_queries=c.NQ, threshold=THRESHOLD, postprocess=pp,
                            tracking=dict(TRACKING, motion=MOTION))
    assert plain.track_poses is None and plain.tracker.motion_buffers is None
    assert runner.tracker.motion_params == dict(dt=1.0, q=16.0, r=900.0, v0=2500.0)
    assert runner.track_poses is runner.tracker.row_poses and tuple(runner.track_poses.shape) == (1, c.NQ, 15, 3)
    eager = PoseTracker(batch=1, rows=c.NQ, num_joints=15, device=DEV, motion=MOTION, **TRACKING)
    graphs = set()
    for i, c in enumerate((cases * 3)[:5]):                                   # frames alternate, no re-capture
        for run in (plain, runner):
            run.set_cameras(c.meta)
            run.load(src_views=c.src_views, tgt=c.tgt, query_pos=c.query_pos, reference_points=c.reference_points)
        if runner.graph is None:
            before = runner.tracker.snapshot()
            assert set(before) == set(_state(runner.tracker))
            runner.capture()
            torch.cuda.synchronize()
            assert all(torch.equal(before[k], t) for k, t in _state(runner.tracker).items())
            assert runner.tracker.state() == dict.fromkeys(ops.TRACK_STATE, 0) and runner.tracker.motion() == [{}]
            assert float(runner.track_poses.abs().sum()) == 0.0
        want_out = _clone(plain.replay())
        got_out = runner.replay()
        graphs.add(id(runner.graph))
        torch.cuda.synchronize()
        assert _eq(got_out, want_out), i
        dets, count, _ = runner.detections
        assert torch.equal(dets, plain.detections[0]) and torch.equal(count, plain.detections[1])
        ids, slots = eager.update(dets.clone(), count.clone())
        assert torch.equal(runner.track_ids[0], ids) and torch.equal(runner.track_ids[1], slots), i
        assert torch.equal(_bits(runner.track_poses), _bits(eager.row_poses)), i
        assert all(torch.equal(_bits(t), _bits(_state(eager)[k])) for k, t in _state(runner.tracker).items()), i
        k = int(count[0, 0])
        has = slots[0] >= 0
        assert int(has[k:].sum()) == 0 and float(runner.track_poses[0][~has].abs().sum()) == 0.0
        live = runner.tracker.buffers["pose"][0][slots[0][has].long()]         # a row with a track: the slot's pose
        assert torch.equal(runner.track_poses[0][has], live)
        pinned = [p.data_ptr() for p in runner._pinned]
        assert all(t.data_ptr() in pinned for t in _state(runner.tracker).values())
    assert len(graphs) == 1 and eager.state()["matches"] >= 2
    assert eager.state()["frames"] == 5 and runner.tracker.state() == eager.state()
    # eager() takes the same path as the capture
    runner.tracker.reset()
    second = PoseTracker(batch=1, rows=c.NQ, num_joints=15, device=DEV, motion=MOTION, **TRACKING)
    for c in cases:
        runner.set_cameras(c.meta)
        runner.load(src_views=c.src_views, tgt=c.tgt, query_pos=c.query_pos, reference_points=c.reference_points)
        runner.eager()
        second.update(runner.detections[0].clone(), runner.detections[1].clone())
    assert all(torch.equal(_bits(t), _bits(_state(second)[k])) for k, t in _state(runner.tracker).items())


def test_motion_is_the_one_new_tracking_key():
    from mvgformer_amd.factory import build_decoder_for_case, case_to_device
    from mvgformer_amd.serving import GraphedDecoder
    c = case_to_device(build_case("mini5", seed=4, layers=2, with_features=False), DEV)
    dec = build_decoder_for_case(c, DEV, dtype=torch.bfloat16)
    args = (dec, c.meta, c.spatial_shapes, c.level_start_index, 1, c.NQ, 0.1)
    with pytest.raises(TypeError, match="unknown tracking keys"):
        GraphedDecoder(*args, postprocess=dict(), tracking=dict(max_tracks=8, motion_model="kalman"))
    with pytest.raises(TypeError, match="unknown tracking keys"):
        GraphedDecoder(*args, postprocess=dict(), tracking=dict(motion=True, dt=1.0))
    with pytest.raises(TypeError, match="unknown motion keys"):
        GraphedDecoder(*args, postprocess=dict(), tracking=dict(motion=dict(model="kalman")))
    with pytest.raises(ValueError, match="requires postprocess"):
        GraphedDecoder(*args, tracking=dict(motion=True))
    runner = GraphedDecoder(*args, postprocess=dict(), tracking=dict(motion=True))
    assert runner.tracker.motion_params == dict(dt=1.0, q=25.0, r=400.0, v0=2500.0) and runner.track_poses is not None
    assert GraphedDecoder(*args, postprocess=dict(), tracking=dict()).track_poses is None
    assert GraphedDecoder(*args, postprocess=dict(), tracking=dict(motion=None)).tracker.motion_buffers is None


@pytest.mark.parametrize("graph", [1, 0])
def test_validate_reports_the_motion_model(graph):
    from mvgformer_amd import validate
    rep = validate.main(["--cfg", "extract:" + PANOPTIC, "--device-nms", "1", "--device-track", "1", "--device-track-motion", "1",
                         "--frames", "4", "--graph", str(graph)])
    assert rep["device_track"] is True and rep["device_track_motion"] is True
    for row in rep["results"]:
        print(row)
        assert row["frames"] == 4 and row["hip_graph"] is bool(graph)
        assert set(row["tracks"]) == {"births", "deaths", "overflow", "dropped", "active"}
        assert row["track_motion"]["tracks"] == row["tracks"]["active"] and row["track_motion"]["mean_speed"] >= 0.0
