"""serving.GraphedDecoder(tracking=...) and validate --device-track: the tracker update behind the NMS inside the captured graph.
mini5, 2 layers, valid_fraction 0.5, bf16, threshold 0.02 as in tests/test_serving_nms_gpu.py (at 0.1 nothing is a candidate)."""
import pytest
import torch

from mvgformer_amd import ops
from mvgformer_amd.synthetic import build_case
from mvgformer_amd.tracking import PoseTracker

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THRESHOLD = 0.02
PANOPTIC = "configs/panoptic/knn5-lr4-q1024-g8.yaml"
TRACKING = dict(max_tracks=8, max_dist=500.0, max_misses=1, min_hits=2)


def _same_tracks(a, b):
    assert [len(x) for x in a] == [len(x) for x in b]
    for ta, tb in zip(a[0], b[0]):
        assert ta[:6] == tb[:6] and ta.pose.tobytes() == tb.pose.tobytes()


def test_tracking_in_the_graph_equals_an_eager_tracker():
    """five replays with new maps: track_ids and the tracks equal those of a second, eager PoseTracker fed clones of
    runner.detections after every replay; one graph; decoder outputs and detections bit-equal to a runner without tracking; the
    capture's warm-up forwards leave the tracker's state as it was"""
    from mvgformer_amd.factory import build_decoder_for_case, case_to_device
    from mvgformer_amd.serving import GraphedDecoder
    from tests.test_serving_nms_gpu import _clone, _eq
    cases = [case_to_device(build_case("mini5", seed=s, layers=2, valid_fraction=0.5), DEV) for s in (4, 3)]
    dec = build_decoder_for_case(cases[0], DEV, dtype=torch.bfloat16)
    c = cases[0]
    args = (dec, c.meta, c.spatial_shapes, c.level_start_index)
    pp = dict(dist_thr=0.3, num_nearby_joints_thr=7)
    plain = GraphedDecoder(*args, batch=1, num_queries=c.NQ, threshold=THRESHOLD, postprocess=pp)
    runner = GraphedDecoder(*args, batch=1, num_queries=c.NQ, threshold=THRESHOLD, postprocess=pp, tracking=TRACKING)
    assert plain.tracker is None and plain.track_ids is None
    assert isinstance(runner.tracker, PoseTracker) and runner.tracker.max_tracks == 8 and runner.tracker.min_hits == 2
    assert runner.track_ids[0] is runner.tracker.buffers["ids"] and tuple(runner.track_ids[1].shape) == (1, c.NQ)
    eager = PoseTracker(batch=1, rows=c.NQ, num_joints=15, device=DEV, **TRACKING)
    graphs, births, lost = set(), 0, 0
    for i, c in enumerate((cases * 3)[:5]):                                   # frames alternate, no re-capture
        for run in (plain, runner):
            run.set_cameras(c.meta)
            run.load(src_views=c.src_views, tgt=c.tgt, query_pos=c.query_pos, reference_points=c.reference_points)
        if runner.graph is None:
            before = runner.tracker.snapshot()
            runner.capture()
            torch.cuda.synchronize()
            assert all(torch.equal(before[k], t) for k, t in runner.tracker.buffers.items())
            assert runner.tracker.state() == dict.fromkeys(ops.TRACK_STATE, 0) and runner.tracker.tracks() == [[]]
        want_out = _clone(plain.replay())
        got_out = runner.replay()
        graphs.add(id(runner.graph))
        torch.cuda.synchronize()
        assert _eq(got_out, want_out), i
        dets, count, _ = runner.detections
        assert torch.equal(dets, plain.detections[0]) and torch.equal(count, plain.detections[1])
        ids, slots = eager.update(dets.clone(), count.clone())
        assert torch.equal(runner.track_ids[0], ids) and torch.equal(runner.track_ids[1], slots), i
        _same_tracks(runner.tracker.tracks(), eager.tracks())
        assert runner.tracker.state() == eager.state() and eager.state()["frames"] == i + 1
        k = int(count[0, 0])
        assert int((slots[0, k:] >= 0).sum()) == 0 and int((slots[0, :k] >= 0).sum()) == k - (eager.state()["overflow"] - lost)
        lost = eager.state()["overflow"]
        births = eager.state()["births"]
        assert all(t.data_ptr() in [p.data_ptr() for p in runner._pinned] for t in runner.tracker.buffers.values())
    assert len(graphs) == 1 and births >= 2                                   # the frame of seed 4 keeps several poses
    assert eager.state()["matches"] >= 2                                       # the same two frames come back every other replay
    # eager() takes the same path as the capture
    runner.tracker.reset()
    second = PoseTracker(batch=1, rows=c.NQ, num_joints=15, device=DEV, **TRACKING)
    for c in cases:
        runner.set_cameras(c.meta)
        runner.load(src_views=c.src_views, tgt=c.tgt, query_pos=c.query_pos, reference_points=c.reference_points)
        runner.eager()
        second.update(runner.detections[0].clone(), runner.detections[1].clone())
    _same_tracks(runner.tracker.tracks(), second.tracks())
    assert runner.tracker.state() == second.state()


def test_tracking_needs_postprocess_and_known_keys():
    from mvgformer_amd.factory import build_decoder_for_case, case_to_device
    from mvgformer_amd.serving import GraphedDecoder
    c = case_to_device(build_case("mini5", seed=4, layers=2, with_features=False), DEV)
    dec = build_decoder_for_case(c, DEV, dtype=torch.bfloat16)
    args = (dec, c.meta, c.spatial_shapes, c.level_start_index, 1, c.NQ, 0.1)
    with pytest.raises(ValueError, match="requires postprocess"):
        GraphedDecoder(*args, tracking=dict(max_tracks=8))
    with pytest.raises(TypeError, match="unknown tracking keys"):
        GraphedDecoder(*args, postprocess=dict(), tracking=dict(max_tracks=8, motion_model="kalman"))
    assert GraphedDecoder(*args, postprocess=dict()).tracker is None
    assert GraphedDecoder(*args, postprocess=dict(), tracking=dict()).tracker.max_tracks == 32


@pytest.mark.parametrize("graph", [1, 0])
def test_validate_reports_the_tracker_counters(graph):
    from mvgformer_amd import validate
    rep = validate.main(["--cfg", "extract:" + PANOPTIC, "--device-nms", "1", "--device-track", "1", "--frames", "4",
                         "--graph", str(graph)])
    assert rep["device_track"] is True and rep["device_nms"] is True
    for row in rep["results"]:
        print(row)
        assert row["frames"] == 4 and row["hip_graph"] is bool(graph)
        assert set(row["tracks"]) == {"births", "deaths", "overflow", "dropped", "active"}
        assert row["tracks"]["births"] >= 0 and row["tracks"]["active"] == row["tracks"]["births"] - row["tracks"]["deaths"]
        assert row["tracks"]["births"] + row["tracks"]["overflow"] <= row["poses_after_nms"]
