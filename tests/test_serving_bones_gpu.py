"""serving.GraphedDecoder(tracking=..., refine=dict(bone_lengths="track")): the per-track bone-length estimate between the tracker
and the structural refiner, inside the decoder's HIP graph.  The rig of tests/test_serving_refine_gpu.py: mini5, 2 layers,
valid_fraction 0.5, bf16, threshold 0.02; the two frames alternate, so the tracks of one frame miss once and come back."""
import numpy as np
import pytest
import torch

from mvgformer_amd import ops
from mvgformer_amd.synthetic import build_case
from tests import bones_ref, st_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THRESHOLD = 0.02
PANOPTIC = "configs/panoptic/knn5-lr4-q1024-g8.yaml"
TRACKING = dict(max_tracks=8, max_dist=500.0, max_misses=1, min_hits=1)
LENGTHS = [180.0 + 15.0 * k for k in range(14)]
REFINE = dict(bone_lengths="track", window=3, min_frames=2, fallback=LENGTHS, n_steps=2)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _np_same(got, want):
    got, want = got.detach().cpu().numpy(), np.asarray(want)
    return got.dtype == want.dtype and np.array_equal(got.view(np.uint32) if got.dtype.kind == "f" else got,
                                                      want.view(np.uint32) if want.dtype.kind == "f" else want)


def _rig():
    from mvgformer_amd.factory import build_decoder_for_case, case_to_device
    cases = [case_to_device(build_case("mini5", seed=s, layers=2, valid_fraction=0.5), DEV) for s in (4, 3)]
    dec = build_decoder_for_case(cases[0], DEV, dtype=torch.bfloat16)
    c = cases[0]
    return cases, (dec, c.meta, c.spatial_shapes, c.level_start_index), dict(batch=1, num_queries=c.NQ, threshold=THRESHOLD,
                                                                             postprocess=dict(dist_thr=0.3, num_nearby_joints_thr=7))


def _load(run, c):
    run.set_cameras(c.meta)
    run.load(src_views=c.src_views, tgt=c.tgt, query_pos=c.query_pos, reference_points=c.reference_points)


def test_track_lengths_in_the_graph():
    from mvgformer_amd.geometry_torch import proj_matrices_from_records
    from mvgformer_amd.serving import GraphedDecoder
    from mvgformer_amd.structural import PANOPTIC15_PARENT, BoneLengthEstimator
    from tests.test_serving_nms_gpu import _clone, _eq
    cases, args, kw = _rig()
    NQ = kw["num_queries"]
    tracked = GraphedDecoder(*args, tracking=TRACKING, **kw)
    fine = GraphedDecoder(*args, tracking=TRACKING, refine=REFINE, **kw)
    assert tracked.bone_estimator is None and tracked.bone_source is None and tracked.bone_lengths is None
    est = fine.bone_estimator
    assert isinstance(est, BoneLengthEstimator) and (est.window, est.min_frames, est.max_tracks) == (3, 2, 8)
    assert fine.bone_lengths is est.row_length is fine.refiner.bone_lengths and fine.bone_source is est.row_source
    assert tuple(fine.bone_lengths.shape) == (1, NQ, 14) and tuple(fine.bone_source.shape) == (1, NQ)
    assert [type(s).__name__ for s, _ in fine.post.stages] == ["PoseTracker", "BoneLengthEstimator", "StructuralRefiner"]
    # the eager twins: the estimator's state on the device and in numpy, fed with the runner's own read-back after every replay
    twin = ops.track_bones_buffers(1, 8, 15, NQ, 3, DEV)
    fallback = torch.tensor(LENGTHS, dtype=torch.float32, device=DEV)
    restated = bones_ref.new_buffers(1, 8, 15, NQ, 3)
    graphs, sources, passes = set(), set(), []
    for rounds in range(2):
        seen_frames = []
        for i, c in enumerate((cases * 3)[:5]):
            for run in (tracked, fine):
                _load(run, c)
            if fine.graph is None:
                fine.capture()
                torch.cuda.synchronize()
                # the capture's warm-up forwards left no history
                assert not est.buffers["seen"].any() and bool((est.buffers["owner"] == -1).all()) and not est.buffers["hist"].any()
                assert fine.tracker.tracks() == [[]] and est.lengths() == [{}]
            want_out = _clone(tracked.replay())
            got_out = fine.replay()
            graphs.add(id(fine.graph))
            torch.cuda.synchronize()
            # decoder outputs, pred, detections and track ids: those of a runner with tracking but without refine
            assert _eq(got_out, want_out) and torch.equal(_bits(fine.pred), _bits(tracked.pred))
            assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(fine.detections, tracked.detections))
            assert all(torch.equal(a, b) for a, b in zip(fine.track_ids, tracked.track_ids))
            dets, count, keep = fine.detections
            # eager ops.track_bones + ops.structural_triangulate on the runner's own read-back
            length, source = ops.track_bones(dets.clone(), count.clone(), fine.tracker.buffers, PANOPTIC15_PARENT, twin, 2, fallback)
            ud, _ = ops.uncrop_undistort_jac(fine.outputs[2][-1], fine.ctx.cams, fine.V, 1)
            Pm = proj_matrices_from_records(fine.ctx.cams, fine.V, 1).contiguous()
            X, status = ops.structural_triangulate(ud, None, Pm, PANOPTIC15_PARENT, length, rows=keep[:, :NQ], count=count, n_steps=2)
            torch.cuda.synchronize()
            assert all(torch.equal(_bits(est.buffers[k]), _bits(twin[k])) for k in twin)
            assert torch.equal(_bits(fine.refined[0]), _bits(X)) and torch.equal(fine.refined[1], status)
            # and the restatements
            d, cnt = dets.cpu().numpy(), count.cpu().numpy()
            bones_ref.update(d, cnt, fine.track_ids[1].cpu().numpy(), fine.tracker.buffers["id"].cpu().numpy(), PANOPTIC15_PARENT,
                             restated, 2, np.array(LENGTHS, np.float32))
            assert all(_np_same(est.buffers[k], restated[k]) for k in bones_ref.STATE + bones_ref.OUTPUTS)
            ref_X, ref_s = st_ref.by_rows(ud.cpu().numpy(), None, Pm.cpu().numpy(), PANOPTIC15_PARENT, restated["row_length"],
                                          keep[:, :NQ].cpu().numpy(), cnt, method="ST", n_steps=2)
            assert _np_same(fine.refined[0], ref_X) and _np_same(fine.refined[1], ref_s)
            k = int(cnt[0, 0])
            src = fine.bone_source[0].cpu().numpy()
            print("round", rounds, "frame", i, "kept", k, "source", src[:k].tolist(), "status", fine.refined[1][0, :k].tolist())
            assert (src[k:] == -1).all() and (src[:k] >= 0).all()
            sources |= set(src[:k].tolist())
            seen_frames.append([t.clone() for t in (fine.refined[0], fine.refined[1], fine.bone_lengths, fine.bone_source)])
            assert all(t.data_ptr() in [p.data_ptr() for p in fine._pinned] for t in list(est.buffers.values()) + [est.fallback])
        passes.append(seen_frames)
        # one read-back of the histories: the live tracks' ids
        live = {t.id for t in fine.tracker.tracks()[0]}
        assert live and set(est.lengths()[0]) == live
        # a second pass over the same frames after a reset: identical bits
        for stage in (tracked.tracker, fine.tracker, est):
            stage.reset()
        for k, t in twin.items():
            t.fill_(-1 if k in ("owner", "row_source") else 0)
        restated = bones_ref.new_buffers(1, 8, 15, NQ, 3)
    assert len(graphs) == 1
    assert {0, 1} <= sources, sources                              # young tracks took the fallback, older ones their own median
    assert all(torch.equal(_bits(a), _bits(b)) for fa, fb in zip(*passes) for a, b in zip(fa, fb))


def test_lengths_from_values_launch_what_they_launched():
    """refine=dict(bone_lengths=<values>) next to the new mode: no estimator, the refiner alone behind the NMS, `refined` equal to
    an eager call, and the launches of one eager forward counted by their labels"""
    from mvgformer_amd.geometry_torch import proj_matrices_from_records
    from mvgformer_amd.serving import GraphedDecoder
    from mvgformer_amd.structural import PANOPTIC15_PARENT
    cases, args, kw = _rig()
    NQ = kw["num_queries"]
    fixed = GraphedDecoder(*args, tracking=TRACKING, refine=dict(bone_lengths=LENGTHS, n_steps=2), **kw)
    assert fixed.bone_estimator is None and fixed.bone_source is None and tuple(fixed.bone_lengths.shape) == (14,)
    assert [type(s).__name__ for s, _ in fixed.post.stages] == ["PoseTracker", "StructuralRefiner"]
    _load(fixed, cases[0])
    fixed.replay()
    torch.cuda.synchronize()
    dets, count, keep = fixed.detections
    ud, _ = ops.uncrop_undistort_jac(fixed.outputs[2][-1], fixed.ctx.cams, fixed.V, 1)
    Pm = proj_matrices_from_records(fixed.ctx.cams, fixed.V, 1).contiguous()
    X, status = ops.structural_triangulate(ud, None, Pm, PANOPTIC15_PARENT, torch.tensor(LENGTHS, device=DEV), rows=keep[:, :NQ],
                                           count=count, n_steps=2)
    torch.cuda.synchronize()
    assert torch.equal(_bits(fixed.refined[0]), _bits(X)) and torch.equal(fixed.refined[1], status) and int(count[0, 0]) > 0
    tracking = GraphedDecoder(*args, tracking=TRACKING, refine=REFINE, **kw)
    _load(tracking, cases[0])
    counts = {}
    for name, run in (("values", fixed), ("track", tracking)):
        run.eager()                                                # builds what the first forward builds
        torch.cuda.synchronize()
        ops.PROFILE = {}
        try:
            run.eager()
            torch.cuda.synchronize()
            counts[name] = {k: len(v) for k, v in ops.PROFILE.items()}
        finally:
            ops.PROFILE = None
    print(counts)
    assert "track_bones" not in counts["values"] and counts["track"].pop("track_bones") == 1
    assert counts["values"] == counts["track"] and counts["values"]["structural_triangulate"] == 1      # one launch more, no other


@pytest.mark.parametrize("graph", [1, 0])
def test_validate_track_lengths_reports_the_same_with_and_without_the_graph(graph):
    from mvgformer_amd import validate
    argv = ["--cfg", "extract:" + PANOPTIC, "--frames", "4", "--device-nms", "1", "--device-track", "1", "--device-refine", "1",
            "--bone-lengths", "track", "--bone-window", "3", "--bone-min-frames", "2"]
    rep = validate.main(argv + ["--graph", str(graph)])
    row = rep["results"][0]
    print(row)
    assert rep["device_refine"] is True and rep["bone_lengths"] == "track" and row["hip_graph"] is bool(graph)
    share = row["refine"]["length_source_share"]
    assert row["refine"]["kept_rows"] == row["poses_after_nms"] > 0 and set(share) == {"track", "fallback", "own"}
    assert abs(sum(share.values()) - 1.0) < 2e-4 and share["fallback"] == 0.0       # no --bone-fallback: young tracks use their own
    _SEEN[graph] = row["refine"]
    if len(_SEEN) == 2:
        assert _SEEN[0] == _SEEN[1]


_SEEN = {}
