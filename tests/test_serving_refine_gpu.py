"""serving.GraphedDecoder(refine=...): structural triangulation of the kept queries captured in the decoder's HIP graph behind the
NMS.  The rig of tests/test_serving_nms_gpu.py: mini5, 2 layers, valid_fraction 0.5, bf16, threshold 0.02 (seed 4 keeps 6 poses)."""
import numpy as np
import pytest
import torch

from mvgformer_amd.synthetic import build_case
from tests import st_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THRESHOLD = 0.02
LENGTHS = [180.0 + 15.0 * k for k in range(14)]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _eq(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[:4], b[:4])) and all(torch.equal(x, y) for x, y in zip(a[4], b[4]))


def _clone(o):
    return [t.clone() for t in o[:4]] + [[p.clone() for p in o[4]]]


def _restated(run, lengths):
    """st_ref on the runner's own read-back: the last layer's 2D points un-cropped on the device, keep and count, and projection
    matrices computed HERE from the camera records (not the runner's static copy: a stale copy must show)"""
    from mvgformer_amd import ops
    from mvgformer_amd.geometry_torch import proj_matrices_from_records
    from mvgformer_amd.structural import PANOPTIC15_PARENT
    B, V = run.tgt.shape[0], run.V
    ud, _ = ops.uncrop_undistort_jac(run.outputs[2][-1], run.ctx.cams, V, B)
    _, count, keep = run.detections
    rows = keep[:, :run.refined[0].shape[1]]
    Pm = proj_matrices_from_records(run.ctx.cams, V, B).contiguous()
    eager = ops.structural_triangulate(ud, None, Pm, PANOPTIC15_PARENT, torch.tensor(lengths, dtype=torch.float32, device=DEV),
                                       rows=rows, count=count, n_steps=run.refiner.n_steps, method=run.refiner.method)
    torch.cuda.synchronize()
    want = st_ref.by_rows(ud.cpu().numpy(), None, Pm.cpu().numpy(), PANOPTIC15_PARENT, np.array(lengths, np.float32),
                          rows.cpu().numpy(), count.cpu().numpy(), method=run.refiner.method, n_steps=run.refiner.n_steps)
    return eager, want


def test_refine_in_the_graph():
    from mvgformer_amd.factory import build_decoder_for_case, case_to_device
    from mvgformer_amd.geometry_torch import proj_matrices_from_records
    from mvgformer_amd.serving import GraphedDecoder
    cases = [case_to_device(build_case("mini5", seed=s, layers=2, valid_fraction=0.5), DEV) for s in (4, 3)]
    dec = build_decoder_for_case(cases[0], DEV, dtype=torch.bfloat16)
    c = cases[0]
    args = (dec, c.meta, c.spatial_shapes, c.level_start_index)
    pp = dict(dist_thr=0.3, num_nearby_joints_thr=7)
    plain = GraphedDecoder(*args, batch=1, num_queries=c.NQ, threshold=THRESHOLD, postprocess=pp)
    fine = GraphedDecoder(*args, batch=1, num_queries=c.NQ, threshold=THRESHOLD, postprocess=pp,
                          refine=dict(bone_lengths=LENGTHS, n_steps=3))
    assert plain.refined is None and plain.refiner is None and plain.bone_lengths is None
    poses, status = fine.refined
    assert tuple(poses.shape) == (1, c.NQ, 15, 3) and tuple(status.shape) == (1, c.NQ) and tuple(fine.bone_lengths.shape) == (14,)
    graphs, solved, pm_ptr, pm_seen = set(), 0, fine.post.Pm.data_ptr(), []
    for i, c in enumerate(cases):
        for run in (plain, fine):
            run.set_cameras(c.meta)
            run.load(src_views=c.src_views, tgt=c.tgt, query_pos=c.query_pos, reference_points=c.reference_points)
        # set_cameras refilled the static projection matrices in place
        assert torch.equal(fine.post.Pm, proj_matrices_from_records(fine.ctx.cams, fine.V, 1)) and fine.post.Pm.data_ptr() == pm_ptr
        pm_seen.append(fine.post.Pm.clone())
        want_out = _clone(plain.replay())
        want_pred, want_dets = plain.pred.clone(), [t.clone() for t in plain.detections]
        got_out = fine.replay()
        graphs.add(id(fine.graph))
        torch.cuda.synchronize()
        # the decoder's outputs, pred and the detections are those of a runner without refine, bit for bit
        assert _eq(got_out, want_out) and torch.equal(_bits(fine.pred), _bits(want_pred))
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(fine.detections, want_dets))
        assert all(t.data_ptr() in [p.data_ptr() for p in fine._pinned] for t in (poses, status, fine.bone_lengths, fine.post.Pm))
        k = int(fine.detections[1][0, 0])
        first = (poses.clone(), status.clone())
        (eager_X, eager_s), (ref_X, ref_s) = _restated(fine, LENGTHS)
        print("frame", i, "kept", k, "status", status[0, :k].tolist())
        assert torch.equal(_bits(first[0]), _bits(eager_X)) and torch.equal(first[1], eager_s)
        assert np.array_equal(first[0].cpu().numpy().view(np.uint32), ref_X.view(np.uint32)) and np.array_equal(first[1].cpu().numpy(), ref_s)
        assert bool((status[0, k:] == -1).all()) and bool((status[0, :k] >= 0).all()) and not bool(poses[0, k:].any())
        solved += int((status[0, :k] == 0).sum())
        # a second replay of the same frame: the same bits
        fine.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(poses), _bits(first[0])) and torch.equal(status, first[1])
        # new lengths in the static tensor: the next replay solves for them, the graph is the same object
        longer = [v + 40.0 for v in LENGTHS]
        fine.bone_lengths.copy_(torch.tensor(longer, device=DEV))
        fine.replay()
        graphs.add(id(fine.graph))
        torch.cuda.synchronize()
        _, (ref_X2, ref_s2) = _restated(fine, longer)
        assert np.array_equal(poses.cpu().numpy().view(np.uint32), ref_X2.view(np.uint32)) and np.array_equal(status.cpu().numpy(), ref_s2)
        if k:
            assert not torch.equal(_bits(poses), _bits(first[0]))
        fine.bone_lengths.copy_(torch.tensor(LENGTHS, device=DEV))
    assert len(graphs) == 1
    assert not torch.equal(pm_seen[0], pm_seen[1])              # the two frames have different cameras: Pm did follow set_cameras
    assert solved >= 2, solved                                  # the comparison is not vacuous


def test_refine_argument_refusals():
    from mvgformer_amd.factory import build_decoder_for_case, case_to_device
    from mvgformer_amd.serving import GraphedDecoder
    c = case_to_device(build_case("mini5", seed=4, layers=2, with_features=False), DEV)
    dec = build_decoder_for_case(c, DEV, dtype=torch.bfloat16)
    args = (dec, c.meta, c.spatial_shapes, c.level_start_index, 1, c.NQ, 0.1)
    with pytest.raises(ValueError, match="requires postprocess"):
        GraphedDecoder(*args, refine=dict(bone_lengths=LENGTHS))
    with pytest.raises(TypeError, match="unknown refine keys"):
        GraphedDecoder(*args, postprocess={}, refine=dict(bone_lengths=LENGTHS, steps=3))
    with pytest.raises(ValueError, match="convert_joint_format_indices"):
        GraphedDecoder(*args, postprocess={}, refine=dict(bone_lengths=LENGTHS), convert_joint_format_indices=list(range(14)))
    with pytest.raises(ValueError, match="bone lengths"):
        GraphedDecoder(*args, postprocess={}, refine=dict(bone_lengths=LENGTHS[:3]))
    with pytest.raises(RuntimeError, match="n_steps"):
        GraphedDecoder(*args, postprocess={}, refine=dict(bone_lengths=LENGTHS, n_steps=9))


@pytest.mark.parametrize("graph", [1, 0])
def test_validate_device_refine_reports_the_same_with_and_without_the_graph(graph, tmp_path):
    """validate.main --device-refine 1: the refiner inside the HIP graph (--graph 1) and behind the eager head (--graph 0) solve the same
    rows to the same bits, so the rounded figures of the report are equal; every kept row is one the solver was given"""
    from mvgformer_amd import validate
    path = str(tmp_path / "lengths.npy")
    np.save(path, np.array(LENGTHS, np.float32))
    argv = ["--cfg", "extract:configs/panoptic/knn5-lr4-q1024-g8.yaml", "--frames", "2", "--device-nms", "1", "--device-refine", "1",
            "--bone-lengths", path]
    rep = validate.main(argv + ["--graph", str(graph)])
    row = rep["results"][0]
    print(row)
    assert rep["device_refine"] is True and row["hip_graph"] is bool(graph)
    assert row["refine"]["kept_rows"] == row["poses_after_nms"] > 0 and 0.0 < row["refine"]["solved_share"] <= 1.0
    _SEEN[graph] = row["refine"]
    if len(_SEEN) == 2:
        assert _SEEN[0] == _SEEN[1]
    with pytest.raises(SystemExit):
        validate.main(argv[:4] + ["--device-refine", "1", "--bone-lengths", path])          # without --device-nms 1


_SEEN = {}
