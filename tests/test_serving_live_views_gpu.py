"""serving.GraphedDecoder(live_views=True): one runner, captured once, replayed for any subset of its cameras
(load(view_live=...): two small H2D copies into the static live-view table), and the post-processing behind it.  The rig of
tests/test_serving_nms_gpu.py: mini5, 2 layers, valid_fraction 0.5, bf16, threshold 0.02."""
import pytest
import torch

from mvgformer_amd.synthetic import build_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THRESHOLD = 0.02
SUBSETS = [(0, 2, 4), (1, 2, 3), (3, 4), (2,)]
LENGTHS = [180.0 + 15.0 * k for k in range(14)]


def _rig():
    from mvgformer_amd.factory import build_decoder_for_case, case_to_device
    case = case_to_device(build_case("mini5", seed=4, layers=2, valid_fraction=0.5), DEV)
    return build_decoder_for_case(case, DEV, dtype=torch.bfloat16), case


def _subset(c, views):
    idx = torch.tensor(list(views), device=DEV)            # B = 1: image v is view v
    return [s.index_select(0, idx).contiguous() for s in c.src_views], [c.meta[v] for v in views]


def _mask(views):
    return [v in views for v in range(5)]


def _eager_subset(dec, c, views):
    src, meta = _subset(c, views)
    with torch.no_grad():
        hs, refs, r2d, p2d, cls = dec(c.tgt, c.reference_points, src, meta, c.spatial_shapes, c.level_start_index, None,
                                      query_pos=c.query_pos, threshold=THRESHOLD)
    torch.cuda.synchronize()
    return [hs.clone(), refs.clone(), r2d.clone(), p2d.clone(), torch.stack(list(cls)).clone()]


def _loaded(run, c, **kw):
    return run.load(src_views=c.src_views, tgt=c.tgt, query_pos=c.query_pos, reference_points=c.reference_points, **kw)


def test_one_capture_serves_every_subset():
    from mvgformer_amd.serving import GraphedDecoder
    dec, c = _rig()
    want = {views: _eager_subset(dec, c, views) for views in SUBSETS + [tuple(range(5))]}
    run = GraphedDecoder(dec, c.meta, c.spatial_shapes, c.level_start_index, batch=1, num_queries=c.NQ, threshold=THRESHOLD,
                         live_views=True)
    _loaded(run, c).capture()
    graph, captured = run.graph, run._captured
    assert all(any(t.data_ptr() == p.data_ptr() for p in run._pinned) for t in run.ctx.live)
    for views in [tuple(range(5))] + SUBSETS + [tuple(range(5))]:           # ... and back to all live
        hs, refs, r2d, p2d, cls = run.load(view_live=_mask(views)).replay()
        torch.cuda.synchronize()
        w, live, dead = want[views], list(views), [v for v in range(5) if v not in views]
        assert torch.equal(hs, w[0]) and torch.equal(refs, w[1]) and torch.equal(torch.stack(list(cls)), w[4]), views
        assert torch.equal(r2d[:, :, live], w[2]) and torch.equal(p2d[:, :, live], w[3]), views
        assert not bool(r2d[:, :, dead].any()) and not bool(p2d[:, :, dead].any())
        assert run.graph is graph and run._captured == captured
    # the table is validated on the host, before anything is copied
    with pytest.raises(ValueError):
        run.load(view_live=[False] * 5)
    with pytest.raises(TypeError):
        run.load(view_live=torch.ones(5, dtype=torch.bool, device=DEV))


def test_a_runner_without_live_views_launches_what_it_always_did(monkeypatch):
    """the entry points of one eager forward, in order: without live_views=True none of them is a *_live one, and the sequence is
    the live runner's with the suffix taken off (the live runner changes three launches per layer and adds none); load(view_live=)
    is refused; the replay equals the eager forward.  Both sequences are recorded from THIS code -- no list of the launches as
    they were before the table existed is pinned here -- so a launch added to, or reordered in, both paths alike would not show
    in this test: the comparison of the replay with the eager forward, and the suite's existing launch counts
    (tests/test_postprocess_gpu.py, tests/test_serving.py), are what stands against that."""
    from mvgformer_amd import ops
    from mvgformer_amd.serving import GraphedDecoder
    dec, c = _rig()
    seen = []
    real = ops._launch
    monkeypatch.setattr(ops, "_launch", lambda symbol, *a, **k: (seen.append(symbol), real(symbol, *a, **k))[1])
    names = {}
    for live in (False, True):
        run = GraphedDecoder(dec, c.meta, c.spatial_shapes, c.level_start_index, batch=1, num_queries=c.NQ, threshold=THRESHOLD,
                             live_views=live)
        _loaded(run, c)
        run.eager()                     # builds the caches
        del seen[:]
        out = run.eager()
        names[live] = list(seen)
        if not live:
            plain, eager = run, [t.clone() for t in out[:4]]
    assert not [n for n in names[False] if n.endswith("_live")]
    assert [n[:-5] if n.endswith("_live") else n for n in names[True]] == names[False]
    assert sorted(set(n for n in names[True] if n.endswith("_live"))) == [
        "mvg_chain_update_ffn_class_live", "mvg_project_live", "mvg_triangulate_live", "mvg_triangulate_project_live"]
    with pytest.raises(RuntimeError, match="live_views=True"):
        plain.load(view_live=_mask((0, 1)))
    assert plain.ctx.live is None
    got = plain.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got[:4], eager))


def test_postprocessing_follows_the_table():
    """detections, track ids and refined poses of a masked replay equal those of a runner built on the subset rig whose refiner is
    handed the same fp32 weights 1 / n.  The refiner of the masked runner gets weight 0 for the dead views: structural_kernel adds
    the views' terms in one sequential loop over v, and a zero-weight term is an exact zero there (the dead views' 2D points are
    zeros and their camera records finite, so the term is 0 * finite), which leaves every partial sum as the subset run has it."""
    from mvgformer_amd.serving import GraphedDecoder
    dec, c = _rig()
    views = (0, 2, 4)
    stages = dict(postprocess=dict(dist_thr=0.3, num_nearby_joints_thr=7), tracking=dict(max_tracks=8),
                  refine=dict(bone_lengths=LENGTHS, n_steps=2))
    run = GraphedDecoder(dec, c.meta, c.spatial_shapes, c.level_start_index, batch=1, num_queries=c.NQ, threshold=THRESHOLD,
                         live_views=True, **stages)
    src, meta = _subset(c, views)
    sub = GraphedDecoder(dec, meta, c.spatial_shapes, c.level_start_index, batch=1, num_queries=c.NQ, threshold=THRESHOLD, **stages)
    # the subset runner's refiner with the weights the masked one builds from its table: 1 / 3 as an fp32 division, for every view
    third = (torch.ones((), dtype=torch.float32, device=DEV) / torch.full((), 3.0, dtype=torch.float32, device=DEV))
    conf = third.expand(1, 3, c.NQ * 15).contiguous()
    refiner, update = sub.post.refiner, sub.post.refiner.update
    refiner.update = lambda *a, **k: update(*a, **dict(k, conf=conf))
    _loaded(run, c, view_live=_mask(views)).capture()
    sub.load(src_views=src, tgt=c.tgt, query_pos=c.query_pos, reference_points=c.reference_points).capture()
    w = run.post.view_weights(run.outputs[2][-1])
    assert torch.equal(w[0, [0, 2, 4]], conf[0]) and not bool(w[0, [1, 3]].any())
    for _ in range(2):                  # two frames: the tracker's second update matches against the first one's tracks
        run.replay()
        sub.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(run.detections, sub.detections))
        assert int(run.detections[1][0, 0]) >= 1                                     # the comparison is not vacuous
        assert all(torch.equal(a, b) for a, b in zip(run.track_ids, sub.track_ids))
        assert torch.equal(run.refined[1], sub.refined[1]) and bool((run.refined[1] == 0).any())
        assert torch.equal(run.refined[0].view(torch.int32), sub.refined[0].view(torch.int32))
        assert torch.equal(run.pred, sub.pred)


def test_validate_view_subsets(monkeypatch):
    """python -m mvgformer_amd.validate --view-subsets: a row per threshold and subset from ONE capture per threshold; the row of
    all cameras is the row of a run without the option"""
    from mvgformer_amd import serving, validate
    captures = []
    real = serving.GraphedDecoder.capture
    monkeypatch.setattr(serving.GraphedDecoder, "capture", lambda self, *a, **k: (captures.append(self), real(self, *a, **k))[1])
    argv = ["--cfg", "extract:configs/panoptic/knn5-lr4-q1024-g8.yaml", "--frames", "2", "--device-nms", "1", "--device-track", "1"]
    rep = validate.main(argv + ["--view-subsets", "0,1,2;4,2,0;0,1,2,3,4"])
    rows = rep["results"]
    thrs = sorted({r["inference_conf_thr"] for r in rows})
    assert rep["view_subsets"] == [[0, 1, 2], [0, 2, 4], [0, 1, 2, 3, 4]] and len(rows) == 3 * len(thrs)
    assert [r["view_subset"] for r in rows] == rep["view_subsets"] * len(thrs) and all(r["hip_graph"] for r in rows)
    assert len(captures) == len(thrs) and len({id(r) for r in captures}) == len(thrs)
    plain = validate.main(argv)["results"]
    keys = ("frames", "candidates_above_thr", "poses_after_nms", "tracks")
    for want, got in zip(plain, [r for r in rows if r["view_subset"] == [0, 1, 2, 3, 4]]):
        assert "view_subset" not in want and {k: want[k] for k in keys} == {k: got[k] for k in keys}
    eager = validate.main(argv + ["--view-subsets", "0,2,4", "--graph", "0"])["results"]
    for want, got in zip([r for r in rows if r["view_subset"] == [0, 2, 4]], eager):
        assert not got["hip_graph"] and {k: want[k] for k in keys} == {k: got[k] for k in keys}
    with pytest.raises(SystemExit):
        validate.main(argv + ["--view-subsets", "0,7"])
