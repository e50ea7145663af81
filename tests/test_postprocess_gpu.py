"""postprocess.PostProcess with every stage at once, inside serving.GraphedDecoder: NMS, evaluator, tracker with its motion model,
track evaluator and refiner in one captured graph.  The rig of the other serving tests: mini5, 2 layers, valid_fraction 0.5, bf16,
threshold 0.02, the maps of seeds 4 and 3 alternating over five frames; the ground truth is the first frame's own kept poses and
frame 3 carries no annotation (tests/test_serving_track_eval_gpu.py); the bone lengths are tests/test_serving_refine_gpu.py's."""
import pytest
import torch

from mvgformer_amd import ops
from mvgformer_amd.synthetic import build_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THRESHOLD = 0.02
STAGES = dict(
    evaluation=dict(kind="panoptic", capacity=64 * 5, max_persons=4),
    tracking=dict(max_tracks=8, max_dist=500.0, max_misses=1, min_hits=1, motion=True),
    track_evaluation=dict(max_ids=64),
    refine=dict(bone_lengths=[180.0 + 15.0 * k for k in range(14)]))
# launches of one eager() with all five options, by ops.PROFILE name, recorded from the hand-wired chain this pipeline replaced
# (the refiner's un-distortion launch carries no name)
LAUNCHES = dict(pose_nms=1, eval_match=1, track_predict=1, track_update=1, track_correct=1, track_eval=1, structural_triangulate=1)


def _bits(tensors):
    return [t.detach().clone().reshape(-1).view(torch.uint8) for t in tensors]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _state(run):
    """every accumulator of the runner's pipeline, as bits"""
    return _bits(t for s in (run.evaluator, run.tracker, run.track_evaluator) if s is not None for t in s.tensors())


def _launches(run):
    ops.PROFILE = {}
    try:
        run.eager()
        torch.cuda.synchronize()
        return {k: len(v) for k, v in ops.PROFILE.items()}
    finally:
        ops.PROFILE = None


def test_all_five_stages_in_one_graph():
    from mvgformer_amd.factory import build_decoder_for_case, case_to_device
    from mvgformer_amd.serving import GraphedDecoder
    from tests.test_serving_nms_gpu import _clone, _eq
    cases = [case_to_device(build_case("mini5", seed=s, layers=2, valid_fraction=0.5), DEV) for s in (4, 3)]
    dec = build_decoder_for_case(cases[0], DEV, dtype=torch.bfloat16)
    c = cases[0]

    def runner(*names):
        options = {n: STAGES[n] for n in names}
        if "track_evaluation" in options and "evaluation" not in options:      # the person slots `full` takes from its evaluator
            options["track_evaluation"] = dict(STAGES["track_evaluation"], max_persons=STAGES["evaluation"]["max_persons"])
        return GraphedDecoder(dec, c.meta, c.spatial_shapes, c.level_start_index, batch=1, num_queries=c.NQ, threshold=THRESHOLD,
                              postprocess=dict(dist_thr=0.3, num_nearby_joints_thr=7), **options)

    def feed(run, c, truth):
        run.set_cameras(c.meta)
        run.load(src_views=c.src_views, tgt=c.tgt, query_pos=c.query_pos, reference_points=c.reference_points,
                 ground_truth=truth if run.ground_truth is not None else None)

    base, full = runner(), runner(*STAGES)
    alone = dict(evaluation=runner("evaluation"), tracking=runner("tracking"), track_evaluation=runner("tracking", "track_evaluation"),
                 refine=runner("refine"))
    assert base.post.stages == [] and len(full.post.stages) == 4
    # the ground truth: the kept poses of the first frame
    feed(base, c, None)
    base.capture().replay()
    torch.cuda.synchronize()
    G = min(int(base.detections[1][0, 0]), 3)
    assert G >= 2
    j3d, vis = base.detections[0][:, :G, :, :3].clone(), torch.ones((1, G, 15), device=DEV)

    def truth(i):
        return j3d, vis, torch.tensor([-1 if i == 3 else G], dtype=torch.int32, device=DEV)

    # 4. a capture leaves accumulators that hold something as they were: one eager frame first, then the warm-up forwards
    feed(full, c, truth(0))
    full.eager()
    torch.cuda.synchronize()
    before = _state(full)
    assert full.evaluator.state()["kept_rows"] > 0 and full.tracker.state()["births"] > 0 and full.track_evaluator.state()["frames"] == 1
    full.capture()
    torch.cuda.synchronize()
    assert _same(_state(full), before)
    for stage in (full.evaluator, full.tracker, full.track_evaluator):
        stage.reset()

    def outputs(run):
        """what the frame left in the static tensors of the stages the runner has, as bits"""
        named = dict(detections=run.detections, track_ids=run.track_ids, refined=run.refined,
                     track_poses=None if run.track_poses is None else (run.track_poses,))
        return {k: _bits(v) for k, v in named.items() if v is not None}

    frames = (cases * 3)[:5]
    replayed, kept_rows, tracked, solved = [], [], 0, 0
    for i, c in enumerate(frames):
        for run in (base, full, *alone.values()):
            feed(run, c, truth(i))
        want_out = _clone(base.replay())
        got_out = full.replay()
        for run in alone.values():
            run.replay()
        torch.cuda.synchronize()
        # 1. the decoder outputs and the detections are those of the runner without any stage
        assert _eq(got_out, want_out), i
        got = outputs(full)
        assert _same(got["detections"], outputs(base)["detections"]), i
        # 2. every stage writes what it writes when it is the only one
        assert _same(got["track_ids"], outputs(alone["tracking"])["track_ids"]), i
        assert _same(got["track_poses"], outputs(alone["tracking"])["track_poses"]), i
        assert _same(got["track_ids"], outputs(alone["track_evaluation"])["track_ids"]), i
        assert _same(got["refined"], outputs(alone["refine"])["refined"]), i
        replayed.append(got)
        k = int(full.detections[1][0, 0])
        kept_rows.append(k)
        tracked += int((full.track_ids[0][0, :k] >= 0).sum())
        solved += int((full.refined[1][0, :k] == 0).sum())
    print("kept", kept_rows, "rows with a track id", tracked, "rows solved", solved)
    assert min(kept_rows) >= 2 and tracked >= 1 and solved >= 1                   # the comparisons are not vacuous
    assert full.evaluator.state()["kept_rows"] > 0
    assert _same(_bits(full.evaluator.buffers.values()), _bits(alone["evaluation"].evaluator.buffers.values()))
    assert _same(_bits(full.tracker.tensors()), _bits(alone["tracking"].tracker.tensors()))
    assert _same(_bits(full.tracker.buffers.values()), _bits(alone["track_evaluation"].tracker.buffers.values()))
    report = full.track_evaluator.report()
    assert report == alone["track_evaluation"].track_evaluator.report() and report["total"]["frames"] == 4
    # 5. the graph's operands are pinned
    pinned = {p.data_ptr() for p in full._pinned}
    assert len(full.post.tensors()) == 38 and all(t.data_ptr() in pinned for t in full.post.tensors())
    # 3. the same frames through eager() after a reset: the same bits, frame by frame and in the accumulators
    final = _state(full)
    for stage in (full.evaluator, full.tracker, full.track_evaluator):
        stage.reset()
    for i, c in enumerate(frames):
        feed(full, c, truth(i))
        full.eager()
        torch.cuda.synchronize()
        got = outputs(full)
        assert all(_same(got[k], replayed[i][k]) for k in replayed[i]) and set(got) == set(replayed[i]), i
    assert _same(_state(full), final) and full.track_evaluator.report() == report
    # 6. one eager() launches what the hand-wired chain launched, and nothing else that the plain runner does not launch
    got, plain = _launches(full), _launches(base)
    print(got)
    assert {k: got.get(k, 0) for k in LAUNCHES} == LAUNCHES
    assert {k: n for k, n in got.items() if k not in LAUNCHES} == {k: n for k, n in plain.items() if k not in LAUNCHES}
    assert {k: plain.get(k, 0) for k in LAUNCHES} == dict(dict.fromkeys(LAUNCHES, 0), pose_nms=1)
