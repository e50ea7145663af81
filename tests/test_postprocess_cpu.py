"""postprocess.PostProcess, what can be checked without a GPU: the option rules, the shared ground-truth inputs and their loading
rules, snapshot / restore and the tensor list, on device="cpu" (the built library is asked for the NMS workspace size only).
Batch 1, 64 queries, 15 joints.  The chain on the device is in tests/test_postprocess_gpu.py."""
import itertools

import pytest
import torch

from mvgformer_amd import _lib
from mvgformer_amd.postprocess import OPTIONS, PostProcess

LENGTHS = [180.0 + 15.0 * k for k in range(14)]
FULL = dict(postprocess={}, evaluation=dict(kind="panoptic", capacity=64), tracking=dict(max_tracks=8, motion=True),
            track_evaluation=dict(max_ids=64), refine=dict(bone_lengths=LENGTHS))


def _post(**options):
    return PostProcess(1, 64, 15, 0.1, "cpu", **options)


def _ptrs(tensors):
    return {t.data_ptr() for t in tensors}


def test_every_combination_of_the_options_constructs_or_is_refused():
    assert list(OPTIONS) == ["postprocess", "evaluation", "tracking", "track_evaluation", "refine"] == list(FULL)
    built = 0
    for on in itertools.product([False, True], repeat=len(FULL)):
        options = {name: FULL[name] for name, o in zip(FULL, on) if o}
        # the first option in the table's order that misses what it needs names it; nothing at all misses postprocess
        missing = [needs for name, (_, needs, _) in OPTIONS.items() if name in options and needs is not None and needs not in options]
        if "postprocess" not in options:
            missing.append("postprocess")
        if missing:
            with pytest.raises(ValueError, match="requires %s" % missing[0]):
                _post(**options)
            continue
        post = _post(**options)
        built += 1
        for name, attr in (("evaluation", "evaluator"), ("tracking", "tracker"), ("track_evaluation", "track_evaluator"),
                           ("refine", "refiner")):
            assert (getattr(post, attr) is not None) == (name in options), (options, attr)
        assert len(post.stages) == len(options) - 1
        assert (post.ground_truth is not None) == ("evaluation" in options or "track_evaluation" in options)
        assert (post.person_id is not None) == ("track_evaluation" in options)
    assert built == 12                  # postprocess x {evaluation} x {refine} x {no tracking, tracking, tracking + its scoring}


def test_defaults_and_the_joint_map():
    post = _post(postprocess=dict(max_dets=5))
    assert post.postprocess == dict(dist_thr=0.3, num_nearby_joints_thr=7, max_dets=5, dets_rows=None)
    assert [tuple(t.shape) for t in post.detections] == [(1, 64, 15, 5), (1, 2), (1, 64)]
    assert post.stages == [] and post.snapshot() == [] and _ptrs(post.tensors()) == _ptrs(post.nms.values())
    shelf = _post(postprocess=dict(dets_rows=16), convert_joint_format_indices=list(range(14)), tracking={})
    assert torch.is_tensor(shelf.convert_joint_format_indices) and shelf.convert_joint_format_indices.dtype == torch.long
    assert tuple(shelf.detections[0].shape) == (1, 16, 14, 5) and tuple(shelf.track_ids[0].shape) == (1, 16)
    assert shelf.tracker.num_joints == 14 and shelf.track_poses is None


@pytest.mark.parametrize("options,error,fragment", [
    (dict(postprocess=dict(threshold=0.3)), TypeError, "unknown postprocess keys"),
    (dict(postprocess={}, evaluation=dict(metric="ap")), TypeError, "unknown evaluation keys"),
    (dict(postprocess={}, tracking=dict(max_tracks=8, motion_model="kalman")), TypeError, "unknown tracking keys"),
    (dict(postprocess={}, tracking=dict(motion=True, dt=1.0)), TypeError, "unknown tracking keys"),
    (dict(postprocess={}, tracking=dict(motion=dict(model="kalman"))), TypeError, "unknown motion keys"),
    (dict(postprocess={}, tracking={}, track_evaluation=dict(metric="hota")), TypeError, "unknown track_evaluation keys"),
    (dict(postprocess={}, refine=dict(bone_lengths=LENGTHS, steps=3)), TypeError, "unknown refine keys"),
    (dict(tracking=dict(motion=True)), ValueError, "requires postprocess"),
    (dict(evaluation=dict(kind="panoptic")), ValueError, "requires postprocess"),
    (dict(refine=dict(bone_lengths=LENGTHS)), ValueError, "requires postprocess"),
    (dict(postprocess={}, track_evaluation={}), ValueError, "requires tracking"),
    (dict(postprocess={}, tracking={}, evaluation=dict(kind="panoptic", capacity=64), track_evaluation=dict(max_persons=4)),
     ValueError, "below the 10 person slots"),
    (dict(postprocess={}, refine=dict(bone_lengths=LENGTHS), convert_joint_format_indices=list(range(14))), ValueError,
     "convert_joint_format_indices"),
    (dict(postprocess=dict(dets_rows=65), refine=dict(bone_lengths=LENGTHS)), ValueError, "dets_rows = 65 > num_queries = 64"),
    (dict(postprocess={}, refine=dict(bone_lengths=LENGTHS[:3])), ValueError, "bone lengths"),
    (dict(postprocess={}, refine=dict(bone_lengths=LENGTHS, n_steps=9)), RuntimeError, "n_steps"),
])
def test_refusals_keep_their_type_and_wording(options, error, fragment):
    with pytest.raises(error, match=fragment):
        _post(**options)


def test_two_scorers_share_one_set_of_ground_truth_tensors():
    both = _post(postprocess={}, tracking={}, evaluation=dict(kind="panoptic", capacity=64), track_evaluation={})
    assert both.track_evaluator.max_persons == both.evaluator.max_persons == 10
    assert len(both.ground_truth) == 3 and tuple(both.ground_truth[0].shape) == (1, 10, 15, 3)
    assert tuple(both.person_id.shape) == (1, 10) and both.person_id.dtype == torch.int32
    assert both.person_id.tolist() == [list(range(10))]
    wide = _post(postprocess={}, tracking={}, evaluation=dict(kind="panoptic", capacity=64, max_persons=4),
                 track_evaluation=dict(max_persons=6))
    assert tuple(wide.ground_truth[0].shape) == (1, 4, 15, 3) and tuple(wide.person_id.shape) == (1, 4)      # the evaluator's slots
    alone = _post(postprocess={}, tracking={}, track_evaluation=dict(max_persons=4))
    assert tuple(alone.ground_truth[1].shape) == (1, 4, 15) and alone.person_id.tolist() == [[0, 1, 2, 3]]


def test_load_ground_truth_rules():
    post = _post(postprocess={}, tracking={}, track_evaluation={})
    j3d, vis, num = torch.ones((1, 2, 15, 3)), torch.ones((1, 2, 15)), torch.tensor([2], dtype=torch.int32)
    post.ground_truth[0].fill_(5.0)
    post.load_ground_truth((j3d, vis, num, torch.tensor([[3, 1]], dtype=torch.int32)))
    assert post.person_id[0, :3].tolist() == [3, 1, 2]
    assert bool((post.ground_truth[0][:, :2] == 1.0).all()) and bool((post.ground_truth[0][:, 2:] == 5.0).all())     # behind G: as it was
    assert bool((post.ground_truth[1][:, :2] == 1.0).all()) and post.ground_truth[2].tolist() == [2]
    post.load_ground_truth((j3d, vis, num))
    assert post.person_id[0].tolist() == list(range(10))
    post.load_ground_truth((j3d, vis, num, None))
    assert post.person_id[0].tolist() == list(range(10))
    with pytest.raises(ValueError, match="person slots, built for max_persons = 10"):
        post.load_ground_truth((torch.ones((1, 11, 15, 3)), torch.ones((1, 11, 15)), num))
    with pytest.raises(ValueError, match="ground_truth needs"):
        _post(postprocess={}, tracking={}).load_ground_truth((j3d, vis, num))
    with pytest.raises(ValueError, match="person_id needs"):
        _post(postprocess={}, evaluation=dict(kind="panoptic", capacity=64)).load_ground_truth((j3d, vis, num, post.person_id))


def test_snapshot_and_restore_cover_every_accumulating_buffer():
    post = _post(**FULL)
    named = {"evaluator": post.evaluator.buffers, "tracker": post.tracker.buffers, "motion": post.tracker.motion_buffers,
             "track_evaluator": post.track_evaluator.buffers}
    assert all(len(b) > 0 for b in named.values())
    for i, t in enumerate(t for b in named.values() for t in b.values()):
        t.copy_((torch.arange(t.numel()) % 7 + i).reshape(t.shape))
    want = {(n, k): t.clone() for n, b in named.items() for k, t in b.items()}
    saved = post.snapshot()
    assert len(saved) == 3                                      # the refiner keeps nothing from frame to frame
    for b in named.values():
        for t in b.values():
            t.fill_(77)
    assert post.restore(saved) is post
    for (n, k), t in want.items():
        assert named[n][k].dtype == t.dtype and torch.equal(named[n][k], t), (n, k)


def test_tensors_lists_every_static_tensor_once_the_cameras_are_set():
    post = _post(**FULL)
    assert post.Pm is None
    cams = torch.zeros((5, _lib.CAM_STRIDE))
    post.set_cameras(cams, 5)
    pm = post.Pm
    assert tuple(pm.shape) == (1, 5, 3, 4) and post.set_cameras(cams + 1.0, 5).Pm is pm and float(pm.abs().sum()) > 0.0
    want = (list(post.nms.values()) + list(post.evaluator.buffers.values()) + list(post.tracker.buffers.values())
            + list(post.tracker.motion_buffers.values()) + list(post.track_evaluator.buffers.values())
            + list(post.refiner.buffers.values()) + list(post.ground_truth) + [post.person_id, post.bone_lengths, post.Pm])
    assert _ptrs(post.tensors()) == _ptrs(want) and len(_ptrs(want)) == len(want)
    assert post.bone_lengths is post.refiner.bone_lengths and post.refined == (post.refiner.poses, post.refiner.status)
    assert post.track_poses is post.tracker.motion_buffers["row_pose"]


def test_run_is_refused_on_the_cpu():
    post = _post(postprocess={})
    g = torch.Generator().manual_seed(0)
    L, B, V, Lq = 2, 1, 5, 64 * 15
    outputs = (torch.rand((L, B, Lq, 8), generator=g), torch.rand((L, B, Lq, 3), generator=g), torch.rand((L, B, V, Lq, 2), generator=g),
               torch.rand((L, B, V, Lq, 2), generator=g), [torch.rand((B, 64, 2), generator=g) * 0.9 + 0.05 for _ in range(L)])
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        post.run(outputs)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        post.run_packed(torch.zeros((1, 64, 15, 5)), outputs[2][-1])
