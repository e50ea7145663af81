"""The caller-owned static buffers of the serving wrappers (ops.pose_nms_buffers, eval_buffers, track_buffers, track_motion_buffers,
track_eval_buffers, structural_buffers) on CPU tensors: each family is described once in ops.py and both allocated and checked from
that description.  Here the layouts are written out a second time, literally, at the smallest shapes, and every key is bent in turn:
wrong dtype, every dimension off by one, a non-contiguous view.  No kernel is launched."""
import pytest
import torch

from mvgformer_amd import _lib, ops

B, T, J, R, P, K, N, CAPACITY, ACTORS = 2, 3, 2, 4, 2, 5, 4, 3, 2
i32, i64, f32, f64, u8 = torch.int32, torch.int64, torch.float32, torch.float64, torch.uint8


def _families():
    nbytes = int(_lib.load().mvg_pose_nms_workspace(B, N, J))
    assert nbytes > 0
    # name -> (the *_buffers call, the description, its dimensions, key -> (dtype, shape, fill or None = not initialised))
    return {
        "pose_nms": (lambda: ops.pose_nms_buffers(B, N, J, device="cpu"), ops._NMS, dict(B=B, N=N, J=J, rows=N, nbytes=nbytes),
                     dict(keep=(i32, (2, 4), None), count=(i32, (2, 2), None), dets=(f32, (2, 4, 2, 5), None),
                          workspace=(u8, (nbytes,), None))),
        "eval": (lambda: ops.eval_buffers(CAPACITY, ACTORS, "cpu"), ops._EVAL, dict(capacity=CAPACITY, actors=ACTORS),
                 dict(mpjpe=(f64, (3,), 0), score=(f64, (3,), 0), gt_id=(i64, (3,), 0), correct=(i64, (2,), 0), total=(i64, (2,), 0),
                      bone_correct=(i64, (2, 10), 0), state=(i64, (8,), 0))),
        "track": (lambda: ops.track_buffers(B, T, J, R, "cpu"), ops._TRACK, dict(B=B, T=T, J=J, R=R),
                  dict(id=(i32, (2, 3), -1), hits=(i32, (2, 3), 0), misses=(i32, (2, 3), 0), born=(i64, (2, 3), 0),
                       score=(f32, (2, 3), 0), pose=(f32, (2, 3, 2, 3), 0), next_id=(i32, (2,), 0), state=(i64, (8,), 0),
                       ids=(i32, (2, 4), -1), slots=(i32, (2, 4), -1))),
        "track_motion": (lambda: ops.track_motion_buffers(B, T, J, R, "cpu"), ops._TRACK_MOTION, dict(B=B, T=T, J=J, R=R),
                         dict(mean=(f64, (2, 3, 2, 2, 3), 0), var=(f64, (2, 3, 3), 0), row_pose=(f32, (2, 4, 2, 3), 0))),
        "track_eval": (lambda: ops.track_eval_buffers(B, P, K, "cpu"), ops._TRACK_EVAL, dict(B=B, P=P, K=K),
                       dict(last_track=(i32, (2, 2), -1), counters=(i64, (2, 13), 0), dist_sum=(f64, (2,), 0), seen=(i64, (2, 2), 0),
                            covered=(i64, (2, 2), 0), overlap=(i32, (2, 2, 5), 0))),
        "structural": (lambda: ops.structural_buffers(B, P, J, "cpu"), ops._STRUCTURAL, dict(B=B, P=P, J=J),
                       dict(poses=(f32, (2, 2, 2, 3), 0), status=(i32, (2, 2), -1))),
    }


FAMILY_NAMES = ("pose_nms", "eval", "track", "track_motion", "track_eval", "structural")


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_buffers_have_the_documented_layout(family):
    make, layout, dims, expected = _families()[family]
    buffers = make()
    assert list(buffers) == list(expected) == list(layout.keys)
    for key, (dtype, shape, fill) in expected.items():
        t = buffers[key]
        assert t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous() and t.device.type == "cpu", key
        if fill is not None:
            assert bool((t == fill).all()), key
    assert layout.check(buffers, dims) is None
    assert layout.check(buffers, dims, keys=list(expected)[:1]) is None


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_check_rejects_every_key_bent_in_every_way(family):
    make, layout, dims, expected = _families()[family]
    good = make()
    for key, (dtype, shape, _) in expected.items():
        bent = [torch.zeros(shape, dtype=f64 if dtype != f64 else f32)]
        for d in range(len(shape)):
            for step in (-1, 1):
                bent.append(torch.zeros(shape[:d] + (shape[d] + step,) + shape[d + 1:], dtype=dtype))
        bent.append(torch.zeros((), dtype=dtype))
        strided = torch.zeros(shape[:-1] + (2 * shape[-1],), dtype=dtype)[..., ::2]
        assert tuple(strided.shape) == shape and not strided.is_contiguous()
        bent.append(strided)
        for t in bent:
            with pytest.raises(RuntimeError, match="contiguous .*%s" % layout.maker) as e:
                layout.check(dict(good, **{key: t}), dims, who="the_caller")
            assert str(e.value).startswith("the_caller: buffer %r " % key)
            assert layout.check(dict(good, **{key: t}), dims, keys=[k for k in expected if k != key]) is None    # not looked at


def test_pose_nms_dets_rows_and_the_limit_messages():
    assert tuple(ops.pose_nms_buffers(B, N, J, dets_rows=3, device="cpu")["dets"].shape) == (2, 3, 2, 5)
    with pytest.raises(_lib.MvgError, match=r"mvg_pose_nms: unsupported shape B = 2, N = 2049 \(<= 2048\), J = 2 \(<= 32\), dets_rows = 2049"):
        ops.pose_nms_buffers(B, 2049, J, device="cpu")
    for call, text in (
            (lambda: ops.track_buffers(0, T, J, R, "cpu"),
             "track_buffers: unsupported shape B = 0 (<= 4096), T = 3 (<= 64), J = 2 (<= 32), R = 4 (<= 16384)"),
            (lambda: ops.track_motion_buffers(B, 65, J, R, "cpu"),
             "track_motion_buffers: unsupported shape B = 2 (<= 4096), T = 65 (<= 64), J = 2 (<= 32), R = 4 (<= 16384)"),
            (lambda: ops.track_eval_buffers(B, P, 4097, "cpu"),
             "track_eval_buffers: unsupported shape B = 2 (<= 4096), P = 2 (<= 64), K = 4097 (<= 4096)"),
            (lambda: ops.structural_buffers(B, P, 18, "cpu"), "structural_buffers: unsupported shape B = 2, P = 2, J = 18 (2 .. 17)")):
        with pytest.raises(_lib.MvgError) as e:
            call()
        assert str(e.value) == text


def test_the_shared_input_checks():
    dets, count = torch.zeros((B, R, J, 5)), torch.zeros((B, 2), dtype=i32)
    assert ops._check_dets("f", dets, count) == ops._check_dets("f", dets, None) == (B, R, J)
    for bad_dets in (dets.double(), dets[..., :4], dets[0]):
        with pytest.raises(RuntimeError, match=r"^f: dets \(B, R, J, 5\) float32 expected$"):
            ops._check_dets("f", bad_dets, count)
    for bad_count in (count.long(), count[:1], count[:, :1]):
        with pytest.raises(RuntimeError, match=r"^f: count \(B, 2\) int32 or None expected$"):
            ops._check_dets("f", dets, bad_count)
    j3d, vis, num = torch.zeros((B, 3, J, 3)), torch.zeros((B, 3, J)), torch.zeros((B,), dtype=i32)
    assert ops._check_ground_truth("f", j3d, vis, num, B, J) == 3
    for bad, what in (((j3d.double(), vis, num), "joints_3d "), ((j3d[:1], vis, num), "joints_3d "), ((j3d[..., :2], vis, num), "joints_3d "),
                      ((j3d, vis.double(), num), "joints_3d_vis"), ((j3d, vis[:, :2], num), "joints_3d_vis"),
                      ((j3d, vis, num.long()), "num_person"), ((j3d, vis, num[:1]), "num_person")):
        with pytest.raises(RuntimeError, match="^f: %s" % what):
            ops._check_ground_truth("f", *bad, B, J)
