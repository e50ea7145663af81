"""The restatement of mvg_track_bones (tests/bones_ref.py) against its stated rules, the statement the stage is built on (lengths
estimated per track make one ST step better than LS, on synthetic scenes) and the host-side refusals.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

from mvgformer_amd import _lib, ops
from tests import bones_cases, bones_ref, track_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT = bones_cases.PANOPTIC15_PARENT
J = len(PARENT)


def _det(rng, bones=None, root=(0.0, 0.0, 900.0)):
    """one detection row (J, 5) of a person with the given bones (random ones by default)"""
    bones = rng.uniform(150.0, 450.0, J - 1) if bones is None else bones
    row = np.zeros((J, 5), np.float32)
    row[:, :3] = bones_cases.posed(rng, PARENT, bones, np.asarray(root))
    row[:, 3], row[:, 4] = 1.0, 0.9
    return row


def _frame(rows, R):
    dets = np.zeros((1, R, J, 5), np.float32)
    dets[..., 3] = -1.0
    for i, row in enumerate(rows):
        dets[0, i] = row
    return dets, np.array([[len(rows), 0]], np.int32)


def test_median_is_numpys_median_of_the_widened_samples():
    rng = np.random.default_rng(0)
    W = bones_ref.BONES_MAX_W
    for n in range(1, 2 * W + 2):
        for ties in (False, True):
            v = rng.uniform(100.0, 500.0, n).astype(np.float32)
            if ties:
                v = np.round(v / 50.0).astype(np.float32) * np.float32(50.0)
            want = np.float32(np.median(v.astype(np.float64)))
            got = bones_ref.median(v)
            assert got.dtype == np.float32 and got.view(np.uint32) == want.view(np.uint32), (n, ties)
            cols = np.stack([v, v[::-1], np.roll(v, 3)], 1)
            assert np.array_equal(bones_ref.median_columns(cols).view(np.uint32), np.repeat(want, 3).view(np.uint32))


def test_ring_wraps_around():
    rng = np.random.default_rng(1)
    W = 3
    bones = rng.uniform(150.0, 450.0, J - 1)
    buf = bones_ref.new_buffers(1, 2, J, 4, W)
    slots = np.array([[1, -1, -1, -1]], np.int32)
    ident = np.array([[-1, 7]], np.int32)
    samples = []
    for f in range(2 * W + 3):
        dets, count = _frame([_det(rng, bones + rng.normal(scale=4.0, size=J - 1))], 4)
        bones_ref.update(dets, count, slots, ident, PARENT, buf, min_frames=1)
        samples.append(bones_ref.bones_of(dets[0, 0], PARENT))
        assert buf["seen"][0, 1] == f + 1 and buf["owner"][0, 1] == 7
        assert np.array_equal(buf["hist"][0, 1, f % W], samples[-1])
        window = np.stack(samples[-W:])
        want = np.median(window.astype(np.float64), axis=0).astype(np.float32)
        assert np.array_equal(buf["length"][0, 1].view(np.uint32), want.view(np.uint32))
        assert np.array_equal(buf["row_length"][0, 0], buf["length"][0, 1]) and buf["row_source"][0].tolist() == [0, -1, -1, -1]
    # the ring holds the last W samples, each at its frame's index modulo W
    for f in range(2 * W, 2 * W + 3):
        assert np.array_equal(buf["hist"][0, 1, f % W], samples[f])
    assert not buf["hist"][0, 0].any() and buf["seen"][0, 0] == 0


def test_a_slot_that_is_freed_and_reopened_starts_over():
    """the real tracker rule (tests/track_ref.py), max_misses = 0: person A is followed for three frames, then only person B, far
    away, is seen: A's slot is freed and reopened for B by the SAME update"""
    rng = np.random.default_rng(2)
    T, R, W = 2, 4, 4
    track = track_ref.new_buffers(1, T, J, R)
    buf = bones_ref.new_buffers(1, T, J, R, W)
    a, b = rng.uniform(150.0, 450.0, J - 1), rng.uniform(150.0, 450.0, J - 1)
    history = []
    for f in range(5):
        who, root = (a, (0.0, 0.0, 900.0)) if f < 3 else (b, (9000.0, 0.0, 900.0))
        row = _det(np.random.default_rng(5), who, root)            # the same figure every frame: the tracker keeps the match
        dets, count = _frame([row], R)
        track_ref.update(dets, count, track, 500.0, 0, 1)
        bones_ref.update(dets, count, track["slots"], track["id"], PARENT, buf, min_frames=2)
        history.append((int(track["slots"][0, 0]), int(track["id"][0, 0]), int(buf["seen"][0, 0]), int(buf["row_source"][0, 0])))
    # slot 0 throughout; ids 0 then 1; seen counts up, starts over with the new owner; min_frames = 2 decides the source
    assert history == [(0, 0, 1, 2), (0, 0, 2, 0), (0, 0, 3, 0), (0, 1, 1, 2), (0, 1, 2, 0)]
    assert buf["owner"][0].tolist() == [1, -1]
    assert np.array_equal(buf["length"][0, 0], bones_ref.bones_of(row, PARENT))
    # a slot that is only freed: its length is zeroed and nothing is sampled
    track["id"][0, 0] = -1
    dets, count = _frame([], R)
    bones_ref.update(dets, count, np.full((1, R), -1, np.int32), track["id"], PARENT, buf)
    assert buf["owner"][0, 0] == -1 and buf["seen"][0, 0] == 0 and not buf["length"][0, 0].any()


def test_a_row_that_is_not_finite_takes_no_sample():
    rng = np.random.default_rng(3)
    buf = bones_ref.new_buffers(1, 1, J, 2, 4)
    slots, ident = np.array([[0, -1]], np.int32), np.array([[5]], np.int32)
    good = _det(rng)
    bones_ref.update(*_frame([good], 2), slots, ident, PARENT, buf, min_frames=1)
    before = {k: v.copy() for k, v in buf.items()}
    for bad_value in (np.nan, np.inf):
        bad = good.copy()
        bad[7, 1] = bad_value
        length, source = bones_ref.update(*_frame([bad], 2), slots, ident, PARENT, buf, min_frames=1)
        assert all(np.array_equal(buf[k], before[k]) for k in bones_ref.STATE)
        # the row still has its track's lengths
        assert source[0].tolist() == [0, -1] and np.array_equal(length[0, 0], before["length"][0, 0])
    # without a track old enough and without a fallback the row's own lengths are handed on as computed
    length, source = bones_ref.update(*_frame([bad], 2), slots, ident, PARENT, buf, min_frames=2)
    assert source[0, 0] == 2 and not np.isfinite(length[0, 0]).all() and np.isfinite(length[0, 0]).sum() >= J - 4


def test_the_three_sources_and_none():
    rng = np.random.default_rng(4)
    R, T = 6, 2
    rows = [_det(rng) for _ in range(4)]
    dets, count = _frame(rows, R)
    dets[0, 2, :, 3] = -1.0                                          # a row in front of the count that is no detection
    slots = np.array([[0, 1, 0, -1, 1, 1]], np.int32)                # rows 4, 5 lie behind the count
    ident = np.array([[3, 4]], np.int32)
    buf = bones_ref.new_buffers(1, T, J, R, 4)
    buf["owner"][:] = ident
    buf["seen"][0] = [2, 0]                                          # slot 0 has two samples and takes its third here
    buf["hist"][0, 0, :2] = [bones_ref.bones_of(rows[3], PARENT), bones_ref.bones_of(rows[2], PARENT)]
    fallback = np.linspace(200.0, 330.0, J - 1).astype(np.float32)
    length, source = bones_ref.update(dets, count, slots, ident, PARENT, buf, min_frames=3, fallback=fallback)
    assert source[0].tolist() == [0, 1, -1, 1, -1, -1] and buf["seen"][0].tolist() == [3, 1]
    assert np.array_equal(length[0, 0], buf["length"][0, 0]) and np.array_equal(length[0, 1], fallback)
    assert not length[0, 2].any() and not length[0, 4:].any()
    length, source = bones_ref.update(dets, count, slots, ident, PARENT, buf, min_frames=5, fallback=None)
    assert source[0].tolist() == [2, 2, -1, 2, -1, -1]
    assert all(np.array_equal(length[0, i], bones_ref.bones_of(rows[i], PARENT)) for i in (0, 1, 3))
    # count None: every row with a flag counts; count above R is clamped
    for c in (None, np.array([[99, 0]], np.int32)):
        _, source = bones_ref.update(dets, c, slots, ident, PARENT, bones_ref.new_buffers(1, T, J, R, 4), min_frames=1)
        assert source[0].tolist() == [0, 0, -1, 2, -1, -1]
    _, source = bones_ref.update(dets, np.array([[0, 0]], np.int32), slots, ident, PARENT, bones_ref.new_buffers(1, T, J, R, 4))
    assert (source == -1).all()


def test_of_two_rows_that_name_a_slot_the_lowest_is_the_sample():
    rng = np.random.default_rng(5)
    rows = [_det(rng) for _ in range(3)]
    dets, count = _frame(rows, 4)
    buf = bones_ref.new_buffers(1, 2, J, 4, 4)
    slots, ident = np.array([[7, 1, 1, -1]], np.int32), np.array([[-1, 0]], np.int32)      # 7 >= T names no slot
    length, source = bones_ref.update(dets, count, slots, ident, PARENT, buf, min_frames=1)
    assert buf["seen"][0].tolist() == [0, 1] and np.array_equal(buf["hist"][0, 1, 0], bones_ref.bones_of(rows[1], PARENT))
    assert source[0].tolist() == [2, 0, 0, -1] and np.array_equal(length[0, 1], length[0, 2])
    # a lowest row that is not finite is still THE sample: the slot takes none
    dets[0, 1, 3, 0] = np.nan
    bones_ref.update(dets, count, slots, ident, PARENT, buf, min_frames=1)
    assert buf["seen"][0].tolist() == [0, 1]


@pytest.mark.parametrize("V", [3, 5])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_one_st_step_under_track_lengths_is_better_than_ls(V, seed):
    """4 persons with fixed bones and a fresh pose per frame, 2 px noise, uniform view weights, W = 8: the LS poses are the samples,
    as the decoder's triangulated poses would be.  The ORDERING only: against the true lengths and against the generating pose one
    ST step under the per-track medians beats LS.  Synthetic scenes; no statement about a dataset."""
    got = bones_cases.study(seed, V, W=8, persons=4, noise=2.0)
    print(V, seed, {k: round(v, 3) for k, v in got.items()})
    assert got["st_bone_mm"] < got["ls_bone_mm"]
    assert got["st_joint_mm"] < got["ls_joint_mm"]


def test_the_header_declares_the_entry_point_and_its_window_limit():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvg_decoder.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+mvg_track_bones\s*\(", header) and re.search(r"#define\s+MVG_BONES_MAX_W\s+32\b", header)
    assert _lib.DEFINES["MVG_BONES_MAX_W"] == 32 == ops.BONES_MAX_W == bones_ref.BONES_MAX_W
    restype, params = _lib.PROTOTYPES["mvg_track_bones"]
    assert restype is __import__("ctypes").c_int and params[-1][1] == "stream" and "mvg_track_bones" in _lib.STREAM_LAST
    assert "bones.hip" in open(os.path.join(ROOT, "mvgformer_amd", "csrc", "Makefile")).read()
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert hasattr(_lib.load(), "mvg_track_bones")


def test_host_side_refusals():
    from mvgformer_amd import structural
    from mvgformer_amd.postprocess import PostProcess
    B, T, R, W = 1, 4, 8, 8
    track = ops.track_buffers(B, T, J, R, "cpu")
    bones = ops.track_bones_buffers(B, T, J, R, W, "cpu")
    assert set(bones) == {"owner", "seen", "hist", "length", "row_length", "row_source"}
    assert tuple(bones["hist"].shape) == (B, T, W, J - 1) and bool((bones["owner"] == -1).all()) and not bones["seen"].any()
    dets, count = torch.zeros((B, R, J, 5)), torch.zeros((B, 2), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.track_bones(dets, count, track, PARENT, bones)
    with pytest.raises(RuntimeError, match="float32"):
        ops.track_bones(dets.double(), count, track, PARENT, bones)
    with pytest.raises(RuntimeError, match="count"):
        ops.track_bones(dets, count.long(), track, PARENT, bones)
    with pytest.raises(RuntimeError, match="fallback"):
        ops.track_bones(dets, count, track, PARENT, bones, fallback=torch.zeros(J - 1, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="fallback"):
        ops.track_bones(dets, count, track, PARENT, bones, fallback=torch.zeros(J))
    with pytest.raises(RuntimeError, match="'seen'"):
        ops.track_bones(dets, count, track, PARENT, dict(bones, seen=bones["seen"].long()))
    with pytest.raises(RuntimeError, match="'slots'"):
        ops.track_bones(dets, count, dict(track, slots=track["slots"].long()), PARENT, bones)
    with pytest.raises(RuntimeError, match="joints"):
        ops.track_bones(dets, count, track, bones_cases.H36M17_PARENT, bones)
    with pytest.raises(_lib.MvgError, match="tree"):
        ops.track_bones(dets, count, track, (-1,) + (3,) * (J - 1), bones)
    for bad in (dict(W=0), dict(W=33), dict(T=65), dict(J=18), dict(J=1), dict(R=16385), dict(B=0)):
        with pytest.raises(_lib.MvgError):
            ops.track_bones_buffers(**{**dict(B=1, T=4, J=15, R=8, W=8, device="cpu"), **bad})
    # the stage object
    est = structural.BoneLengthEstimator(batch=1, rows=R, max_tracks=T, window=W, min_frames=2, fallback=[250.0] * (J - 1), device="cpu")
    assert len(est.tensors()) == 7 and est.row_length is est.buffers["row_length"] and est.lengths() == [{}]
    est.buffers["owner"][0, 1], est.buffers["seen"][0, 1] = 9, 3
    est.buffers["length"][0, 1] = torch.arange(J - 1, dtype=torch.float32)
    got = est.lengths()
    assert list(got[0]) == [9] and got[0][9][1] == 3 and got[0][9][0].tolist() == list(range(J - 1))
    saved = est.snapshot()
    est.reset()
    assert est.lengths() == [{}] and bool((est.row_source == -1).all())
    assert est.restore(saved).lengths()[0][9][1] == 3
    for bad in (dict(window=0), dict(window=33), dict(min_frames=0)):
        with pytest.raises(ValueError, match="window"):
            structural.BoneLengthEstimator(batch=1, rows=R, max_tracks=T, device="cpu", **bad)
    with pytest.raises(ValueError, match="fallback"):
        structural.BoneLengthEstimator(batch=1, rows=R, max_tracks=T, device="cpu", fallback=[1.0, 2.0])
    # the refiner takes the row tensor by reference, and only in its own shape
    ref = structural.StructuralRefiner(batch=1, rows=R, bone_lengths=est.row_length, device="cpu")
    assert ref.bone_lengths is est.row_length
    with pytest.raises(ValueError, match="per-person"):
        structural.StructuralRefiner(batch=1, rows=R + 1, bone_lengths=est.row_length, device="cpu")
    # the pipeline: track lengths need the tracker, and their keys belong to them
    args = dict(batch=1, num_queries=16, num_joints=J, threshold=0.1, device="cpu", postprocess={})
    with pytest.raises(ValueError, match="requires tracking"):
        PostProcess(refine=dict(bone_lengths="track"), **args)
    with pytest.raises(ValueError, match="bone_lengths"):
        PostProcess(refine=dict(bone_lengths="tracks"), tracking={}, **args)
    with pytest.raises(TypeError, match="belong to"):
        PostProcess(refine=dict(bone_lengths=[200.0] * (J - 1), window=4), **args)
    with pytest.raises(TypeError, match="unknown refine keys"):
        PostProcess(refine=dict(bone_lengths="track", frames=4), tracking={}, **args)


def test_validate_parser_knows_track_lengths(capsys):
    from mvgformer_amd import validate
    cfg = ["--cfg", "extract:configs/panoptic/knn5-lr4-q1024-g8.yaml", "--device-nms", "1", "--device-refine", "1", "--bone-lengths", "track"]
    with pytest.raises(SystemExit) as e:
        validate.main(cfg)
    assert e.value.code == 2 and "--device-track 1" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        validate.main(cfg + ["--device", "cpu", "--device-track", "1", "--bone-window", "4", "--bone-min-frames", "2"])
    assert e.value.code == "Not implemented on the CPU"
