"""The tracker's constant-velocity motion model on the device (csrc/track.hip mvg_track_predict / mvg_track_correct ->
ops.track_predict / track_correct -> tracking.PoseTracker(motion=...)) against the fp64 restatement of tests/track_motion_ref.py,
chained with tests/track_ref.py for the update: frame by frame, ids, slots, every tracker state buffer, mean, var and row_pose
equal as BYTES, on the sequences of tests/track_motion_ref.py, whose preconditions tests/test_track_motion_cpu.py checks.
B <= 2, T <= 8, J = 15, R <= 8."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from mvgformer_amd import _lib, ops
from mvgformer_amd.tracking import PoseTracker
from tests import track_motion_ref as MR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STATE_KEYS = ("id", "hits", "misses", "born", "score", "pose", "next_id", "state", "ids", "slots")
MOTION_KEYS = ("mean", "var", "row_pose")


@functools.lru_cache(maxsize=None)
def _sequences():
    return MR.sequences()


@functools.lru_cache(maxsize=None)
def _reference_run(name, motion=True):
    """the restatement over the sequence, computed once and left unchanged"""
    return MR.run(_sequences()[name], "seq" if motion else None)


def _tracker(seq, motion="seq"):
    B, R, J = seq["frames"][0][0].shape[:3]
    return PoseTracker(batch=B, rows=R, num_joints=J, max_tracks=seq["T"], max_dist=seq["max_dist"], max_misses=seq["max_misses"],
                       min_hits=seq["min_hits"], device=DEV, motion=seq["motion"] if motion == "seq" else motion)


def _snap(tracker):
    out = MR.live_only({k: t.cpu().numpy() for k, t in tracker.buffers.items()})
    out.update({k: t.cpu().numpy() for k, t in (tracker.motion_buffers or {}).items()})
    return out


def _feed(tracker, frame):
    dets, count = frame
    return tracker.update(torch.from_numpy(dets).to(DEV), None if count is None else torch.from_numpy(count).to(DEV))


def _device_run(name, motion="seq"):
    seq = _sequences()[name]
    tracker = _tracker(seq, motion)
    snaps = []
    for frame in seq["frames"]:
        ids, slots = _feed(tracker, frame)
        assert ids is tracker.buffers["ids"] and slots is tracker.buffers["slots"]
        snaps.append(_snap(tracker))
    return snaps, tracker


def _assert_same(got, want, keys, what):
    for f, (g, w) in enumerate(zip(got, want)):
        for k in keys:
            assert g[k].dtype == w[k].dtype and g[k].shape == w[k].shape, (what, f, k)
            assert g[k].tobytes() == w[k].tobytes(), (what, f, k, g[k], w[k])


@pytest.mark.parametrize("name", sorted(MR.sequences()))
def test_motion_tracker_equals_the_restatement_frame_by_frame(name):
    want = _reference_run(name)
    got, tracker = _device_run(name)
    assert len(got) == len(want)
    _assert_same(got, want, STATE_KEYS + MOTION_KEYS, name)
    # the read-backs: tracks() gives the filtered pose, motion() velocity and covariance of the live slots
    last = want[-1]
    for b, (tracks, motion) in enumerate(zip(tracker.tracks(), tracker.motion())):
        assert [t.slot for t in tracks] == sorted(motion) == [t for t in range(tracker.max_tracks) if last["id"][b, t] >= 0]
        for t in tracks:
            assert t.pose.tobytes() == last["pose"][b, t.slot].tobytes()
            vel, var = motion[t.slot]
            assert vel.tobytes() == last["mean"][b, t.slot, :, 1].tobytes() and var == tuple(last["var"][b, t.slot].tolist())
    assert tracker.row_poses is tracker.motion_buffers["row_pose"]
    print(name, tracker.state())


def test_ids_follow_the_persons_through_occlusion_and_crossing():
    """read from the device's ids: the occluded walker keeps id 0 and the crossing pair keep theirs with the motion model; without
    it (the same tracker, motion=None) the walker comes back as id 1 and the pair swap"""
    seqs = _sequences()
    got, tracker = _device_run("walk_occluded")
    hist = MR.ids_per_person(seqs["walk_occluded"], got)
    assert all(h[0] in ({}, {0: 0}) for h in hist) and hist[-1][0] == {0: 0} and tracker.state()["births"] == 1
    got, tracker = _device_run("walk_occluded", None)
    assert MR.ids_per_person(seqs["walk_occluded"], got)[-1][0] == {0: 1} and tracker.state()["deaths"] == 1
    got, _ = _device_run("cross_fast")
    hist = MR.ids_per_person(seqs["cross_fast"], got)
    assert all(h[0] == hist[0][0] for h in hist)
    got, _ = _device_run("cross_fast", None)
    hist = MR.ids_per_person(seqs["cross_fast"], got)
    assert hist[-1][0] == {0: hist[0][0][1], 1: hist[0][0][0]}


def test_two_runs_give_the_same_bits_and_reset_snapshot_restore():
    a, tracker = _device_run("two_streams")
    b, _ = _device_run("two_streams")
    _assert_same(a, b, STATE_KEYS + MOTION_KEYS, "second run")
    seq = _sequences()["two_streams"]
    # snapshot / restore: three frames on, then back, then the same three frames again give the same bits
    tracker.reset()
    for frame in seq["frames"][:4]:
        _feed(tracker, frame)
    saved = tracker.snapshot()
    assert set(saved) == set(STATE_KEYS + MOTION_KEYS)
    first = []
    for frame in seq["frames"][4:7]:
        _feed(tracker, frame)
        first.append(_snap(tracker))
    tracker.restore(saved)
    assert all(torch.equal(saved[k], t) for k, t in {**tracker.buffers, **tracker.motion_buffers}.items())
    second = []
    for frame in seq["frames"][4:7]:
        _feed(tracker, frame)
        second.append(_snap(tracker))
    _assert_same(second, first, STATE_KEYS + MOTION_KEYS, "restored")
    _assert_same(second, _reference_run("two_streams")[4:7], STATE_KEYS + MOTION_KEYS, "restored against the restatement")
    # reset: everything as allocated, and the sequence starts over
    tracker.reset()
    fresh = {**ops.track_buffers(2, 4, 15, 4, DEV), **ops.track_motion_buffers(2, 4, 15, 4, DEV)}
    assert all(torch.equal({**tracker.buffers, **tracker.motion_buffers}[k], fresh[k]) for k in fresh)
    _feed(tracker, seq["frames"][0])
    _assert_same([_snap(tracker)], a[:1], STATE_KEYS + MOTION_KEYS, "after reset")


def test_the_three_launches_are_capturable():
    """predict, update and correct in a HIP graph of their own, replayed over the whole sequence on new static inputs"""
    seq = _sequences()["walk_occluded"]
    want = _reference_run("walk_occluded")
    tracker = _tracker(seq)
    dets = torch.from_numpy(seq["frames"][0][0]).to(DEV)
    count = torch.from_numpy(seq["frames"][0][1]).to(DEV)
    saved = tracker.snapshot()
    tracker.update(dets, count)                               # warm-up outside the capture
    tracker.restore(saved)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tracker.update(dets, count)
    assert tracker.state() == dict.fromkeys(ops.TRACK_STATE, 0) and float(tracker.motion_buffers["var"].abs().sum()) == 0.0
    got = []
    for frame_dets, frame_count in seq["frames"]:
        dets.copy_(torch.from_numpy(frame_dets))
        count.copy_(torch.from_numpy(frame_count))
        graph.replay()
        torch.cuda.synchronize()
        got.append(_snap(tracker))
    _assert_same(got, want, STATE_KEYS + MOTION_KEYS, "replayed")


def test_motion_none_is_the_tracker_as_it_was():
    seq = _sequences()["cross_fast"]
    B, R, J = seq["frames"][0][0].shape[:3]
    never = PoseTracker(batch=B, rows=R, num_joints=J, max_tracks=seq["T"], max_dist=seq["max_dist"], max_misses=seq["max_misses"],
                        min_hits=seq["min_hits"], device=DEV)
    off = _tracker(seq, None)
    assert off.motion_buffers is None and off.row_poses is None and set(off.snapshot()) == set(STATE_KEYS)
    want = _reference_run("cross_fast", False)
    for f, frame in enumerate(seq["frames"]):
        _feed(never, frame)
        _feed(off, frame)
        a, b = _snap(never), _snap(off)
        _assert_same([b], [a], STATE_KEYS, "motion=None, frame %d" % f)
        _assert_same([b], [want[f]], STATE_KEYS, "motion=None against the restatement, frame %d" % f)


def test_refusals():
    tracker = PoseTracker(batch=1, rows=8, max_tracks=4, device=DEV, motion=True)
    buf, mot = tracker.buffers, tracker.motion_buffers
    for bad in (dict(dt=0.0), dict(dt=-1.0), dict(dt=float("inf")), dict(dt=float("nan")), dict(q=-1.0), dict(q=float("nan")),
                dict(q=2e15)):
        with pytest.raises(_lib.MvgError):
            ops.track_predict(buf, mot, **{**dict(dt=1.0, q=25.0), **bad})
    for bad in (dict(r=0.0), dict(r=-1.0), dict(r=float("nan")), dict(r=2e15), dict(v0=-1.0), dict(v0=float("nan")), dict(v0=2e15)):
        with pytest.raises(_lib.MvgError):
            ops.track_correct(buf, mot, **{**dict(r=400.0, v0=2500.0), **bad})
    with pytest.raises(RuntimeError, match="track_motion_buffers"):
        ops.track_predict(buf, dict(mot, mean=mot["mean"].float()))
    with pytest.raises(RuntimeError, match="track_motion_buffers"):
        ops.track_correct(buf, dict(mot, var=torch.zeros((1, 4, 4), dtype=torch.float64, device=DEV)))
    with pytest.raises(RuntimeError, match="track_motion_buffers"):
        ops.track_correct(buf, dict(mot, row_pose=torch.zeros((1, 9, 15, 3), device=DEV)))
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.track_predict(buf, dict(mot, var=torch.zeros((1, 4, 6), dtype=torch.float64, device=DEV)[..., ::2]))
    with pytest.raises(RuntimeError, match="track_buffers"):
        ops.track_correct(dict(buf, hits=buf["hits"].long()), mot)
    # the raw ABI: MVG_E_BADARG and nothing launched
    lib = _lib.load()
    p = {k: _lib.ptr(t) for k, t in {**buf, **mot}.items()}
    stream = _lib.stream_ptr()
    odd = ctypes.c_void_p(mot["mean"].data_ptr() + 4)

    def predict(B=1, T=4, J=15, ident=p["id"], pose=p["pose"], mean=p["mean"], var=p["var"], dt=1.0, q=25.0):
        return lib.mvg_track_predict(B, T, J, ident, pose, mean, var, dt, q, stream)

    def correct(B=1, R=8, T=4, J=15, ident=p["id"], hits=p["hits"], misses=p["misses"], slots=p["slots"], pose=p["pose"],
                mean=p["mean"], var=p["var"], r=400.0, v0=2500.0, row_pose=p["row_pose"]):
        return lib.mvg_track_correct(B, R, T, J, ident, hits, misses, slots, pose, mean, var, r, v0, row_pose, stream)

    badarg = 10001                                                              # MVG_E_BADARG
    assert predict(B=0) == badarg
    for kw in (dict(B=4097), dict(T=0), dict(T=65), dict(J=0), dict(J=33), dict(ident=None), dict(pose=None), dict(mean=None),
               dict(var=None), dict(mean=odd), dict(var=odd), dict(dt=0.0), dict(dt=-1.0), dict(dt=float("inf")),
               dict(dt=float("nan")), dict(q=-1.0), dict(q=float("nan")), dict(q=2e15)):
        assert predict(**kw) == badarg, kw
    for kw in (dict(B=0), dict(B=4097), dict(R=0), dict(R=16385), dict(T=0), dict(T=65), dict(J=0), dict(J=33), dict(ident=None),
               dict(hits=None), dict(misses=None), dict(slots=None), dict(pose=None), dict(mean=None), dict(var=None),
               dict(row_pose=None), dict(mean=odd), dict(var=odd), dict(r=0.0), dict(r=-1.0), dict(r=float("nan")), dict(r=2e15),
               dict(v0=-1.0), dict(v0=float("nan")), dict(v0=2e15)):
        assert correct(**kw) == badarg, kw
    torch.cuda.synchronize()
    fresh = {**ops.track_buffers(1, 4, 15, 8, DEV), **ops.track_motion_buffers(1, 4, 15, 8, DEV)}
    assert all(torch.equal({**buf, **mot}[k], fresh[k]) for k in fresh)          # nothing was launched
    assert predict() == 0 and correct() == 0
    torch.cuda.synchronize()
