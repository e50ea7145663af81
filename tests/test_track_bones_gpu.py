"""mvg_track_bones (csrc/bones.hip) against its numpy restatement (tests/bones_ref.py) as BITS -- owner, seen, hist, length, row_length,
row_source -- after EVERY frame of sequences that the real tracker (ops.track_update, with and without its motion model) drives:
2 W + 3 frames, so the ring wraps; persons leave and enter, so slots are freed and reopened; one row carries a NaN and one an Inf.
A length that is NaN (a row's own lengths, source 2) is compared as "NaN on both sides": the contract names no payload."""
import ctypes

import numpy as np
import pytest
import torch

from mvgformer_amd import _lib, ops
from tests import bones_cases, bones_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BADARG = 10001                  # MVG_E_BADARG


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(got, want):
    """equal bits, or NaN on both sides"""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype.kind != "f":
        return np.array_equal(got, want)
    both_nan = np.isnan(got) & np.isnan(want)
    return np.array_equal(np.where(both_nan, 0, got.view(np.uint32)), np.where(both_nan, 0, want.view(np.uint32)))


def _fallback(J):
    return np.linspace(210.0, 390.0, J - 1).astype(np.float32)


def _drive(frames, T, W, variants, motion=False, no_count=False):
    """the frames through the real tracker and one launch of mvg_track_bones per variant (min_frames, fallback or None) and
    frame -> per frame dict(slots, id, unchanged, bufs: one dict of numpy arrays per variant)"""
    B, R, J = frames[0][0].shape[:3]
    parent = bones_cases.PARENTS[J]
    track = ops.track_buffers(B, T, J, R, DEV)
    mot = ops.track_motion_buffers(B, T, J, R, DEV) if motion else None
    bufs = [ops.track_bones_buffers(B, T, J, R, W, DEV) for _ in variants]
    falls = [None if fb is None else torch.from_numpy(fb).to(DEV) for _, fb in variants]
    out = []
    for dets, count in frames:
        d = torch.from_numpy(dets).to(DEV)
        c = None if no_count else torch.from_numpy(count).to(DEV)
        if motion:
            ops.track_predict(track, mot)
        ops.track_update(d, c, track, 500.0, 1, 1)
        if motion:
            ops.track_correct(track, mot)
        theirs = dict(track, **(mot or {}))
        before = {k: v.clone() for k, v in theirs.items()}
        for (min_frames, _), fb, buf in zip(variants, falls, bufs):
            ops.track_bones(d, c, track, parent, buf, min_frames, fb)
        torch.cuda.synchronize()
        out.append(dict(slots=track["slots"].cpu().numpy(), id=track["id"].cpu().numpy(),
                        unchanged=all(torch.equal(_bits(before[k]), _bits(v)) for k, v in theirs.items()),
                        bufs=[{k: v.cpu().numpy() for k, v in buf.items()} for buf in bufs]))
    return out


def _check_against_restatement(frames, got, T, W, variants, no_count=False):
    B, R, J = frames[0][0].shape[:3]
    parent = bones_cases.PARENTS[J]
    want = bones_ref.new_buffers(B, T, J, R, W)
    sources = set()
    for f, ((dets, count), g) in enumerate(zip(frames, got)):
        count = None if no_count else count
        assert g["unchanged"], "frame %d: the launch wrote to the tracker's buffers" % f
        bones_ref.advance(dets, count, g["slots"], g["id"], parent, want)
        for v, ((min_frames, fb), dev) in enumerate(zip(variants, g["bufs"])):
            bones_ref.rows(dets, count, g["slots"], parent, want, min_frames, fb)
            for k in bones_ref.STATE + bones_ref.OUTPUTS:
                assert _same(dev[k], want[k]), "frame %d, variant %d: %s differs" % (f, v, k)
            sources |= set(np.unique(dev["row_source"]).tolist())
    return want, sources


@pytest.mark.parametrize("motion", [False, True])
@pytest.mark.parametrize("W", [1, 2, 5, 32])
@pytest.mark.parametrize("J", [15, 17])
@pytest.mark.parametrize("R", [8, 80])
@pytest.mark.parametrize("T", [4, 64])
def test_every_frame_equals_the_restatement(T, R, J, W, motion):
    """B = 2; min_frames in {1, 3, W + 1} x fallback given / NULL are six launches per frame on six sets of buffers over the same
    tracker state (the state they keep does not depend on either; the rows do)"""
    frames = bones_cases.sequence(J, R, W)
    assert len(frames) == 2 * W + 3
    variants = [(m, fb) for m in (1, 3, W + 1) for fb in (_fallback(J), None)]
    got = _drive(frames, T, W, variants, motion)
    want, sources = _check_against_restatement(frames, got, T, W, variants)
    # the sequence does what it is for: every source occurs, the ring wrapped, a slot changed hands, the bad rows were tracked
    assert sources == {-1, 0, 1, 2}
    assert want["seen"].max() > W
    owners = np.stack([g["bufs"][0]["owner"] for g in got])
    if W > 1:                                                       # 2 W + 3 >= 7 frames: person 2 has left and a slot was reopened
        assert any(len(set(owners[:, b, t].tolist()) - {-1}) > 1 for b in range(2) for t in range(T))
    if R == 8:                                                      # (behind a crowd the row has no slot)
        for f, bad in ((3, np.isnan), (5, np.isinf)):
            if f < len(frames):
                row = [i for i in range(R) if bad(frames[f][0][0, i]).any()]
                assert len(row) == 1 and got[f]["slots"][0, row[0]] >= 0
    if R > 64 and len(frames) > 4:
        assert any(((g["slots"][0] < 0) & (fr[0][0, :, 0, 3] >= 0)).any() for fr, g in zip(frames, got))


@pytest.mark.parametrize("mode", ["null", "zero", "above"])
def test_count_null_zero_and_above_the_rows(mode):
    J, R, T, W = 15, 8, 4, 2
    frames = bones_cases.sequence(J, R, W)
    if mode == "zero":
        frames = [(d, np.zeros_like(c)) for d, c in frames]
    if mode == "above":
        frames = [(d, c + R + 5) for d, c in frames]
    variants = [(1, None), (2, _fallback(J))]
    got = _drive(frames, T, W, variants, no_count=mode == "null")
    want, sources = _check_against_restatement(frames, got, T, W, variants, no_count=mode == "null")
    assert (sources == {-1}) if mode == "zero" else (0 in sources and want["seen"].max() > W)


def test_hand_made_slots_with_a_duplicate_and_an_index_outside():
    J, R, T, W = 17, 8, 4, 5
    parent = bones_cases.PARENTS[J]
    frames = bones_cases.sequence(J, R, W)[:4]
    track = ops.track_buffers(2, T, J, R, DEV)
    track["id"].copy_(torch.tensor([[5, -1, 6, 7], [1, 2, -1, -1]], dtype=torch.int32))
    made = np.array([[2, 2, T, 0, 2, -1, 3, 3], [T + 60, 1, 1, 0, -7, 0, 1, 0]], np.int32)
    track["slots"].copy_(torch.from_numpy(made))
    buf = ops.track_bones_buffers(2, T, J, R, W, DEV)
    want = bones_ref.new_buffers(2, T, J, R, W)
    for dets, count in frames:
        count = np.full_like(count, R)
        dets = dets.copy()
        dets[:, :, :, 3] = 1.0                                     # every row a detection (rows without a person are all zeros)
        ops.track_bones(torch.from_numpy(dets).to(DEV), torch.from_numpy(count).to(DEV), track, parent, buf, 2, None)
        torch.cuda.synchronize()
        bones_ref.update(dets, count, made, track["id"].cpu().numpy(), parent, want, 2, None)
        for k in bones_ref.STATE + bones_ref.OUTPUTS:
            assert _same(buf[k].cpu().numpy(), want[k]), k
    # one sample per frame for every named slot, whatever the number of rows that name it; slot 1 of stream 0 is never named
    # (slot 2 of stream 0 takes none in frame 3, where the lowest row that names it carries a NaN)
    assert want["seen"].tolist() == [[4, 0, 3, 4], [4, 4, 0, 0]]


def test_a_stream_does_not_depend_on_the_other_and_runs_repeat():
    J, R, T, W = 15, 80, 64, 5
    frames = bones_cases.sequence(J, R, W)
    variants = [(3, None)]
    rng = np.random.default_rng(0)
    perm = rng.permutation(R)
    shuffled = []
    for dets, count in frames:
        d = dets.copy()
        d[1] = dets[1][perm]                                       # the other stream's rows in another order, all R looked at
        shuffled.append((d, np.array([count[0], [R, 0]], np.int32)))
    alone = [(dets[:1].copy(), count[:1].copy()) for dets, count in frames]
    a, again, b, c = (_drive(fr, T, W, variants) for fr in (frames, frames, shuffled, alone))
    for f in range(len(frames)):
        for k in bones_ref.STATE + bones_ref.OUTPUTS:
            first = a[f]["bufs"][0][k]
            assert _same(first, again[f]["bufs"][0][k]), (f, k)    # two identical runs: identical bits
            assert _same(first[0], b[f]["bufs"][0][k][0]) and _same(first[0], c[f]["bufs"][0][k][0]), (f, k)
    assert not _same(a[-1]["bufs"][0]["row_source"][1], b[-1]["bufs"][0]["row_source"][1])      # the other stream did change


def test_raw_abi_refusals_launch_nothing():
    J, R, T, W = 15, 8, 4, 8
    lib = _lib.load()
    track = ops.track_buffers(1, T, J, R, DEV)
    buf = ops.track_bones_buffers(1, T, J, R, W, DEV)
    dets = torch.zeros((1, R, J, 5), device=DEV)
    dets[..., 3] = -1.0                                              # no row is a detection
    count = torch.full((1, 2), R, dtype=torch.int32, device=DEV)
    fallback = torch.ones((J - 1,), device=DEV)
    for k in buf:
        buf[k].fill_(77)
    tree = (ctypes.c_int * J)(*bones_cases.PARENTS[J])
    loop = (ctypes.c_int * J)(-1, 2, 1, *([0] * (J - 3)))           # joints 1 and 2 hang from each other
    far = (ctypes.c_int * J)(-1, J, *([0] * (J - 2)))               # a parent outside the joints
    rooted = (ctypes.c_int * J)(0, *([0] * (J - 1)))                # parent[0] is not -1
    stream = _lib.stream_ptr()

    def call(B=1, R=R, J=J, T=T, W=W, min_frames=1, parent=tree, **ptr):
        p = dict(dets=dets, count=count, slots=track["slots"], id=track["id"], fallback=fallback, **buf)
        p.update(ptr)
        return lib.mvg_track_bones(p["dets"], p["count"], p["slots"], p["id"], parent, B, R, J, T, W, min_frames, p["fallback"],
                                   p["owner"], p["seen"], p["hist"], p["length"], p["row_length"], p["row_source"], stream)

    for kw in (dict(B=0), dict(B=4097), dict(R=0), dict(R=16385), dict(T=0), dict(T=65), dict(J=1), dict(J=18), dict(W=0), dict(W=33),
               dict(min_frames=0), dict(min_frames=-3), dict(parent=None), dict(parent=loop), dict(parent=far), dict(parent=rooted),
               dict(dets=None), dict(slots=None), dict(id=None), dict(owner=None), dict(seen=None), dict(hist=None),
               dict(length=None), dict(row_length=None), dict(row_source=None)):
        assert call(**kw) == BADARG, kw
    torch.cuda.synchronize()
    assert all(bool((t == 77).all()) for t in buf.values())          # nothing was launched
    assert call(count=None, fallback=None) == 0 and call() == 0      # the two pointers that may be NULL
    torch.cuda.synchronize()
    assert bool((buf["row_source"] == -1).all()) and not buf["row_length"].any() and bool((buf["owner"] == -1).all())
