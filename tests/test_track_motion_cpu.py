"""The tracker's constant-velocity motion model (csrc/track.hip mvg_track_predict / mvg_track_correct, ops.track_predict /
track_correct, tracking.PoseTracker(motion=...), validate --device-track-motion): what can be checked without a GPU -- the
restatement of tests/track_motion_ref.py against a textbook matrix Kalman filter, the test sequences and their preconditions, the
C-ABI surface, the refusals, the argument parser.  The device numerics are in tests/test_track_motion_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from mvgformer_amd import _lib, ops
from tests import track_motion_ref as MR
from tests import track_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mvg_track_predict", "mvg_track_correct")


# ------------------------------------------------------------------------------------------- the restatement is a Kalman filter
def _textbook(history, z, dt, q, r, v0):
    """per axis x = [position, velocity], F = [[1, dt], [0, 1]], Q = q [[dt^4/4, dt^3/2], [dt^3/2, dt^2]], H = [1, 0], numpy 2 x 2
    matrices; history[f] True = a detection z[f] in frame f (frame 0 is the birth) -> per frame (x (2), P (2, 2))"""
    F = np.array([[1.0, dt], [0.0, 1.0]])
    Q = q * np.array([[dt ** 4 / 4.0, dt ** 3 / 2.0], [dt ** 3 / 2.0, dt ** 2]])
    H = np.array([[1.0, 0.0]])
    x, P = np.array([z[0], 0.0]), np.array([[r, 0.0], [0.0, v0]])
    out = [(x, P)]
    for f in range(1, len(history)):
        x, P = F @ x, F @ P @ F.T + Q
        if history[f]:
            S = H @ P @ H.T + r
            K = P @ H.T / S
            x = x + (K * (z[f] - H @ x)).ravel()
            P = (np.eye(2) - K @ H) @ P
        out.append((x, P))
    return out


@pytest.mark.parametrize("seed,dt,q,r,v0", [(0, 1.0, 25.0, 400.0, 2500.0), (1, 0.5, 100.0, 225.0, 1e4), (2, 2.0, 0.0, 50.0, 0.0),
                                            (3, 1.0 / 30.0, 9e4, 400.0, 4e6)])
def test_restatement_equals_a_textbook_kalman_filter(seed, dt, q, r, v0):
    """random hit / miss histories of 40 frames (never more misses in a row than max_misses), one track, J = 2: the six axes are six
    independent filters with one shared covariance.  1e-12 relative, positions against the size of the positions."""
    rng = np.random.default_rng(seed)
    for trial in range(4):
        n, J = 40, 2
        history = [True] + [bool(h) for h in rng.uniform(size=n - 1) < 0.7]
        z = np.cumsum(rng.normal(scale=30.0 * dt, size=(n, J, 3)), axis=0) + rng.uniform(-2000.0, 2000.0, size=(J, 3))
        z = z.astype(np.float32).astype(np.float64)
        buf, mot = TR.new_buffers(1, 2, J, 2), MR.new_motion(1, 2, J, 2)
        want = [[_textbook(history, z[:, j, a], dt, q, r, v0) for a in range(3)] for j in range(J)]
        for f in range(n):
            dets = np.zeros((1, 2, J, 5), np.float32)
            dets[..., 3] = -1.0
            if history[f]:
                dets[0, 0, :, :3], dets[0, 0, :, 3] = z[f], 1.0
            MR.step(dets, None, buf, mot, dict(dt=dt, q=q, r=r, v0=v0), 1e9, n, 1)       # gate and max_misses out of the way
            assert buf["id"][0].tolist() == [0, -1] and int(buf["misses"][0, 0] == 0) == int(history[f])
            P = want[0][0][f][1]
            got_P = mot["var"][0, 0]
            assert np.allclose(got_P, [P[0, 0], P[0, 1], P[1, 1]], rtol=1e-12, atol=0.0), (f, got_P, P)
            assert abs(P[0, 1] - P[1, 0]) <= 1e-12 * abs(P[0, 1])
            for j in range(J):
                for a in range(3):
                    x = want[j][a][f][0]
                    scale = max(abs(x[0]), 1.0)
                    assert abs(mot["mean"][0, 0, j, 0, a] - x[0]) <= 1e-12 * scale, (f, j, a)
                    assert abs(mot["mean"][0, 0, j, 1, a] - x[1]) <= 1e-12 * max(scale / dt, abs(x[1])), (f, j, a)
            # a missed track's pose is the prediction; fp32 of the mean either way
            assert np.array_equal(buf["pose"][0, 0], mot["mean"][0, 0, :, 0].astype(np.float32))
        assert np.all(mot["mean"][0, 1] == 0.0) and np.all(mot["var"][0, 1] == 0.0)       # the free slot


# ------------------------------------------------------------------------------------------------------------------ the sequences
def _no_near_ties(seq):
    """with the motion model on, in every frame: no cost within 1e-6 mm of the gate, and the best total of the padded, gated
    problem more than 1e-6 mm from the second best assignment (brute force; at most 3 tracks and 3 detections here)"""
    B, R, J = seq["frames"][0][0].shape[:3]
    buf, mot = TR.new_buffers(B, seq["T"], J, R), MR.new_motion(B, seq["T"], J, R)
    p = seq["motion"]
    for dets, count in seq["frames"]:
        MR.predict(buf, mot, p["dt"], p["q"])
        for b in range(B):
            rows = [r for r in range(R if count is None else int(count[b, 0])) if dets[b, r, 0, 3] >= 0]
            active = [t for t in range(seq["T"]) if buf["id"][b, t] >= 0]
            if not rows or not active:
                continue
            c = np.array([[TR.joint_cost(buf["pose"][b, t], dets[b, r]) for r in rows] for t in active])
            assert not (np.abs(c - seq["max_dist"]) <= 1e-6).any()
            assert max(c.shape) <= 3
            best, second = TR.brute_force(np.where(c <= seq["max_dist"], c, seq["max_dist"]))
            finite = c[c == c]
            if second - best <= 1e-6:               # only where nothing is in the gate: every assignment then matches nobody
                assert not (finite <= seq["max_dist"]).any()
        TR.update(dets, count, buf, seq["max_dist"], seq["max_misses"], seq["min_hits"])
        MR.correct(buf, mot, p["r"], p["v0"])


@pytest.mark.parametrize("name", sorted(MR.sequences()))
def test_sequences_have_no_near_ties(name):
    _no_near_ties(MR.sequences()[name])


def test_walk_occluded_keeps_its_id_only_with_the_motion_model():
    seq = MR.walk_occluded()
    assert seq["max_misses"] == 10 and seq["max_dist"] == 500.0 and seq["motion"] == MR.DEFAULTS
    seen = [int(c[0, 0]) for _, c in seq["frames"]]
    assert seen == [1] * 12 + [0] * 10 + [1] * 3
    back = 22
    # 60 mm per frame: the return is 660 mm from the last seen pose
    last, ret = seq["frames"][11][0][0, 0], seq["frames"][back][0][0, 0]
    assert 650.0 < TR.joint_cost(last[:, :3], ret) < 670.0
    plain = MR.run(seq, None)
    hist = MR.ids_per_person(seq, plain)
    assert hist[11][0] == {0: 0} and hist[back][0] == {0: 1}                  # without the motion model: a new id
    assert plain[back - 1]["misses"][0, 0] == 10 and plain[back - 1]["id"][0, 0] == 0
    with_motion = MR.run(seq)
    hist = MR.ids_per_person(seq, with_motion)
    assert all(h[0] == {0: 0} for h, n in zip(hist, seen) if n) and with_motion[-1]["state"][2] == 1      # one birth
    assert with_motion[back - 1]["misses"][0, 0] == 10 and with_motion[back]["misses"][0, 0] == 0
    # the prediction the returning detection met: the coasting mean one more step ahead
    before = with_motion[back - 1]["mean"][0, 0]
    predicted = (before[:, 0] + before[:, 1]).astype(np.float32)
    dist = TR.joint_cost(predicted, ret)
    print("prediction to return: %.2f mm" % dist)
    assert dist < seq["max_dist"] / 2.0


def test_cross_fast_swaps_ids_only_without_the_motion_model():
    seq = MR.cross_fast()
    a = [f[0][0][list(w[0]).index(0), 0, :3] for f, w in zip(seq["frames"], seq["persons"])]
    b = [f[0][0][list(w[0]).index(1), 0, :3] for f, w in zip(seq["frames"], seq["persons"])]
    steps = np.diff(np.array(a), axis=0)[:, 0], np.diff(np.array(b), axis=0)[:, 0]
    assert np.all(np.abs(steps[0] - 80.0) < 2.5) and np.all(np.abs(steps[1] + 80.0) < 2.5)
    assert all(abs((q[1] - p[1]) - 50.0) < 2.5 for p, q in zip(a, b))
    plain = MR.ids_per_person(seq, MR.run(seq, None))
    assert plain[0][0] == {0: 0, 1: 1} or plain[0][0] == {0: 1, 1: 0}
    assert plain[-1][0] == {0: plain[0][0][1], 1: plain[0][0][0]}             # swapped
    with_motion = MR.ids_per_person(seq, MR.run(seq))
    assert all(h[0] == with_motion[0][0] for h in with_motion) and sorted(with_motion[0][0].values()) == [0, 1]


def test_noisy_walk_is_smoothed():
    seq = MR.noisy_walk()
    snaps = MR.run(seq)
    raw, filtered = [], []
    for f in range(6, len(seq["frames"])):                                     # the frames after frame 5
        truth = seq["truth"][f]
        noise = seq["frames"][f][0][0, 0, :, :3].astype(np.float64) - truth
        assert np.abs(noise).max() <= 5.0 + 1e-3                               # +-5 mm, and the fp32 rounding of the input
        raw.append(np.mean(noise ** 2))
        assert snaps[f]["slots"][0, 0] == 0
        filtered.append(np.mean((snaps[f]["row_pose"][0, 0].astype(np.float64) - truth) ** 2))
        assert np.array_equal(snaps[f]["row_pose"][0, 0], snaps[f]["pose"][0, 0])
    raw, filtered = float(np.sqrt(np.mean(raw))), float(np.sqrt(np.mean(filtered)))
    print("RMS to the true line: raw %.3f mm, filtered %.3f mm" % (raw, filtered))
    assert filtered < raw


def test_further_cases_do_what_their_names_say():
    seq = MR.reborn()
    snaps = MR.run(seq)
    live = [t for t in range(seq["T"]) if snaps[2]["id"][0, t] >= 0]
    died = [t for t in live if snaps[3]["id"][0, t] != snaps[2]["id"][0, t]]
    assert len(died) == 1 and snaps[3]["id"][0, died[0]] == 2 and snaps[3]["hits"][0, died[0]] == 1      # freed and reopened
    assert snaps[3]["state"][3] == 1 and np.all(snaps[3]["mean"][0, died[0], :, 1] == 0.0)
    assert snaps[3]["var"][0, died[0]].tolist() == [400.0, 0.0, 2500.0]
    seq = MR.nan_pose()
    snaps, plain = MR.run(seq), MR.run(seq, None)
    assert all(np.array_equal(s["ids"], p["ids"]) and np.array_equal(s["state"], p["state"]) for s, p in zip(snaps, plain))
    nan_slots = [t for t in range(seq["T"]) if np.isnan(snaps[2]["mean"][0, t]).any()]
    assert len(nan_slots) == 1 and int(np.isnan(snaps[3]["mean"][0, nan_slots[0]]).sum()) == 1
    assert int(np.isnan(snaps[3]["pose"]).sum()) == 1 and not np.isnan(snaps[-1]["mean"]).any()          # it died, zeros again
    seq = MR.two_streams()
    snaps = MR.run(seq)
    assert snaps[4]["misses"][0].max() == 2 and snaps[-1]["state"][2] == 4 and snaps[-1]["state"][3] == 0
    assert MR.sequences()["dt_half"]["motion"]["dt"] == 0.5


# ------------------------------------------------------------------------------------------------------------- surface, refusals
def test_symbols_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvg_decoder.h")).read(), flags=re.S)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in _lib.SIGNATURES and hasattr(lib, s), s
        params = re.search(r"\b%s\s*\((.*?)\)\s*;" % s, header, flags=re.S).group(1).split(",")
        assert len(params) == len(_lib.SIGNATURES[s]), s
        doubles = [i for i, p in enumerate(params) if p.strip().startswith("double ")]
        assert [i for i, t in enumerate(_lib.SIGNATURES[s]) if t is ctypes.c_double] == doubles and len(doubles) == 2, s


def test_cpu_tensors_and_bad_options_are_refused():
    from mvgformer_amd import tracking
    motion = ops.track_motion_buffers(2, 4, 15, 8, "cpu")
    assert set(motion) == {"mean", "var", "row_pose"}
    assert tuple(motion["mean"].shape) == (2, 4, 15, 2, 3) and motion["mean"].dtype == torch.float64
    assert tuple(motion["var"].shape) == (2, 4, 3) and motion["var"].dtype == torch.float64
    assert tuple(motion["row_pose"].shape) == (2, 8, 15, 3) and motion["row_pose"].dtype == torch.float32
    assert all(int((t != 0).sum()) == 0 for t in motion.values())
    buffers = ops.track_buffers(2, 4, 15, 8, "cpu")
    assert set(buffers) == {"id", "hits", "misses", "born", "score", "pose", "next_id", "state", "ids", "slots"}
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.track_predict(buffers, motion, 1.0, 25.0)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.track_correct(buffers, motion, 400.0, 2500.0)
    for bad in (dict(T=65), dict(J=33), dict(R=16385), dict(B=0)):
        with pytest.raises(_lib.MvgError):
            ops.track_motion_buffers(**{**dict(B=1, T=4, J=15, R=8, device="cpu"), **bad})
    tracker = tracking.PoseTracker(batch=1, rows=8, device="cpu", motion=True)
    assert tracker.motion_params == dict(dt=1.0, q=25.0, r=400.0, v0=2500.0) == MR.DEFAULTS
    assert tuple(tracker.row_poses.shape) == (1, 8, 15, 3) and tracker.motion() == [{}] and tracker.tracks() == [[]]
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        tracker.update(torch.zeros((1, 8, 15, 5)))
    assert tracking.PoseTracker(batch=1, rows=8, device="cpu", motion=dict(dt=0.5)).motion_params["dt"] == 0.5
    plain = tracking.PoseTracker(batch=1, rows=8, device="cpu")
    assert plain.motion_params is None and plain.motion_buffers is None and plain.row_poses is None
    assert set(plain.snapshot()) == set(plain.buffers) and set(tracker.snapshot()) == set(plain.buffers) | set(motion)
    with pytest.raises(RuntimeError, match="without motion"):
        plain.motion()
    with pytest.raises(TypeError, match="unknown motion keys"):
        tracking.PoseTracker(batch=1, rows=8, device="cpu", motion=dict(model="kalman"))
    for bad in (dict(dt=0.0), dict(dt=-1.0), dict(dt=float("inf")), dict(dt=float("nan")), dict(q=-1.0), dict(q=float("nan")),
                dict(q=2e15), dict(r=0.0), dict(r=float("nan")), dict(r=2e15), dict(v0=-1.0), dict(v0=float("nan")), dict(v0=2e15)):
        with pytest.raises(ValueError, match="motion"):
            tracking.PoseTracker(batch=1, rows=8, device="cpu", motion=bad)
    # reset / snapshot / restore cover the motion buffers
    tracker.motion_buffers["mean"].fill_(3.0)
    saved = tracker.snapshot()
    assert float(tracker.reset().motion_buffers["mean"].abs().sum()) == 0.0 and int(tracker.buffers["id"].max()) == -1
    assert float(tracker.restore(saved).motion_buffers["mean"].min()) == 3.0


def test_validate_parser_knows_device_track_motion(capsys):
    from mvgformer_amd import validate
    cfg = ["--cfg", "extract:configs/panoptic/knn5-lr4-q1024-g8.yaml"]
    with pytest.raises(SystemExit) as e:
        validate.main(cfg + ["--device-track-motion", "1", "--device-nms", "1"])
    assert e.value.code == 2 and "--device-track 1" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        validate.main(cfg + ["--device", "cpu", "--device-track-motion", "1", "--device-track", "1", "--device-nms", "1"])
    assert e.value.code == "Not implemented on the CPU"
