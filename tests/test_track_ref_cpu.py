"""Device-side person tracking (csrc/track.hip, ops.linear_assignment / track_update, tracking.PoseTracker, validate
--device-track): what can be checked without a GPU -- the restated solver against brute force and scipy, the preconditions of
the float-valued test sequences, the C-ABI surface, the refusals, the argument parser.  The device numerics are in
tests/test_track_gpu.py."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

from mvgformer_amd import _lib, ops
from tests import track_cases as TC
from tests import track_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mvg_linear_assignment", "mvg_track_update")


# ------------------------------------------------------------------------------------------------------------ the restated solver
def _check_assignment(col, n, m):
    live = [c for c in col[:n] if c >= 0]
    assert len(live) == min(n, m) and len(set(live)) == len(live) and all(0 <= c < m for c in live)
    assert all(c == -1 for c in col[n:])


@pytest.mark.parametrize("n,m", [(n, m) for n in range(1, 8) for m in range(1, 8)])
def test_restated_solver_against_brute_force(n, m):
    rng = np.random.default_rng(100 * n + m)
    for trial in range(3 if max(n, m) == 7 else 6):
        cost = rng.uniform(0.0, 100.0, size=(n, m))
        col, total = TR.solve(cost)
        _check_assignment(col, n, m)
        best, _ = TR.brute_force(cost)
        assert abs(total - best) <= 1e-12 * max(abs(best), 1.0), (n, m, total, best)
        ties = rng.integers(0, 4, size=(n, m)).astype(np.float64)             # many equal totals: the optimum value is unique
        col, total = TR.solve(ties)
        _check_assignment(col, n, m)
        assert total == TR.brute_force(ties)[0]


def test_restated_solver_on_live_sizes_and_odd_entries():
    rng = np.random.default_rng(5)
    cost = rng.uniform(0.0, 10.0, size=(6, 8))
    col, total = TR.solve(cost, 4, 5)
    sub_col, sub_total = TR.solve(cost[:4, :5])
    assert list(col[:4]) == list(sub_col) and list(col[4:]) == [-1, -1] and total == sub_total
    for n, m in ((0, 7), (7, 0), (0, 0)):
        col, total = TR.solve(cost, n, m)
        assert list(col) == [-1] * 6 and total == 0.0
    # NaN, +inf and 1e300 count as 1e15 in the solve; the total adds the entries as given
    odd = np.array([[np.nan, 1.0], [2.0, np.inf]])
    col, total = TR.solve(odd)
    assert list(col) == [1, 0] and total == 3.0
    col, total = TR.solve(np.array([[np.nan, np.inf], [1e300, np.nan]]))
    assert sorted(col) == [0, 1]                                               # returns, with a full assignment
    assert list(TR.solve(np.array([[100.0, 110.0], [105.0, 300.0]]))[0]) == [1, 0]


def test_restated_solver_against_scipy():
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    rng = np.random.default_rng(6)
    shapes = [(int(rng.integers(1, 13)), int(rng.integers(1, 13))) for _ in range(300)] + [(64, 64)]
    for n, m in shapes:
        cost = rng.uniform(0.0, 1000.0, size=(n, m))
        _, total = TR.solve(cost)
        r, c = lsa(cost)
        want = float(cost[r, c].sum())
        assert abs(total - want) <= 1e-12 * max(abs(want), 1.0), (n, m)
        ties = rng.integers(0, 4, size=(n, m)).astype(np.float64)
        r, c = lsa(ties)
        assert TR.solve(ties)[1] == float(ties[r, c].sum()), (n, m)


# ------------------------------------------------------------------------------------------------ preconditions of the sequences
def _outcome_gap(c, max_dist):
    """smallest difference between the best total of the padded, gated problem and the best total of any assignment that gives
    ANOTHER set of valid matches (brute force over all permutations)"""
    na, nd = c.shape
    s = max(na, nd)
    S = np.zeros((s, s))
    S[:na, :nd] = np.where(c <= max_dist, c, max_dist)
    best = {}
    for perm in itertools.permutations(range(s)):
        key = frozenset((a, perm[a]) for a in range(na) if perm[a] < nd and c[a, perm[a]] <= max_dist)
        total = sum(S[i, perm[i]] for i in range(s))
        best[key] = min(best.get(key, np.inf), total)
    order = sorted(best.values())
    return order[1] - order[0] if len(order) > 1 else np.inf


@pytest.mark.parametrize("name", sorted(TC.float_sequences()))
def test_float_sequences_have_no_near_ties(name):
    """so that a tie cannot hide a defect: in every frame the best outcome is more than 1e-6 mm better than the second best
    (brute force, at most 6 persons and 7 tracks), and no cost lies within 1e-6 mm of the gate unless it is exactly on it by
    construction (the gate case)"""
    seq = TC.float_sequences()[name]
    dets0 = seq["frames"][0][0]
    B, R, J = dets0.shape[:3]
    buf = TR.new_buffers(B, seq["T"], J, R)
    for dets, count in seq["frames"]:
        for b in range(B):
            rows = R if count is None else int(count[b, 0])
            det_rows = [r for r in range(rows) if dets[b, r, 0, 3] >= 0][:TR.TRACK_MAX_D]
            active = [t for t in range(seq["T"]) if buf["id"][b, t] >= 0]
            if not active or not det_rows:
                continue
            c = np.array([[TR.joint_cost(buf["pose"][b, t], dets[b, r]) for r in det_rows] for t in active])
            near = np.abs(c - seq["max_dist"]) <= 1e-6
            if seq["exact"]:
                assert np.all(~near | (c == 512.0)), name
            else:
                assert not near.any(), name
            if max(c.shape) <= 7:
                assert _outcome_gap(c, seq["max_dist"]) > 1e-6, name
            else:                                  # the crowd: every person is nearest to itself by far, nobody else in the gate
                assert name == "crowd" and np.all((c <= seq["max_dist"]).sum(0) <= 1) and np.all((c <= seq["max_dist"]).sum(1) <= 1)
        TR.update(dets, count, buf, seq["max_dist"], seq["max_misses"], seq["min_hits"])


def test_sequences_do_what_their_names_say():
    """the restatement on the sequences: ids per person as the issue describes them"""
    def run(seq):
        dets0 = seq["frames"][0][0]
        B, R, J = dets0.shape[:3]
        buf = TR.new_buffers(B, seq["T"], J, R)
        hist = []
        for (dets, count), who in zip(seq["frames"], seq["persons"]):
            ids, _ = TR.update(dets, count, buf, seq["max_dist"], seq["max_misses"], seq["min_hits"])
            hist.append([{int(w): int(i) for w, i in zip(who[b], ids[b]) if w >= 0} for b in range(B)])
        return hist, dict(zip(TR.STATE, buf["state"].tolist()))
    seqs = TC.float_sequences()
    hist, st = run(seqs["walk"])
    assert all(h[0] == hist[0][0] for h in hist) and len(set(hist[0][0].values())) == 4 and st["births"] == 4 and st["frames"] == 12
    hist, _ = run(seqs["cross"])
    assert hist[0][0] == hist[1][0] == {0: 0, 1: 1}                            # greedy would swap them
    hist, st = run(seqs["occlusion"])
    assert hist[-1][0][0] == hist[0][0][0] and hist[-1][0][1] not in hist[0][0].values() and st["deaths"] == 1
    hist, st = run(seqs["overflow"])
    assert st["overflow"] == 6 and st["active"] == 4 and sorted(hist[0][0].values())[:2] == [-1, -1]
    assert run(seqs["gate_on"])[0][1][0] == {0: 0} and run(seqs["gate_off"])[0][1][0] == {0: 1}
    hist, st = run(seqs["nan_pose"])
    assert hist[2][0][1] == 2 and hist[3][0] == hist[0][0] and st["deaths"] == 1 and st["active"] == 2
    hist, _ = run(seqs["min_hits"])
    assert set(hist[0][0].values()) == set(hist[1][0].values()) == {-1} and -1 not in hist[2][0].values()
    assert run(seqs["crowd"])[1]["dropped"] == 12


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
        assert len(params) == len(_lib.SIGNATURES[s]), s                       # one ctypes entry per declared parameter


def test_defines_equal_the_ops_constants():
    header = open(os.path.join(ROOT, "include", "mvg_decoder.h")).read()
    define = lambda name: re.search(r"#define %s (\S+)" % name, header).group(1)           # noqa: E731
    assert int(define("MVG_LAP_MAX_N")) == ops.LAP_MAX_N == TR.LAP_MAX_N == 64
    assert float(define("MVG_LAP_BIG")) == ops.LAP_BIG == TR.LAP_BIG == 1e15
    assert int(define("MVG_TRACK_MAX_D")) == ops.TRACK_MAX_D == TR.TRACK_MAX_D == 64
    assert int(define("MVG_TRACK_MAX_T")) == ops.TRACK_MAX_T == TR.TRACK_MAX_T == 64
    assert int(define("MVG_TRACK_MAX_J")) == ops.TRACK_MAX_J == 32
    assert int(define("MVG_TRACK_MAX_R")) == ops.TRACK_MAX_R and int(define("MVG_TRACK_MAX_B")) == ops.TRACK_MAX_B
    assert int(define("MVG_TRACK_STATE_WORDS")) == len(ops.TRACK_STATE) == 8 and ops.TRACK_STATE == TR.STATE


def test_cpu_tensors_raise_like_every_other_operator():
    from mvgformer_amd import tracking
    assert "PoseTracker" in tracking.__all__
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.linear_assignment(torch.zeros((1, 3, 3), dtype=torch.float64))
    buffers = ops.track_buffers(2, 4, 15, 8, "cpu")
    assert set(buffers) == {"id", "hits", "misses", "born", "score", "pose", "next_id", "state", "ids", "slots"}
    assert all(int((buffers[k] != -1).sum()) == 0 for k in ("id", "ids", "slots")) and buffers["born"].dtype == torch.int64
    assert tuple(buffers["pose"].shape) == (2, 4, 15, 3) and tuple(buffers["ids"].shape) == (2, 8)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.track_update(torch.zeros((2, 8, 15, 5)), None, buffers, 500.0, 10, 1)
    tracker = tracking.PoseTracker(batch=1, rows=8, device="cpu")
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        tracker.update(torch.zeros((1, 8, 15, 5)))
    assert tracker.tracks() == [[]] and tracker.state()["frames"] == 0
    for bad in (dict(T=65), dict(J=33)):
        with pytest.raises(_lib.MvgError):
            ops.track_buffers(**{**dict(B=1, T=4, J=15, R=8, device="cpu"), **bad})


def test_validate_parser_knows_device_track(capsys):
    from mvgformer_amd import validate
    with pytest.raises(SystemExit) as e:
        validate.main(["--cfg", "extract:configs/panoptic/knn5-lr4-q1024-g8.yaml", "--device-track", "1", "--device-nms", "0"])
    assert e.value.code == 2 and "--device-nms 1" in capsys.readouterr().err
    # accepted together with --device-nms 1: the run then stops where every CPU run of validate stops
    with pytest.raises(SystemExit) as e:
        validate.main(["--cfg", "extract:configs/panoptic/knn5-lr4-q1024-g8.yaml", "--device", "cpu", "--device-track", "1",
                       "--device-nms", "1"])
    assert e.value.code == "Not implemented on the CPU"
