"""Seeded scenes for the device NMS tests (tests/test_pose_nms_cpu.py, tests/test_pose_nms_gpu.py): inputs only, and the
restatement's result on them, computed once per process (tests/nms_ref.py)."""
import functools

import numpy as np

from tests import nms_ref
from tests.golden.eval_cases import _person

SCALES = (0.5, 1.0, 1.0, 1.6)       # about the centroid: poses of different extent have different limits -> `close` not symmetric
SIGMAS = (5.0, 40.0, 120.0)         # mm


def scene(N, seed, J=15, flagged=0.0):
    """(N, J, 5) fp32 rows [x, y, z, flag, score]: max(1, N // 6) persons, every candidate a random person scaled about its
    centroid plus Gaussian noise; distinct scores; a share `flagged` of the rows below the classification threshold (flag -1)."""
    rng = np.random.default_rng(seed)
    persons = [_person(rng, J) for _ in range(max(1, N // 6))]
    p = np.zeros((N, J, 5))
    for n in range(N):
        body = persons[int(rng.integers(len(persons)))]
        c = body.mean(0)
        p[n, :, :3] = c + (body - c) * rng.choice(SCALES) + rng.normal(0.0, rng.choice(SIGMAS), size=(J, 3))
    p[:, :, 4] = (rng.permutation(N) / N * 0.9 + 0.05)[:, None]
    p[:, :, 3] = np.where(rng.uniform(size=N) < flagged, -1.0, 0.0)[:, None]
    return p.astype(np.float32)


# name -> (N, seed, J, flagged share, kwargs of the operator)
GENERATED = {
    "n1": (1, 101, 15, 0.0, {}),
    "n63": (63, 163, 15, 0.0, {}),
    "n64": (64, 164, 15, 0.0, {}),
    "n65": (65, 165, 15, 0.0, {}),
    "n130": (130, 230, 15, 0.0, {}),
    "n130_flagged": (130, 231, 15, 0.4, {}),
    "n65_j14": (65, 166, 14, 0.0, {"num_nearby_joints_thr": None}),
    "n130_maxdets": (130, 230, 15, 0.0, {"max_dets": 7}),
    "n1024": (1024, 1124, 15, 0.0, {}),
    "n2048_sparse": (2048, 2148, 15, 0.9, {}),
}


def _tied(N, seed, levels):
    p = scene(N, seed)
    rng = np.random.default_rng(seed + 1)
    p[:, :, 4] = rng.choice(np.asarray(levels, dtype=np.float32), size=N)[:, None]
    return p


def degenerate():
    """name -> (pred fp32, kwargs): hand-made inputs at the edges of the contract"""
    out = {}
    # tied scores in a small scene whose outcome does not depend on the order in which tied rows are visited (every group of tied
    # rows is one pose repeated, so its members have the same row and column of `close`): the host functions, whose argsort
    # leaves that order open, must agree with the rule whatever sort numpy picks.  Rows 0 / 1 are the best scored pair.
    t = scene(12, 7)
    for src, dup in ((0, 1), (4, 5), (8, 9)):
        t[dup] = t[src]
    t[:2, :, 4] = np.float32(0.99)
    out["ties_small"] = (t, {})
    out["ties_large"] = (_tied(150, 8, (0.2, 0.4, 0.6, 0.8)), {})             # N > 16: the documented rule
    out["ties_large_maxdets"] = (_tied(150, 9, (0.25, 0.75)), {"max_dets": 5})
    z = scene(9, 11)
    z[4, :, :3] = np.float32([9000.0, 9000.0, 500.0])                          # zero extent, far from everybody: limit 0, 0 < 0 false
    out["zero_extent"] = (z, {})
    n = scene(9, 12)
    n[2, :, 0] += np.float32(20000.0)                                          # in nobody's neighbourhood
    n[2, 5, 1] = np.nan
    n[2, :, 4] = np.float32(0.99)                                              # visited first, before anything can suppress it
    out["nan_coordinate"] = (n, {})
    a = scene(20, 13)
    a[:, :, 3] = -1.0
    out["all_flagged"] = (a, {})
    o = scene(20, 14)
    o[:, :, 3] = -1.0
    o[13, :, 3] = 0.0
    out["one_candidate"] = (o, {})
    return out


@functools.lru_cache(maxsize=None)
def generated(name):
    """-> (pred, kwargs, (keep, count, dets, stats)); shared between tests, never modified"""
    N, seed, J, flagged, kw = GENERATED[name]
    pred = scene(N, seed, J, flagged)
    pred.setflags(write=False)
    return pred, kw, nms_ref.pose_nms(pred, **kw)


@functools.lru_cache(maxsize=None)
def degenerate_reference(name):
    pred, kw = degenerate()[name]
    pred.setflags(write=False)
    return pred, kw, nms_ref.pose_nms(pred, **kw)
