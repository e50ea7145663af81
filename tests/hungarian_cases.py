"""Seeded inputs of the one-to-one matcher's tests (tests/test_hungarian_cpu.py, tests/test_hungarian_gpu.py) and of the fixture
tests/golden/hungarian.npz: the maker and the tests build them here, so the fixture stores only the pairs the reference chose.

A case = Lm sets of query poses and logits, ground truth and person counts.  Coordinates and logits are continuous random numbers
(the reference rounds its cost matrix in fp32, the restatement and the kernel in fp64: with continuous costs the optimum is
separated by far more than fp32 rounding).  A quarter of the queries start near a person, the rest anywhere in the space.
`contend`: every person stands within a few mm of person 0 and only three queries are near them, so every person's cheapest
queries are the same three and every insertion re-routes earlier rows.  TIE_CASES are hand-written integer-coordinate problems in
'hungarian-dis' whose equal costs are decided by the lowest-column rule; their expected pairs are written out in the test."""
import zlib

import numpy as np

SPACE_SIZE = (8000.0, 8000.0, 2000.0)
SPACE_CENTER = (0.0, -500.0, 800.0)
SHELF_MAP = [14, 13, 12, 6, 7, 8, 11, 10, 9, 3, 4, 5, 0, 1]       # configs/shelf_campus/*.yaml: 14 of the 15 joints

_D = dict(Lm=1, B=1, J=15, Jp=None, joint_map=None, method="hungarian", cost_class=2.0, cost_pose=5.0, contend=False, logit_scale=2.0)


def _case(**kw):
    return {**_D, **kw}


# the shapes at which the kernel takes another path: one column; square; a partial wavefront; one column past the workgroup
# width (a second slot per lane); the training shape (costs in LDS, 4 slots); 4096 x 64 (costs in the workspace, 16 slots, the
# longest search)
CASES = {
    "one":       _case(NQ=1, Gmax=1, J=1, num_person=[1], seed=101),
    "square7":   _case(NQ=7, Gmax=7, num_person=[7], seed=102),
    "nq70":      _case(NQ=70, Gmax=10, num_person=[10], seed=103),
    "nq70_g3":   _case(NQ=70, Gmax=10, num_person=[3], seed=104),
    "nq257":     _case(NQ=257, Gmax=10, num_person=[9], seed=105),
    "train":     _case(NQ=1024, Gmax=10, B=2, num_person=[10, 5], seed=106),
    "big":       _case(NQ=4096, Gmax=64, num_person=[64], seed=107),
    "dis":       _case(NQ=70, Gmax=10, B=2, num_person=[10, 4], method="hungarian-dis", seed=108),
    "counts":    _case(NQ=70, Gmax=6, B=3, num_person=[0, 6, 3], seed=109),
    "clamp":     _case(NQ=70, Gmax=6, B=2, num_person=[9, 1000], seed=110),
    "contend10": _case(NQ=257, Gmax=10, num_person=[10], contend=True, seed=111),
    "contend64": _case(NQ=1025, Gmax=64, num_person=[64], contend=True, seed=112),
    "logit40":   _case(NQ=70, Gmax=10, num_person=[10], logit_scale=40.0, seed=113),
    "shelf":     _case(NQ=70, Gmax=10, B=2, J=14, Jp=15, joint_map=SHELF_MAP, num_person=[10, 3], seed=114),
    "lm4":       _case(NQ=257, Gmax=10, B=2, Lm=4, num_person=[10, 6], seed=115),
}
# the cases the reference's matcher runs for the fixture: no empty batch element (matcher.py:141-143 raises on it), no count above
# Gmax, no joint map (the reference's callers gather before the matcher)
GOLDEN = ("one", "square7", "nq70", "nq70_g3", "nq257", "train", "dis", "contend10", "logit40", "lm4")


def make_inputs(name):
    """dict: poses (Lm, B, NQ*Jp, 3) float32, logits (Lm, B, NQ, 2) float32, joints_3d (B, Gmax, J, 3) float32, num_person (B,) int64"""
    c = name if isinstance(name, dict) else CASES[name]
    rs = np.random.RandomState(c["seed"])
    Lm, B, NQ, Gmax, J = c["Lm"], c["B"], c["NQ"], c["Gmax"], c["J"]
    Jp = J if c["Jp"] is None else c["Jp"]
    jm = list(range(J)) if c["joint_map"] is None else c["joint_map"]
    size, cen = np.array(SPACE_SIZE), np.array(SPACE_CENTER)
    spread = np.array([180.0, 180.0, 450.0])
    gt = np.zeros((B, Gmax, J, 3))
    for b in range(B):
        for g in range(Gmax):
            if c["contend"] and g > 0:
                gt[b, g] = gt[b, 0] + rs.standard_normal((J, 3)) * 4.0
            else:
                gt[b, g] = cen + (rs.rand(3) - 0.5) * size * np.array([0.7, 0.7, 0.2]) + rs.standard_normal((J, 3)) * spread
    poses = cen + (rs.rand(Lm, B, NQ, 1, 3) - 0.5) * size + rs.standard_normal((Lm, B, NQ, Jp, 3)) * spread
    for l in range(Lm):
        for b in range(B):
            near = range(min(3, NQ)) if c["contend"] else range(0, NQ, 4)
            for q in near:
                g = 0 if c["contend"] else (q // 4) % Gmax
                poses[l, b, q][jm] = gt[b, g] + rs.standard_normal(3) * 150.0 + rs.standard_normal((J, 3)) * 50.0
    logits = rs.standard_normal((Lm, B, NQ, 2)) * c["logit_scale"]
    return dict(poses=poses.reshape(Lm, B, NQ * Jp, 3).astype(np.float32), logits=logits.astype(np.float32),
                joints_3d=gt.astype(np.float32), num_person=np.array(c["num_person"], np.int64))


def checksum(inputs):
    """of the arrays of make_inputs: the fixture stores it, the tests check that they build what the maker built"""
    crc = 0
    for k in sorted(inputs):
        crc = zlib.crc32(np.ascontiguousarray(inputs[k]).tobytes(), crc)
    return np.int64(crc)


def match_kwargs(name):
    """the keyword arguments of ops.hungarian_match / hungarian_ref.hungarian_match for a case"""
    c = name if isinstance(name, dict) else CASES[name]
    return dict(method=c["method"], cost_class=c["cost_class"], cost_pose=c["cost_pose"], joint_map=c["joint_map"],
                num_joints=c["Jp"])


def _points(rows):
    """one joint per pose: rows of (x, y, z) -> (1, 1, n, 3) float32"""
    return np.array(rows, np.float32).reshape(1, 1, -1, 3)


# 'hungarian-dis' with J = 1 inside a 1024 mm cube centred at the origin, whose norm round trip is exact for integer
# coordinates: cost = 0.01 * (|dx| + |dy| + |dz|).  name -> queries, persons, expected (query, person) pairs in ascending query order.
TIE_SPACE = ((1024.0, 1024.0, 1024.0), (0.0, 0.0, 0.0))
TIE_CASES = {
    # all costs equal: row 0 takes the lowest column, row 1 the lowest unused one
    "all_equal": dict(queries=[(100, 0, 0), (0, 100, 0), (0, 0, 100), (-100, 0, 0)], persons=[(0, 0, 0), (0, 0, 0)],
                      pairs=[(0, 0), (1, 1)]),
    # both persons are nearest to query 1 at equal cost; the second best of each is query 0 or 2 at equal cost: row 0 takes
    # query 1, row 1 then finds delta equal for "take query 0" and "take query 2" and the lowest column wins
    "shared_best": dict(queries=[(200, 0, 0), (0, 0, 0), (-200, 0, 0), (0, 500, 0)], persons=[(0, 0, 0), (0, 0, 0)],
                        pairs=[(0, 1), (1, 0)]),
    # person 1 can only be served cheaply by query 2, which row 0 holds after a tie between queries 2 and 3 for itself: row 0
    # moves to query 3 (equal cost), not to the lower but dearer query 0
    "reroute": dict(queries=[(400, 0, 0), (0, 400, 400), (100, 0, 0), (-100, 0, 0)], persons=[(0, 0, 0), (100, 0, 0)],
                    pairs=[(2, 1), (3, 0)]),
    # three persons on a line of queries: every row has its own zero-cost query between equal second-best costs; no row moves
    "line": dict(queries=[(0, 0, 0), (50, 0, 0), (100, 0, 0), (150, 0, 0), (200, 0, 0)], persons=[(50, 0, 0), (100, 0, 0), (150, 0, 0)],
                 pairs=[(1, 0), (2, 1), (3, 2)]),
}


def tie_inputs(name):
    t = TIE_CASES[name]
    G = len(t["persons"])
    return dict(poses=_points(t["queries"])[0], joints_3d=np.array(t["persons"], np.float32).reshape(1, G, 1, 3),
                num_person=np.array([G], np.int64))
