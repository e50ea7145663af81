"""Numpy restatement of the one-to-one ground-truth matcher (mvg_hungarian_match, include/mvg_decoder.h), the yardstick of
tests/test_hungarian_cpu.py and tests/test_hungarian_gpu.py.  Pinned to the reference's own pairs (lib/models/matcher.py with
scipy's linear_sum_assignment) in tests/golden/hungarian.npz, to scipy on the restated costs, and to brute force.

  pose_costs()    the fp32 pose cost, bit for bit what the matchers' shared device function computes: the ground truth through
                  the norm round trip of tests/criterion_ref.norm_round_trip in fp32 with n * size + center as ONE fused
                  multiply-add (csrc/match_dev.h says why), then 0.01 * the L1 sum over the 3J coordinates added one coordinate
                  after the other in fp32, joint by joint.  criterion_ref.costs rounds n * size on its own and sums with
                  torch.cdist, whose vectorised order differs: last-bit differences; the CPU test holds the two together.
  class_term()    matcher.py:151-162 with every target in class 1, in fp64
  cost_matrix()   C (P, Gmax, NQ) fp64 as the header states it, NaN and > 1e15 taken as 1e15
  solve()         the solver, written from the header text of mvg_linear_assignment for the rectangular problem; returns the duals
  hungarian_match()  everything mvg_hungarian_match writes, for all P = Lm * B problems
"""
import numpy as np

LAP_BIG = 1e15


def fma_f32(a, b, c):
    """a * b + c of float32 arrays with ONE rounding to float32.  The product of two float32 is exact in float64; TwoSum gives the
    exact error of the float64 addition, which decides the one case where rounding twice differs from rounding once: the float64
    sum lying exactly half way between two float32 neighbours."""
    f32, f64 = np.float32, np.float64
    p, c = a.astype(f64) * b.astype(f64), np.asarray(c, f32).astype(f64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)                               # exact: (p + c) - s
    t = s.astype(f32)
    up, dn = np.nextafter(t, f32(np.inf)).astype(f64), np.nextafter(t, f32(-np.inf)).astype(f64)
    t64 = t.astype(f64)
    half_up, half_dn = (s - t64) == (up - t64) / 2, (s - t64) == (dn - t64) / 2
    lo = np.where(half_up, t64, np.where(half_dn, dn, t64))     # the float32 neighbours around a half-way sum
    hi = np.where(half_up, up, np.where(half_dn, t64, t64))
    mid = (half_up | half_dn) & (e != 0) & np.isfinite(s)
    return np.where(mid, np.where(e > 0, hi, lo), t64).astype(f32)


def norm_round_trip_f32(x, size, center):
    """absolute -> norm -> absolute as csrc/match_dev.h rounds it: every operation in float32, n * size + center fused"""
    x, size, center = np.asarray(x, np.float32), np.asarray(size, np.float32), np.asarray(center, np.float32)
    half = size / np.float32(2.0)
    n = ((x - center) + half) / size
    return fma_f32(n, np.broadcast_to(size, n.shape), np.broadcast_to(center, n.shape)) - half


def pose_costs(poses, joints_3d, size, center, joint_map=None, num_joints=None):
    """poses (B, NQ*Jp, 3), joints_3d (B, Gmax, J, 3) -> (B, Gmax, NQ) float32"""
    poses, joints_3d = np.asarray(poses, np.float32), np.asarray(joints_3d, np.float32)
    B, Gmax, J = joints_3d.shape[:3]
    Jp = J if joint_map is None else int(num_joints)
    jm = list(range(J)) if joint_map is None else [int(v) for v in joint_map]
    x = poses.reshape(B, -1, Jp, 3)
    gt = norm_round_trip_f32(joints_3d, size, center)
    assert gt.dtype == np.float32
    s = np.zeros((B, Gmax, x.shape[1]), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(J):
            for c in range(3):
                s = s + np.abs(x[:, None, :, jm[j], c] - gt[:, :, None, j, c])
        s = s * np.float32(0.01)
        return np.where(s < np.float32(np.inf), s, np.float32(np.inf)).astype(np.float32)     # NaN / inf poses sort last


def class_term(logits):
    """logits (..., NQ, 2) -> (..., NQ) float64"""
    x = np.asarray(logits, np.float32)[..., 1].astype(np.float64)
    p = 1.0 / (1.0 + np.exp(-x))
    om = 1.0 - p
    pos = (0.25 * (om * om)) * (-np.log(p + 1e-8))
    neg = (0.75 * (p * p)) * (-np.log(om + 1e-8))
    return pos - neg


def cost_matrix(poses, joints_3d, size, center, logits=None, method="hungarian", cost_class=1.0, cost_pose=1.0, joint_map=None,
                num_joints=None):
    """poses (Lm, B, NQ*Jp, 3), logits (Lm, B, NQ, 2) or None -> C (Lm * B, Gmax, NQ) float64, problem p = l * B + b"""
    poses = np.asarray(poses, np.float32)
    Lm, B = poses.shape[:2]
    pose = np.stack([pose_costs(poses[l], joints_3d, size, center, joint_map, num_joints) for l in range(Lm)]).astype(np.float64)
    pose = pose.reshape((Lm * B,) + pose.shape[2:])
    with np.errstate(invalid="ignore", over="ignore"):
        if method == "hungarian-dis":
            C = pose
        elif method == "hungarian":
            NQ = pose.shape[-1]
            cls = class_term(np.ones((Lm, B, NQ, 2), np.float32) if logits is None else logits).reshape(Lm * B, 1, NQ)
            C = np.float64(np.float32(cost_pose)) * pose + np.float64(np.float32(cost_class)) * cls
        else:
            raise ValueError(method)
        return np.where(C <= LAP_BIG, C, LAP_BIG)              # NaN or above


def solve(C):
    """C (G, NQ) float64 with G <= NQ -> (col_of_row (G,), u (G,), v (NQ,)).  Shortest augmenting paths with potentials from 0, rows
    inserted in order; the lowest column among equal minima, a NaN minimum ordered as +inf; a search of row i is a counted loop of
    at most i + 1 steps."""
    G, NQ = C.shape
    inf = np.inf
    u, v = np.zeros(G), np.zeros(NQ)
    p = np.full(NQ, -1, np.int64)                               # row of every column
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(G):
            minv = np.full(NQ, inf)
            way = np.full(NQ, -1, np.int64)                      # -1: the virtual column, whose row is i
            used = np.zeros(NQ, bool)
            j0, i0, found = -1, i, False
            for _ in range(i + 1):
                if j0 >= 0:
                    used[j0] = True                              # 1.
                cand = ~used
                cur = (C[i0] - u[i0]) - v                        # 2.
                better = cand & (cur < minv)
                minv[better] = cur[better]
                way[better] = j0
                key = np.where(cand & ~np.isnan(minv), minv, inf)                  # 3.
                holders = np.nonzero(cand & (key == key[cand].min()))[0]
                j1 = int(holders[0])
                delta = minv[j1]
                u[p[used]] += delta                              # 4.: a used column has a row, every row at most one column
                u[i] += delta
                v[used] -= delta
                minv[cand] -= delta
                j0 = j1
                if p[j0] < 0:
                    found = True
                    break
                i0 = int(p[j0])
            assert found
            for _ in range(i + 1):                               # flip the path back to the virtual column
                j1 = int(way[j0])
                p[j0] = i if j1 < 0 else p[j1]
                j0 = j1
                if j0 < 0:
                    break
    col = np.full(G, -1, np.int64)
    col[p[p >= 0]] = np.nonzero(p >= 0)[0]
    return col, u, v


def hungarian_match(poses, joints_3d, num_person, size, center, logits=None, method="hungarian", cost_class=1.0, cost_pose=1.0,
                    joint_map=None, num_joints=None):
    """numpy inputs shaped like ops.hungarian_match's -> dict of pair_query, pair_gt (P... , Gmax) int32, pair_count int32, matched
    uint8, u (…, Gmax), v (…, NQ) float64 and C (…, Gmax, NQ); a leading Lm is kept."""
    poses = np.asarray(poses, np.float32)
    lead = poses.ndim == 4
    if not lead:
        poses = poses[None]
        logits = None if logits is None else np.asarray(logits)[None]
    Lm, B = poses.shape[:2]
    C = cost_matrix(poses, joints_3d, size, center, logits, method, cost_class, cost_pose, joint_map, num_joints)
    P, Gmax, NQ = C.shape
    out = dict(pair_query=np.full((P, Gmax), -1, np.int32), pair_gt=np.full((P, Gmax), -1, np.int32), pair_count=np.zeros(P, np.int32),
               matched=np.zeros((P, NQ), np.uint8), u=np.zeros((P, Gmax)), v=np.zeros((P, NQ)), C=C)
    for pi in range(P):
        G = int(min(max(int(np.asarray(num_person)[pi % B]), 0), Gmax))
        col, u, v = solve(C[pi, :G])
        order = np.argsort(col, kind="stable")
        out["pair_query"][pi, :G] = col[order]
        out["pair_gt"][pi, :G] = order
        out["pair_count"][pi] = G
        out["matched"][pi, col] = 1
        out["u"][pi, :G] = u
        out["v"][pi] = v
    head = (Lm, B) if lead else (B,)
    return {k: a.reshape(head + a.shape[1:]) for k, a in out.items()}


def check_certificate(C, G, pair_query, pair_gt, u, v, what=""):
    """the dual certificate of optimality on one problem: feasible everywhere, tight on the pairs, v = 0 off them.
    tol = 1e-9 * max|C|: the rounding of at most G (G + 1) / 2 fp64 updates is orders of magnitude below it."""
    C = np.asarray(C)[:G]
    tol = 1e-9 * float(np.abs(C).max()) if C.size else 0.0
    slack = C - (np.asarray(u)[:G, None] + np.asarray(v)[None, :])
    assert slack.size == 0 or slack.min() >= -tol, (what, float(slack.min()), tol)
    q, g = np.asarray(pair_query)[:G], np.asarray(pair_gt)[:G]
    assert np.all(np.abs(slack[g, q]) <= tol), (what, float(np.abs(slack[g, q]).max()), tol)
    free = np.ones(C.shape[1], bool)
    free[q] = False
    assert np.all(np.asarray(v)[free] == 0.0), what
    assert np.all(np.asarray(u)[G:] == 0.0), what
