"""Seeded synthetic scenes for the structural-triangulation tests, shared by make_golden_st.py and the tests: a ring of V cameras
looking at the origin, persons as random trees with bones of 150-450 mm, their projections with optional pixel noise.  Everything
that is handed to a solver is rounded to fp32 first."""
import numpy as np


def ring_cameras(V):
    """(V, 3, 4) fp64 projection matrices K [R | -R c], cameras on a ring of 4 m radius at 1.5 m height"""
    Ps = []
    for v in range(V):
        a = 2 * np.pi * v / V + 0.3
        c = np.array([4000 * np.cos(a), 4000 * np.sin(a), 1500.0])
        z = -c / np.linalg.norm(c)
        x = np.cross(z, [0, 0, 1.0])
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        R = np.stack([x, y, z])
        K = np.array([[1400, 0, 960], [0, 1400, 540], [0, 0, 1.0]])
        Ps.append(K @ np.concatenate([R, -(R @ c)[:, None]], 1))
    return np.stack(Ps)


def random_pose(rng, parent):
    J = len(parent)
    X = np.zeros((J, 3))
    X[0] = rng.normal(0, 800, 3) + [0, 0, 900]
    done = {0}
    while len(done) < J:
        for k in range(1, J):
            if k not in done and parent[k] in done:
                d = rng.normal(size=3)
                d /= np.linalg.norm(d)
                X[k] = X[parent[k]] + d * rng.uniform(150, 450)
                done.add(k)
    return X


def scene(seed, V, parent, persons=4, noise=0.0):
    """-> dict of ud (N, V, J, 2), conf (N, V, J), Pm (V, 3, 4), bone_len (N, J-1) fp32 and truth (N, J, 3) fp64.  conf are random
    weights that sum to 1 over the views; bone_len are the TRUE lengths (of the fp64 pose, rounded to fp32)."""
    rng = np.random.default_rng(seed)
    J = len(parent)
    P = ring_cameras(V)
    truth = np.stack([random_pose(rng, parent) for _ in range(persons)])
    h = np.concatenate([truth, np.ones((persons, J, 1))], -1)
    p = np.einsum("vij,nkj->nvki", P, h)
    ud = p[..., :2] / p[..., 2:] + rng.normal(0, 1.0, (persons, V, J, 2)) * noise
    conf = rng.uniform(0.5, 1.5, (persons, V, J))
    conf /= conf.sum(1, keepdims=True)
    bl = np.stack([np.linalg.norm(truth[:, k] - truth[:, parent[k]], axis=-1) for k in range(1, J)], 1)
    return dict(ud=ud.astype(np.float32), conf=conf.astype(np.float32), Pm=P.astype(np.float32), bone_len=bl.astype(np.float32),
                truth=truth)


def bone_residual(X, parent, bone_len):
    """mean absolute difference between the bone lengths of X (..., J, 3) and bone_len (..., J-1), fp64"""
    X = np.asarray(X, np.float64)
    J = len(parent)
    got = np.stack([np.linalg.norm(X[..., k, :] - X[..., parent[k], :], axis=-1) for k in range(1, J)], -1)
    return float(np.abs(got - np.asarray(bone_len, np.float64)).mean())
