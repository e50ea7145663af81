"""Seeded inputs for the bone-length estimator's tests (tests/test_track_bones_cpu.py, tests/test_track_bones_gpu.py) and the
synthetic table of tools/bench_st.py --track-lengths 1.

    study(seed, V, W)          persons with FIXED bones and a fresh pose per frame, seen by the ring cameras of golden/st_cases.py:
                               LS per frame, the estimator on the LS poses, one ST step under the estimated lengths
    sequence(J, R, W, seed)    per frame dets (2, R, J, 5) and count for the real tracker: persons leave and enter, so that slots
                               are freed and reopened, one frame carries a NaN and one an Inf coordinate
"""
import numpy as np

from tests import bones_ref, st_ref
from tests.golden.st_cases import ring_cameras

PANOPTIC15_PARENT = (-1, 0, 0, 0, 3, 4, 2, 6, 7, 0, 9, 10, 2, 12, 13)
H36M17_PARENT = (-1, 2, 0, 0, 3, 4, 1, 0, 7, 16, 11, 12, 8, 8, 13, 14, 8)
PARENTS = {15: PANOPTIC15_PARENT, 17: H36M17_PARENT}


def posed(rng, parent, bones, root):
    """a pose (J, 3) with the given bone lengths in random directions"""
    J = len(parent)
    X = np.zeros((J, 3))
    X[0] = root
    done = {0}
    while len(done) < J:
        for k in range(1, J):
            if k not in done and parent[k] in done:
                d = rng.normal(size=3)
                X[k] = X[parent[k]] + d / np.linalg.norm(d) * bones[k - 1]
                done.add(k)
    return X


def _lengths(X, parent):
    return np.stack([np.linalg.norm(X[..., k, :] - X[..., parent[k], :], axis=-1) for k in range(1, len(parent))], -1)


def study(seed, V, W=8, persons=4, noise=2.0, scored=4, parent=PANOPTIC15_PARENT):
    """W - 1 + scored frames; the last `scored` are solved under the median of the W frames up to and including their own.
    -> dict: bone residual against the TRUE lengths (mm, mean absolute) and mean joint error against the generating pose (mm) for
    the LS poses and for one ST step under the estimated lengths, uniform view weights, over the scored frames"""
    rng = np.random.default_rng(seed)
    J, F = len(parent), W - 1 + scored
    P = ring_cameras(V)
    bones = rng.uniform(150.0, 450.0, (persons, J - 1))
    truth = np.stack([np.stack([posed(rng, parent, bones[n], rng.normal(0, 800, 3) + [0, 0, 900]) for n in range(persons)])
                      for _ in range(F)])                                                      # (F, N, J, 3)
    h = np.concatenate([truth, np.ones((F, persons, J, 1))], -1)
    p = np.einsum("vij,fnkj->fnvki", P, h)
    ud = (p[..., :2] / p[..., 2:] + rng.normal(0, 1.0, (F, persons, V, J, 2)) * noise).astype(np.float32)
    Pm = np.broadcast_to(P.astype(np.float32), (F * persons, V, 3, 4))
    ls, status = st_ref.solve(ud.reshape(F * persons, V, J, 2), None, Pm, parent, None, "LS")
    assert not status.any()
    ls = ls.reshape(F, persons, J, 3)
    # the estimator on the LS poses: row n is person n, in slot n, from the first frame on
    buf = bones_ref.new_buffers(1, persons, J, persons, W)
    slots = np.arange(persons, dtype=np.int32)[None]
    est = []
    for f in range(F):
        dets = np.zeros((1, persons, J, 5), np.float32)
        dets[0, :, :, :3] = ls[f]
        dets[0, :, :, 3] = 1.0
        row_length, source = bones_ref.update(dets, None, slots, slots, parent, buf, min_frames=W)
        assert (source[0] == (0 if f >= W - 1 else 2)).all()
        est.append(row_length[0].copy())
    last = slice(F - scored, F)
    n = scored * persons
    st, status = st_ref.solve(ud[last].reshape(n, V, J, 2), None, Pm[:n], parent, np.stack(est[F - scored:]).reshape(n, J - 1), "ST", 1)
    assert not status.any()
    want = np.broadcast_to(bones, (scored, persons, J - 1)).reshape(n, J - 1)
    gen = truth[last].reshape(n, J, 3)
    out = {}
    for name, X in (("ls", ls[last].reshape(n, J, 3).astype(np.float64)), ("st", st.astype(np.float64))):
        out[name + "_bone_mm"] = float(np.abs(_lengths(X, parent) - want).mean())
        out[name + "_joint_mm"] = float(np.linalg.norm(X - gen, axis=-1).mean())
    return out


def sequence(J, R, W, seed=0, people=6):
    """2 W + 3 frames for B = 2 streams -> list of (dets (2, R, J, 5) fp32, count (2, 2) int32), R >= 8.  Every person is a rigid
    figure with 5 mm of noise per joint and frame that walks 30 mm per frame, 1.5 m from the next; who is present changes: person 0 and 1 stay, person 2 leaves for two frames
    (with max_misses = 1 its slot is freed, and reopened by whoever is born next) while person 3 enters; stream 1 shows the
    persons in another order, without person 1, and a person 4 who comes and goes every other frame.  With R > 64, stream 0
    also carries 70 far-away one-frame detections in its FIRST rows in every fourth frame: the persons' rows are then behind
    the first 64 detections and have no slot.  One tracked row has a NaN
    coordinate in frame 3 and an Inf coordinate in frame 5."""
    rng = np.random.default_rng(1000 * seed + 10 * J + W)
    parent = PARENTS[J]
    bones = rng.uniform(150.0, 450.0, (people, J - 1))
    start = np.array([[1500.0 * k, 300.0 * k, 900.0] for k in range(people)])
    shape = [posed(rng, parent, bones[k], np.zeros(3)) for k in range(people)]        # a rigid figure per person, plus 5 mm noise
    frames = []
    F = 2 * W + 3
    for f in range(F):
        present = {0, 1}
        if not 4 <= f < 6:
            present.add(2)
        if f >= 4:
            present.add(3)
        dets = np.zeros((2, R, J, 5), np.float32)
        dets[..., 3] = -1.0
        count = np.zeros((2, 2), np.int32)
        for b in range(2):
            who = sorted(present) if b == 0 else sorted((present - {1}) | ({4} if f % 2 else set()))[::-1]
            if b == 0 and f % 3 == 2:
                who = who[1:] + who[:1]                                   # the keep order reshuffles the rows
            n = 0
            if R > 64 and b == 0 and f and f % 4 == 0:                     # a crowd in front: the tracked persons fall behind row 64
                for c in range(70):
                    X = posed(rng, parent, bones[5], [40000.0 + 3000.0 * c, 50000.0 * (f + 1), 900.0])
                    dets[b, n, :, :3], dets[b, n, :, 3], dets[b, n, :, 4] = X, 1.0, 0.5
                    n += 1
            for k in who:
                X = shape[k] + start[k] + [30.0 * f, 0.0, 7000.0 * b] + rng.normal(scale=5.0, size=(J, 3))
                dets[b, n, :, :3], dets[b, n, :, 3], dets[b, n, :, 4] = X, 1.0, 0.9 - 0.1 * k
                if b == 0 and k == 0 and f == 3:
                    dets[b, n, 4, 1] = np.nan
                if b == 0 and k == 0 and f == 5:
                    dets[b, n, 6, 2] = np.inf
                n += 1
            count[b, 0] = n
        frames.append((dets, count))
    return frames
