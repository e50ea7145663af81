"""Seeded frame sequences for the tracker tests.  Coordinates are rounded to fp32 first; the same arrays go to the restatement
(tests/track_ref.py) and to the device.  A sequence is a dict:

    frames   list of (dets (B, R, J, 5) fp32, count (B, 2) int32 or None)
    persons  list, per frame, of a (B, R) int array: the person a row shows, -1 for a row that is no detection
    T, max_dist, max_misses, min_hits   the tracker's parameters
    exact    True when a cost sits on the gate by construction (the gate case)
"""
import numpy as np

J = 15


def skeleton(rng, joints=J):
    """joint offsets of one person around its centre, mm"""
    return rng.uniform(-300.0, 300.0, size=(joints, 3))


def frame(people, R, count=True, rows=None, joints=J):
    """people: list of (person, pose (J, 3), score) in row order (rows: their row indices, default 0, 1, ...) -> one batch element:
    (dets (R, J, 5) fp32 with the rows behind the detections zero with flag -1, count [k, 0], persons (R))"""
    dets = np.zeros((R, joints, 5), np.float32)
    dets[:, :, 3] = -1.0
    who = np.full((R,), -1, np.int64)
    rows = list(range(len(people))) if rows is None else rows
    for r, (person, pose, score) in zip(rows, people):
        dets[r, :, :3] = np.asarray(pose, np.float32)
        dets[r, :, 3] = 1.0
        dets[r, :, 4] = np.float32(score)
        who[r] = person
    return dets, (np.array([len(people), 0], np.int32) if count else None), who


def _stack(elements):
    dets = np.stack([e[0] for e in elements])
    count = None if elements[0][1] is None else np.stack([e[1] for e in elements])
    return (dets, count), np.stack([e[2] for e in elements])


def _sequence(frames_people, R, T=8, max_dist=500.0, max_misses=2, min_hits=1, count=True, rows=None, exact=False, joints=J):
    """frames_people: per frame a list (one entry per batch element) of people lists"""
    frames, persons = [], []
    for elements in frames_people:
        f, who = _stack([frame(p, R, count, rows and rows[len(frames)], joints) for p in elements])
        frames.append(f)
        persons.append(who)
    return dict(frames=frames, persons=persons, T=T, max_dist=max_dist, max_misses=max_misses, min_hits=min_hits, exact=exact)


def _walkers(rng, n, n_frames, spacing=1500.0, step=40.0, noise=5.0):
    """n persons on a line `spacing` apart, each drifting `step` mm per frame, with detection noise: poses[f][k] (J, 3)"""
    skel = [skeleton(rng) for _ in range(n)]
    centre = np.array([[spacing * k, 200.0 * k, 900.0] for k in range(n)])
    heading = rng.normal(size=(n, 3))
    heading /= np.linalg.norm(heading, axis=1, keepdims=True)
    return [[centre[k] + step * f * heading[k] + skel[k] + rng.normal(scale=noise, size=(J, 3)) for k in range(n)]
            for f in range(n_frames)]


def _by_score(rng, poses, present=None):
    """the people of one frame in descending random score (the NMS keep order reshuffles the rows every frame)"""
    who = [k for k in range(len(poses)) if present is None or k in present]
    scores = rng.uniform(0.2, 0.99, size=len(who))
    order = np.argsort(-scores)
    return [(who[i], poses[who[i]], scores[i]) for i in order]


def walk(seed=1, min_hits=1, R=8):
    rng = np.random.default_rng(seed)
    poses = _walkers(rng, 4, 12)
    return _sequence([[_by_score(rng, p)] for p in poses], R, min_hits=min_hits)


def cross():
    """two persons passing each other: in frame 1 the mean joint distances are about [[100, 110], [105, 300]]: the greedy nearest
    choice pairs track 0 with detection 0 (then 300 for the other pair, 400 in all), the optimum is (0, 1) and (1, 0), 215"""
    rng = np.random.default_rng(2)
    skel = [skeleton(rng)] * 2                # one skeleton: every track / detection pair is a rigid translation
    t0, t1, d0 = np.array([0.0, 0.0, 900.0]), np.array([205.0, 0.0, 900.0]), np.array([100.0, 0.0, 900.0])
    cos = (110.0 ** 2 + 205.0 ** 2 - 300.0 ** 2) / (2.0 * 110.0 * 205.0)
    d1 = np.array([110.0 * cos, 110.0 * np.sqrt(1.0 - cos * cos), 900.0])
    # the person of detection 0 is the one that was track 1
    f0 = [(0, t0 + skel[0], 0.9), (1, t1 + skel[1], 0.8)]
    f1 = [(1, d0 + skel[1], 0.9), (0, d1 + skel[0], 0.8)]
    return _sequence([[f0], [f1]], 4)


def occlusion(max_misses=2):
    """person 0 is absent for max_misses frames and keeps its id, person 1 for max_misses + 1 frames and gets a new one; person 2
    stays"""
    rng = np.random.default_rng(3)
    n_frames = max_misses + 3
    poses = _walkers(rng, 3, n_frames, step=10.0)
    present = [{0, 1, 2}] + [{2}] * max_misses + [{0, 2}, {0, 1, 2}]
    return _sequence([[_by_score(rng, p, s)] for p, s in zip(poses, present)], 4, max_misses=max_misses)


def overflow():
    rng = np.random.default_rng(4)
    poses = _walkers(rng, 6, 3)
    return _sequence([[_by_score(rng, p)] for p in poses], 8, T=4)


def gate(max_dist):
    """one person on integer coordinates, displaced by exactly 512 mm along x on every joint in frame 1: every joint distance and
    their mean are exactly 512.0 in fp64"""
    rng = np.random.default_rng(5)
    pose = np.round(np.array([100.0, -200.0, 900.0]) + skeleton(rng))
    moved = pose + np.array([512.0, 0.0, 0.0])
    return _sequence([[[(0, pose, 0.9)]], [[(0, moved, 0.9)]], [[(0, moved, 0.9)]]], 2, max_dist=max_dist, exact=True)


def nan_pose(max_misses=2):
    """person 1's detection carries a NaN coordinate in frame 2: it matches nothing, opens a track whose pose matches nothing
    later, and that track dies after max_misses frames; person 1's own track misses one frame and goes on"""
    rng = np.random.default_rng(6)
    poses = _walkers(rng, 2, 7, step=10.0)
    frames = []
    for f, p in enumerate(poses):
        people = _by_score(rng, p)
        if f == 2:
            people = [(k, np.where(np.arange(J * 3).reshape(J, 3) == 7, np.nan, pose) if k == 1 else pose, s) for k, pose, s in people]
        frames.append([people])
    return _sequence(frames, 4, max_misses=max_misses)


def no_count():
    """count = None: all R rows are looked at, rows with flag -1 lie between the detections"""
    rng = np.random.default_rng(7)
    poses = _walkers(rng, 3, 4)
    rows = [[1, 4, 6], [0, 4, 7], [2, 3, 6], [1, 4, 6]]
    return _sequence([[_by_score(rng, p)] for p in poses], 8, count=False, rows=rows)


def two_streams():
    """B = 2: element 0 follows three persons, element 1 one person and from frame 2 a second"""
    rng = np.random.default_rng(8)
    a, b = _walkers(rng, 3, 5), _walkers(rng, 2, 5)
    return _sequence([[_by_score(rng, a[f]), _by_score(rng, b[f], {0} if f < 2 else {0, 1})] for f in range(5)], 4)


def serving_shape():
    """R = 1024 with 3 detections: the serving buffer shape"""
    rng = np.random.default_rng(9)
    poses = _walkers(rng, 3, 3)
    return _sequence([[_by_score(rng, p)] for p in poses], 1024, T=32)


def crowd():
    """70 detections: the first 64 take part, 6 are dropped; 64 slots"""
    rng = np.random.default_rng(10)
    skel = [skeleton(rng) for _ in range(70)]
    centre = np.array([[2000.0 * (k % 10), 2000.0 * (k // 10), 900.0] for k in range(70)])
    frames = []
    for f in range(2):
        people = [(k, centre[k] + 30.0 * f + skel[k] + rng.normal(scale=5.0, size=(J, 3)), 0.99 - 0.01 * k) for k in range(70)]
        frames.append([people])
    return _sequence(frames, 80, T=64)


def float_sequences():
    """name -> sequence, every float-valued case of tests/test_track_gpu.py"""
    return dict(walk=walk(), cross=cross(), occlusion=occlusion(), overflow=overflow(), gate_on=gate(512.0),
                gate_off=gate(float(np.nextafter(512.0, 0.0))), nan_pose=nan_pose(), min_hits=walk(seed=11, min_hits=3),
                no_count=no_count(), two_streams=two_streams(), serving_shape=serving_shape(), crowd=crowd())


# ------------------------------------------------------------------------------------------------------- solver matrices
SOLVER_SIZES = ((1, 1), (5, 9), (64, 64), (64, 3), (0, 7), (7, 0))


def solver_matrices():
    """name -> (cost (6, 64, 64) fp64, n (6) int32, m (6) int32) with the live sizes SOLVER_SIZES"""
    rng = np.random.default_rng(12)
    n = np.array([s[0] for s in SOLVER_SIZES], np.int32)
    m = np.array([s[1] for s in SOLVER_SIZES], np.int32)
    B = len(SOLVER_SIZES)
    odd = rng.uniform(0.0, 100.0, size=(B, 64, 64))
    hit = rng.uniform(size=odd.shape)
    odd[hit < 0.05] = np.nan
    odd[(hit >= 0.05) & (hit < 0.10)] = np.inf
    odd[(hit >= 0.10) & (hit < 0.15)] = 1e300
    return dict(random=(rng.uniform(0.0, 1000.0, size=(B, 64, 64)), n, m),
                ties=(rng.integers(0, 4, size=(B, 64, 64)).astype(np.float64), n, m),
                equal=(np.full((B, 64, 64), 7.5), n, m),
                odd=(odd, n, m))
