"""Seeded sequences with ground truth for the tracking scores (mvg_track_eval), built with the helpers of tests/track_cases.py.
The ground truth of a frame is every person's NOISE-FREE pose, present in the detections or not; coordinates are rounded to fp32
first and the same arrays go to the restatement (tests/trackeval_ref.py) and to the device.  A case is a dict:

    frames      list of (dets (B, R, J, 5) fp32, count (B, 2) int32 or None)
    truth       list, per frame, of (joints_3d (B, G, J, 3) fp32, joints_3d_vis (B, G, J) fp32, num_person (B) int32,
                person_id (B, G) int32 or None)
    T, max_dist, max_misses, min_hits, motion     the tracker's parameters
    dist_thr, P, K                                 the scorer's
    clear_last  frames in front of which last_track is reset to -1 (the kept-correspondence case)
"""
import numpy as np

from tests import track_cases as TC

J = TC.J
R = 8                                  # rows of dets in every case but the full size


def _truth(streams, G, vis=None, num=None, person_id=None):
    """streams: per stream the list of its persons' (J, 3) poses -> one frame's ground truth"""
    B = len(streams)
    j3d = np.zeros((B, G, J, 3), np.float32)
    v = np.zeros((B, G, J), np.float32)
    for b, poses in enumerate(streams):
        for g, pose in enumerate(poses):
            j3d[b, g] = np.asarray(pose, np.float32)
            v[b, g] = 1.0
    if vis is not None:
        v = np.asarray(vis, np.float32)
    n = np.array([len(p) for p in streams] if num is None else num, np.int32)
    return j3d, v, n, (None if person_id is None else np.asarray(person_id, np.int32))


def _case(frames_people, truth, R, T=8, max_dist=500.0, max_misses=2, min_hits=1, motion=False, dist_thr=500.0, P=None, K=16,
          count=True, rows=None, clear_last=()):
    seq = TC._sequence(frames_people, R, T=T, max_dist=max_dist, max_misses=max_misses, min_hits=min_hits, count=count, rows=rows)
    G = truth[0][0].shape[1]
    return dict(frames=seq["frames"], truth=truth, T=T, max_dist=max_dist, max_misses=max_misses, min_hits=min_hits, motion=motion,
                dist_thr=dist_thr, P=G if P is None else P, K=K, clear_last=frozenset(clear_last))


def _walkers(seed, n, n_frames, step=40.0, noise=5.0):
    """(rng, noisy poses[f][k], noise-free poses[f][k]): two generators on one seed draw the same skeletons and headings"""
    rng = np.random.default_rng(seed)
    noisy = TC._walkers(rng, n, n_frames, step=step, noise=noise)
    clean = TC._walkers(np.random.default_rng(seed), n, n_frames, step=step, noise=0.0)
    return rng, noisy, clean


def walkers(seed=21, n=3, n_frames=8, present=None, ghost=(), step=40.0, G=4, **params):
    """n walkers; present[f]: the persons detected in frame f (default all); ghost: the frames with a spurious detection 9 m away"""
    rng, noisy, clean = _walkers(seed, n, n_frames, step=step)
    spurious = clean[0][0] + np.array([0.0, 9000.0, 0.0])
    frames = []
    for f in range(n_frames):
        people = TC._by_score(rng, noisy[f], None if present is None else present[f])
        if f in ghost:
            people = people + [(99, spurious, 0.1)]
        frames.append([people])
    return _case(frames, [_truth([clean[f]], G) for f in range(n_frames)], R, **params)


def perfect():
    return walkers()


def occlusion():
    """person 0 is undetected for max_misses = 2 frames and keeps its id, person 1 for 3 frames and comes back under a new one"""
    present = [{0, 1, 2}, {2}, {2}, {0, 2}] + [{0, 1, 2}] * 4
    return walkers(seed=22, present=present, step=10.0)


def min_hits():
    return walkers(seed=23, min_hits=3)


def ghost():
    return walkers(seed=24, ghost=(2, 3, 4))


def small_table():
    """the occlusion sequence with K = 2 columns: the ids 2 and 3 do not fit"""
    present = [{0, 1, 2}, {2}, {2}, {0, 2}] + [{0, 1, 2}] * 4
    return walkers(seed=22, present=present, step=10.0, K=2)


def moving(motion):
    """walkers at 60 mm a frame with the occlusion pattern, for the motion model (row_pose) against the plain tracker"""
    present = [{0, 1, 2}] * 3 + [{2}, {2}, {0, 2}] + [{0, 1, 2}] * 4
    return walkers(seed=25, n_frames=10, present=present, step=60.0, motion=motion)


def _rigid(points, skel):
    return [np.array([x, y, 900.0]) + skel for x, y in points]


def kept_pairs(clear=False):
    """two persons at (0, 0) and (300, 0).  Frame 0: detections at (0, -200) and (300, 200), ids 0 and 1.  Frame 1: (200, -100) and
    (100, 100): the tracker keeps the ids (224 + 224 against 316 + 316), against the ground truth the swapped pairing is the
    cheaper one (141 + 141 against 224 + 224), and every pair is within 500: step 5 keeps the old pairs.  With clear the scorer
    forgets last_track in front of frame 1 and takes the swap."""
    skel = np.round(TC.skeleton(np.random.default_rng(26)))
    gt = _rigid([(0.0, 0.0), (300.0, 0.0)], skel)
    d0 = _rigid([(0.0, -200.0), (300.0, 200.0)], skel)
    d1 = _rigid([(200.0, -100.0), (100.0, 100.0)], skel)
    frames = [[[(0, d0[0], 0.9), (1, d0[1], 0.8)]], [[(0, d1[0], 0.9), (1, d1[1], 0.8)]]]
    return _case(frames, [_truth([gt], 2)] * 2, R, clear_last=(1,) if clear else ())


def contested():
    """persons A (slot 0) at (0, 0) and B at (300, 0).  Frame 0: one detection at (0, 0), id 0, is A's.  Frame 1: A has no visible
    joint, the detection at (150, 0) is B's: both last_track name id 0.  Frame 2: both visible, detections at (160, 0) (id 0) and
    (330, 0) (id 1): A, the lower slot, keeps id 0, B goes to the assignment and takes id 1, one switch."""
    skel = np.round(TC.skeleton(np.random.default_rng(27)))
    gt = _rigid([(0.0, 0.0), (300.0, 0.0)], skel)
    d = _rigid([(0.0, 0.0), (150.0, 0.0), (160.0, 0.0), (330.0, 0.0)], skel)
    frames = [[[(0, d[0], 0.9)]], [[(0, d[1], 0.9)]], [[(0, d[2], 0.9), (1, d[3], 0.8)]]]
    hidden = np.ones((1, 2, J), np.float32)
    hidden[0, 0] = 0.0
    return _case(frames, [_truth([gt], 2), _truth([gt], 2, vis=hidden), _truth([gt], 2)], R)


def threshold(dist_thr):
    """one person on integer coordinates, the detection displaced by exactly 512 mm along x on every joint (track_cases.gate): the
    distance is exactly 512.0"""
    pose = np.round(np.array([100.0, -200.0, 900.0]) + TC.skeleton(np.random.default_rng(5)))
    moved = pose + np.array([512.0, 0.0, 0.0])
    return _case([[[(0, moved, 0.9)]]], [_truth([[pose]], 1)], R, max_dist=600.0, dist_thr=dist_thr)


VISIBLE = (0, 3, 4)


def visibility():
    """person 0 has joints 0, 3, 4 visible and its detection is displaced by 8 (j + 1) mm along x on joint j: the mean is
    (8 + 32 + 40) / 3; person 1 has no visible joint and is no person: its detection is a false positive"""
    rng = np.random.default_rng(28)
    pose = [np.round(np.array([1500.0 * k, 0.0, 900.0]) + TC.skeleton(rng)) for k in range(2)]
    moved = pose[0] + np.stack([np.array([8.0 * (j + 1), 0.0, 0.0]) for j in range(J)])
    vis = np.zeros((1, 2, J), np.float32)
    vis[0, 0, list(VISIBLE)] = 1.0
    return _case([[[(0, moved, 0.9), (1, pose[1], 0.8)]]], [_truth([pose], 2, vis=vis)], R)


def nan_detection():
    """frame 2: person 1's detection carries a NaN coordinate: a false positive and a miss, and dist_sum stays a number"""
    rng, noisy, clean = _walkers(29, 2, 4, step=10.0)
    frames = []
    for f in range(4):
        people = TC._by_score(rng, noisy[f])
        if f == 2:
            people = [(k, np.where(np.arange(J * 3).reshape(J, 3) == 7, np.nan, pose) if k == 1 else pose, s) for k, pose, s in people]
        frames.append([people])
    return _case(frames, [_truth([clean[f]], 2) for f in range(4)], R)


def annotation():
    """frame 1 has no annotation (num_person = -1: skipped), frame 2 is annotated empty (num_person = 0: all false positives)"""
    rng, noisy, clean = _walkers(30, 2, 4)
    frames = [[TC._by_score(rng, noisy[f])] for f in range(4)]
    num = [None, [-1], [0], None]
    return _case(frames, [_truth([clean[f]], 3, num=num[f]) for f in range(4)], R)


def identities():
    """person_id: slots 0, 1, 2 are the identities 2, 0, 7 -- 7 is out of range (P = 4) -- and from frame 2 on 2, 2, 1: a repeat"""
    rng, noisy, clean = _walkers(31, 3, 4)
    frames = [[TC._by_score(rng, noisy[f])] for f in range(4)]
    pid = [[[2, 0, 7, -1]], [[2, 0, 7, -1]], [[2, 2, 1, -1]], [[2, 2, 1, -1]]]
    return _case(frames, [_truth([clean[f]], 4, person_id=pid[f]) for f in range(4)], R, P=4)


def no_count():
    """count = None: all R rows are looked at, rows with flag -1 lie between the detections"""
    rng, noisy, clean = _walkers(32, 3, 4)
    rows = [[1, 4, 6], [0, 4, 7], [2, 3, 6], [1, 4, 6]]
    frames = [[TC._by_score(rng, noisy[f])] for f in range(4)]
    return _case(frames, [_truth([clean[f]], 3) for f in range(4)], R, count=False, rows=rows)


def two_streams():
    """B = 2, uneven: stream 0 follows three persons; stream 1 has two, the second undetected in the first two frames, and no
    annotation in frame 3"""
    rng, a_noisy, a_clean = _walkers(33, 3, 5)
    _, b_noisy, b_clean = _walkers(34, 2, 5)
    frames = [[TC._by_score(rng, a_noisy[f]), TC._by_score(rng, b_noisy[f], {0} if f < 2 else {0, 1})] for f in range(5)]
    truth = [_truth([a_clean[f], b_clean[f]], 4, num=[3, -1] if f == 3 else None) for f in range(5)]
    return _case(frames, truth, R)


def crowd():
    """the full size: G = P = 64 persons and 64 hypotheses on 64 slots, 2 frames"""
    rng = np.random.default_rng(35)
    skel = [TC.skeleton(rng) for _ in range(64)]
    centre = np.array([[2000.0 * (k % 8), 2000.0 * (k // 8), 900.0] for k in range(64)])
    frames, truth = [], []
    for f in range(2):
        clean = [centre[k] + 30.0 * f + skel[k] for k in range(64)]
        frames.append([[(k, clean[k] + rng.normal(scale=5.0, size=(J, 3)), 0.99 - 0.01 * k) for k in range(64)]])
        truth.append(_truth([clean], 64))
    return _case(frames, truth, 64, T=64, K=64)


def cases():
    """name -> case, everything but the full size (which only the device runs)"""
    return dict(perfect=perfect(), occlusion=occlusion(), min_hits=min_hits(), ghost=ghost(), small_table=small_table(),
                kept_pairs=kept_pairs(), kept_pairs_cleared=kept_pairs(clear=True), contested=contested(),
                threshold_on=threshold(512.0), threshold_off=threshold(float(np.nextafter(512.0, 0.0))), visibility=visibility(),
                nan_detection=nan_detection(), annotation=annotation(), identities=identities(), no_count=no_count(),
                two_streams=two_streams())
