"""Plain-Python fp64 restatement of the tracker's constant-velocity motion model (include/mvg_decoder.h, mvg_track_predict and
mvg_track_correct), written from the stated rules: scalar Python floats (IEEE fp64, every operation rounded on its own), plain
loops.  One frame is predict -> tests/track_ref.py update (imported as it is) -> correct.  The device kernels (csrc/track.hip)
must reproduce it bit for bit.  The test sequences of the motion model are at the bottom."""
import numpy as np

from tests import track_cases as TC
from tests import track_ref as TR

DEFAULTS = dict(dt=1.0, q=25.0, r=400.0, v0=2500.0)          # tracking.PoseTracker's defaults


def new_motion(B, T, J, R):
    return dict(mean=np.zeros((B, T, J, 2, 3), np.float64), var=np.zeros((B, T, 3), np.float64),
                row_pose=np.zeros((B, R, J, 3), np.float32))


def predict(buf, mot, dt, q):
    """every live slot one step ahead, in place: x += v dt, the covariance through F P F' + Q, pose = (float) x"""
    dt, q = float(dt), float(q)
    B, T, J = mot["mean"].shape[:3]
    dt2 = dt * dt
    dt3 = dt2 * dt
    dt4 = dt2 * dt2
    qxx, qxv, qvv = (q * dt4) / 4.0, (q * dt3) / 2.0, q * dt2
    for b in range(B):
        for t in range(T):
            if buf["id"][b, t] < 0:
                continue
            for j in range(J):
                for a in range(3):
                    x, v = float(mot["mean"][b, t, j, 0, a]), float(mot["mean"][b, t, j, 1, a])
                    x = x + v * dt
                    mot["mean"][b, t, j, 0, a] = x
                    buf["pose"][b, t, j, a] = np.float32(x)
            pxx, pxv, pvv = (float(p) for p in mot["var"][b, t])
            mot["var"][b, t, 0] = ((pxx + (2.0 * dt) * pxv) + dt2 * pvv) + qxx
            mot["var"][b, t, 1] = (pxv + dt * pvv) + qxv
            mot["var"][b, t, 2] = pvv + qvv


def correct(buf, mot, r, v0):
    """every slot by its state after the update, in place, then the filtered pose of every row"""
    r, v0 = float(r), float(v0)
    B, T, J = mot["mean"].shape[:3]
    R = mot["row_pose"].shape[1]
    for b in range(B):
        for t in range(T):
            ident, hits, misses = int(buf["id"][b, t]), int(buf["hits"][b, t]), int(buf["misses"][b, t])
            if ident < 0:                                     # free
                mot["mean"][b, t] = 0.0
                mot["var"][b, t] = 0.0
            elif misses > 0:                                  # missed: the prediction stands
                pass
            elif hits == 1:                                   # born in this call
                for j in range(J):
                    for a in range(3):
                        mot["mean"][b, t, j, 0, a] = float(buf["pose"][b, t, j, a])
                        mot["mean"][b, t, j, 1, a] = 0.0
                mot["var"][b, t] = (r, 0.0, v0)
            else:                                             # matched: pose holds the detection
                pxx, pxv, pvv = (float(p) for p in mot["var"][b, t])
                s = pxx + r
                kx, kv = pxx / s, pxv / s
                for j in range(J):
                    for a in range(3):
                        x, v = float(mot["mean"][b, t, j, 0, a]), float(mot["mean"][b, t, j, 1, a])
                        e = float(buf["pose"][b, t, j, a]) - x
                        x = x + kx * e
                        v = v + kv * e
                        mot["mean"][b, t, j, 0, a], mot["mean"][b, t, j, 1, a] = x, v
                        buf["pose"][b, t, j, a] = np.float32(x)
                mot["var"][b, t, 2] = pvv - kv * pxv
                mot["var"][b, t, 1] = (1.0 - kx) * pxv
                mot["var"][b, t, 0] = (1.0 - kx) * pxx
        for row in range(R):
            slot = int(buf["slots"][b, row])
            mot["row_pose"][b, row] = buf["pose"][b, slot] if slot >= 0 else 0.0


def step(dets, count, buf, mot, params, max_dist, max_misses, min_hits):
    """one frame with the motion model on (params: dt, q, r, v0); params None: the plain update"""
    if params is None:
        return TR.update(dets, count, buf, max_dist, max_misses, min_hits)
    p = dict(DEFAULTS, **params)
    predict(buf, mot, p["dt"], p["q"])
    ids, slots = TR.update(dets, count, buf, max_dist, max_misses, min_hits)
    correct(buf, mot, p["r"], p["v0"])
    return ids, slots


def live_only(buf):
    """tracker buffers with the hits / misses / born / score / pose of FREE slots blanked (whatever the last owner left); the
    motion buffers need no blanking: correct() writes zeros into free slots"""
    out = {k: np.array(v, copy=True) for k, v in buf.items()}
    free = out["id"] < 0
    for k in ("hits", "misses", "born", "score"):
        out[k][free] = 0
    out["pose"][free] = 0
    return out


def run(seq, motion="seq"):
    """the restatement over a sequence -> per frame a dict of copies of every buffer (tracker state live_only, motion buffers as
    they are).  motion: "seq" = the sequence's own parameters, None = the motion-free tracker, or a dict."""
    params = seq["motion"] if motion == "seq" else motion
    B, R, J = seq["frames"][0][0].shape[:3]
    buf, mot = TR.new_buffers(B, seq["T"], J, R), new_motion(B, seq["T"], J, R)
    snaps = []
    for dets, count in seq["frames"]:
        step(dets, count, buf, mot, params, seq["max_dist"], seq["max_misses"], seq["min_hits"])
        snap = live_only(buf)
        snap.update({k: v.copy() for k, v in mot.items()})
        snaps.append(snap)
    return snaps


def ids_per_person(seq, snaps):
    """per frame and batch element {person: id} as the rows report it"""
    return [[{int(w): int(i) for w, i in zip(who[b], s["ids"][b]) if w >= 0} for b in range(who.shape[0])]
            for s, who in zip(snaps, seq["persons"])]


# ------------------------------------------------------------------------------------------------------------------- sequences
R_ROWS, T_SLOTS = 8, 8
WALK_STEP, WALK_SEEN, WALK_GONE = 60.0, 12, 10


def _line(rng, n_frames, step, heading, centre, noise, skel):
    """(true, seen) poses of one person on a straight line: seen = true + uniform noise in [-noise, noise]"""
    heading = np.asarray(heading, np.float64)
    heading = heading / np.linalg.norm(heading)
    true = [np.asarray(centre, np.float64) + step * f * heading + skel for f in range(n_frames)]
    return true, [p + rng.uniform(-noise, noise, size=p.shape) for p in true]


def _seq(frames_people, motion=None, **kw):
    seq = TC._sequence(frames_people, kw.pop("R", R_ROWS), T=kw.pop("T", T_SLOTS), **kw)
    seq["motion"] = dict(DEFAULTS, **(motion or {}))
    return seq


def walk_occluded():
    """one person moving 60 mm per frame, seen in frames 0..11, absent for exactly max_misses = 10 frames, then back: 660 mm from
    the last seen pose, beyond max_dist = 500"""
    rng = np.random.default_rng(21)
    n = WALK_SEEN + WALK_GONE + 3
    _, seen = _line(rng, n, WALK_STEP, (0.8, 0.6, 0.0), (-500.0, 300.0, 900.0), 5.0, TC.skeleton(rng))
    frames = [[[(0, seen[f], 0.9)] if not (WALK_SEEN <= f < WALK_SEEN + WALK_GONE) else []] for f in range(n)]
    return _seq(frames, max_misses=WALK_GONE)


def cross_fast(dt=1.0):
    """two people of one skeleton at +-80 mm per frame on lines 50 mm apart, passing each other between frames 10 and 11: there
    each is 50 mm from the other's last pose and 80 mm from its own"""
    rng = np.random.default_rng(22)
    skel = TC.skeleton(rng)
    a = _line(rng, 22, 80.0, (1.0, 0.0, 0.0), (-840.0, 0.0, 900.0), 1.0, skel)[1]
    b = _line(rng, 22, 80.0, (-1.0, 0.0, 0.0), (840.0, 50.0, 900.0), 1.0, skel)[1]
    return _seq([[TC._by_score(rng, [a[f], b[f]])] for f in range(22)], motion=dict(dt=dt))


def noisy_walk():
    """one person on a straight line with seeded +-5 mm noise on every coordinate; ``truth`` holds the noise-free poses"""
    rng = np.random.default_rng(23)
    true, seen = _line(rng, 30, WALK_STEP, (0.6, -0.8, 0.0), (0.0, 0.0, 900.0), 5.0, TC.skeleton(rng))
    seq = _seq([[[(0, p, 0.9)]] for p in seen])
    seq["truth"] = true
    return seq


def reborn():
    """max_misses = 0: person 0 leaves in frame 3 and person 1 appears in the same frame far away: the slot is freed and reopened
    in one update; person 2 is followed throughout"""
    rng = np.random.default_rng(24)
    lines = [_line(rng, 6, 30.0, rng.normal(size=3), (3000.0 * k, 0.0, 900.0), 5.0, TC.skeleton(rng))[1] for k in range(3)]
    present = [{0, 2}] * 3 + [{1, 2}] * 3
    return _seq([[TC._by_score(rng, [l[f] for l in lines], present[f])] for f in range(6)], max_misses=0)


def nan_pose():
    """tests/track_cases.nan_pose with the motion model on: the NaN detection's track carries NaN in one coordinate until it dies"""
    seq = TC.nan_pose()
    seq["motion"] = dict(DEFAULTS)
    return seq


def two_streams():
    """B = 2 with different histories: element 0 follows two persons, one of them absent in frames 3..4; element 1 one person
    and from frame 2 a second"""
    rng = np.random.default_rng(25)
    a = [_line(rng, 8, 50.0, rng.normal(size=3), (2500.0 * k, 0.0, 900.0), 5.0, TC.skeleton(rng))[1] for k in range(2)]
    b = [_line(rng, 8, 35.0, rng.normal(size=3), (2500.0 * k, 500.0, 900.0), 5.0, TC.skeleton(rng))[1] for k in range(2)]
    frames = [[TC._by_score(rng, [l[f] for l in a], {0} if f in (3, 4) else {0, 1}),
               TC._by_score(rng, [l[f] for l in b], {0} if f < 2 else {0, 1})] for f in range(8)]
    return _seq(frames, R=4, T=4)


def sequences():
    """name -> sequence, every case of tests/test_track_motion_gpu.py"""
    return dict(walk_occluded=walk_occluded(), cross_fast=cross_fast(), noisy_walk=noisy_walk(), reborn=reborn(),
                nan_pose=nan_pose(), two_streams=two_streams(), dt_half=cross_fast(dt=0.5))
