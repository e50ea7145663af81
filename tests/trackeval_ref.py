"""Plain-Python fp64 restatement of one mvg_track_eval frame (include/mvg_decoder.h, "CLEAR-MOT counts and the identity overlap
table"), written from the stated rules: scalar Python floats (IEEE fp64, every operation rounded on its own), plain loops, no
vector reductions.  The device kernel (csrc/track.hip) must reproduce it: every integer equal, dist_sum bit for bit.  Step 6 uses
the solver restatement of tests/track_ref.py."""
import itertools
import math

import numpy as np

from tests import track_ref as TR

STATE = ("frames", "gt", "hyp", "matches", "misses", "false_pos", "switches", "kept", "dropped", "unreported", "bad_id",
         "id_overflow", "reserved")
MAX_HYP = 64


def new_buffers(B, P, K):
    return dict(last_track=np.full((B, P), -1, np.int32), counters=np.zeros((B, len(STATE)), np.int64),
                dist_sum=np.zeros((B,), np.float64), seen=np.zeros((B, P), np.int64), covered=np.zeros((B, P), np.int64),
                overlap=np.zeros((B, P, K), np.int32))


def distance(pose, person, vis):
    """pose (J, >= 3) fp32, person (J, 3) fp32, vis (J) fp32 -> the mean over the visible joints, in joint order"""
    total, n = 0.0, 0
    for j in range(person.shape[0]):
        if not vis[j] > 0:
            continue
        dx = float(pose[j, 0]) - float(person[j, 0])
        dy = float(pose[j, 1]) - float(person[j, 1])
        dz = float(pose[j, 2]) - float(person[j, 2])
        sq = (dx * dx + dy * dy) + dz * dz
        total += math.sqrt(sq) if sq == sq and sq >= 0.0 else float("nan")
        n += 1
    return total / float(n)


def update(dets, count, ids, joints_3d, joints_3d_vis, num_person, buf, dist_thr=500.0, row_pose=None, person_id=None):
    """one frame of every stream, in place on ``buf`` (new_buffers)"""
    dets = np.asarray(dets, np.float32)
    B, R, J = dets.shape[:3]
    G = joints_3d.shape[1]
    P, K = buf["overlap"].shape[1:]
    thr = float(dist_thr)
    for b in range(B):
        c = dict.fromkeys(STATE, 0)
        # 1
        if int(num_person[b]) < 0:
            continue
        # 2
        rows = R if count is None else min(max(int(count[b, 0]), 0), R)
        hyp = []
        for i in range(rows):
            if dets[b, i, 0, 3] >= 0:
                if ids[b, i] >= 0:
                    hyp.append(i)
                else:
                    c["unreported"] += 1
        c["dropped"] = max(len(hyp) - MAX_HYP, 0)
        hyp = hyp[:MAX_HYP]
        hid = [int(ids[b, i]) for i in hyp]
        # 3
        persons, pid = [], []
        for g in range(min(int(num_person[b]), G)):
            if not any(joints_3d_vis[b, g, j] > 0 for j in range(J)):
                continue
            p = g if person_id is None else int(person_id[b, g])
            if p < 0 or p >= P or p in pid:
                c["bad_id"] += 1
                continue
            persons.append(g)
            pid.append(p)
        # 4
        d = [[distance(dets[b, i] if row_pose is None else row_pose[b, i], joints_3d[b, g], joints_3d_vis[b, g]) for i in hyp]
             for g in persons]
        # 5
        match = [-1] * len(persons)
        taken = [False] * len(hyp)
        for a, p in enumerate(pid):
            last = int(buf["last_track"][b, p])
            if last < 0 or last not in hid:
                continue
            h = hid.index(last)
            if not taken[h] and d[a][h] <= thr:
                match[a], taken[h] = h, True
                c["kept"] += 1
        # 6
        rest_p = [a for a in range(len(persons)) if match[a] < 0]
        rest_h = [h for h in range(len(hyp)) if not taken[h]]
        if rest_p and rest_h:
            gated = np.zeros((len(rest_p), len(rest_h)), np.float64)
            for i, a in enumerate(rest_p):
                for j, h in enumerate(rest_h):
                    gated[i, j] = d[a][h] if d[a][h] <= thr else thr
            col, _ = TR.solve(gated)
            for i, a in enumerate(rest_p):
                j = int(col[i])
                if j >= 0 and d[a][rest_h[j]] <= thr:
                    match[a], taken[rest_h[j]] = rest_h[j], True
        # 7
        for a, p in enumerate(pid):
            buf["seen"][b, p] += 1
            if match[a] >= 0:
                c["matches"] += 1
                buf["dist_sum"][b] = float(buf["dist_sum"][b]) + d[a][match[a]]
                buf["covered"][b, p] += 1
                last, tid = int(buf["last_track"][b, p]), hid[match[a]]
                if last >= 0 and last != tid:
                    c["switches"] += 1
                buf["last_track"][b, p] = tid
            else:
                c["misses"] += 1
        # 8
        c["false_pos"] = len(hyp) - c["matches"]
        c["gt"], c["hyp"], c["frames"] = len(persons), len(hyp), 1
        # 9
        for a, p in enumerate(pid):
            for h, tid in enumerate(hid):
                if d[a][h] <= thr:
                    if tid < K:
                        buf["overlap"][b, p, tid] += 1
                    else:
                        c["id_overflow"] += 1
        for k, name in enumerate(STATE):
            buf["counters"][b, k] += c[name]
    return buf


def host_ids(case):
    """the tracker restatement (tests/track_ref.py) over the case's frames -> per frame a copy of its ids (B, R)"""
    B, R, J = case["frames"][0][0].shape[:3]
    tracks = TR.new_buffers(B, case["T"], J, R)
    out = []
    for dets, count in case["frames"]:
        ids, _ = TR.update(dets, count, tracks, case["max_dist"], case["max_misses"], case["min_hits"])
        out.append(np.array(ids, copy=True))
    return out


def run(case, ids, row_poses=None):
    """the restatement over a case (tests/trackeval_cases.py) for the given per-frame ids (and per-frame row_pose) -> per frame a
    copy of every buffer"""
    buf = new_buffers(case["frames"][0][0].shape[0], case["P"], case["K"])
    snaps = []
    for f, ((dets, count), (j3d, vis, num, pid)) in enumerate(zip(case["frames"], case["truth"])):
        if f in case["clear_last"]:
            buf["last_track"][:] = -1
        update(dets, count, ids[f], j3d, vis, num, buf, case["dist_thr"], None if row_poses is None else row_poses[f], pid)
        snaps.append({k: np.array(v, copy=True) for k, v in buf.items()})
    return snaps


def counters(buf, b=None):
    """the named counters of stream b, or summed over the streams"""
    row = buf["counters"].sum(axis=0) if b is None else buf["counters"][b]
    return dict(zip(STATE, (int(x) for x in row)))


def best_assignment(table):
    """brute force over all one-to-one assignments of rows to columns: the maximum total weight"""
    table = np.asarray(table)
    n, m = table.shape
    if n > m:
        table, n, m = table.T, m, n
    best = 0
    for cols in itertools.permutations(range(m), n):
        best = max(best, sum(int(table[r, c]) for r, c in enumerate(cols)))
    return best
