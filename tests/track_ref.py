"""numpy fp64 restatement of the assignment solver and of one tracker update (include/mvg_decoder.h, "person identities across
frames"), written from the stated rules: scalar Python floats (IEEE fp64, every operation rounded on its own), plain loops, no
vector reductions whose order is not defined.  The device kernels (csrc/track.hip) must reproduce it bit for bit."""
import itertools
import math

import numpy as np

LAP_MAX_N = 64
LAP_BIG = 1e15
TRACK_MAX_D = 64
TRACK_MAX_T = 64
STATE = ("frames", "matches", "births", "deaths", "overflow", "dropped", "active", "reserved")
INF = float("inf")


def solve(cost, n=None, m=None):
    """cost (N, M) fp64, live sizes n, m -> (col_of_row (N) int32, total): shortest augmenting paths with potentials, rows
    inserted in order, the minimum of a step taken at the lowest column among equals (a NaN minv ordered as +inf)."""
    cost = np.asarray(cost, np.float64)
    N, M = cost.shape
    n = N if n is None else min(max(int(n), 0), N)
    m = M if m is None else min(max(int(m), 0), M)
    s = max(n, m)
    S = [[0.0] * s for _ in range(s)]
    for i in range(n):
        for j in range(m):
            c = float(cost[i, j])
            S[i][j] = LAP_BIG if (c != c or c > LAP_BIG) else c
    VIRT = s                                   # the virtual column a search starts from
    u, v = [0.0] * s, [0.0] * s
    p = [-1] * (s + 1)                         # row of a column
    for i in range(s):
        p[VIRT] = i
        minv, way, used = [INF] * s, [VIRT] * s, [False] * (s + 1)
        j0, found = VIRT, False
        for _ in range(s):                     # a counted loop: at most i + 1 <= s steps are needed
            used[j0] = True
            i0 = p[j0]
            for j in range(s):
                if not used[j]:
                    cur = (S[i0][j] - u[i0]) - v[j]
                    if cur < minv[j]:
                        minv[j], way[j] = cur, j0
            j1, best = -1, INF
            for j in range(s):
                if not used[j]:
                    key = minv[j] if minv[j] == minv[j] else INF
                    if j1 < 0 or key < best:
                        j1, best = j, key
            delta = minv[j1]
            for j in range(s + 1):
                if used[j]:
                    u[p[j]] += delta
                    if j != VIRT:
                        v[j] -= delta
                else:
                    minv[j] -= delta
            j0 = j1
            if p[j0] < 0:
                found = True
                break
        if not found:
            continue
        for _ in range(s + 1):
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
            if j0 == VIRT:
                break
    col = np.full((N,), -1, np.int32)
    for j in range(min(m, s)):
        if 0 <= p[j] < n:
            col[p[j]] = j
    total = 0.0
    for r in range(n):
        if col[r] >= 0:
            total += float(cost[r, col[r]])
    return col, total


def brute_force(cost):
    """the optimum of the same padded problem over all permutations: (best total, second-best total over distinct assignments of
    the live rows to live columns / 'unassigned')"""
    cost = np.asarray(cost, np.float64)
    n, m = cost.shape
    s = max(n, m)
    S = np.zeros((s, s))
    S[:n, :m] = cost
    totals = {}
    for perm in itertools.permutations(range(s)):
        key = tuple(perm[i] if perm[i] < m else -1 for i in range(n))
        if key not in totals:
            totals[key] = sum(S[i, perm[i]] for i in range(s))
    order = sorted(totals.values())
    return order[0], (order[1] if len(order) > 1 else INF)


def joint_cost(pose, det):
    """(J, 3) fp32 track pose, (J, 5) fp32 detection -> mean joint distance in fp64, joints in order"""
    J = pose.shape[0]
    total = 0.0
    for j in range(J):
        dx = float(pose[j, 0]) - float(det[j, 0])
        dy = float(pose[j, 1]) - float(det[j, 1])
        dz = float(pose[j, 2]) - float(det[j, 2])
        sq = (dx * dx + dy * dy) + dz * dz
        total += math.sqrt(sq) if sq == sq and sq >= 0.0 else float("nan")
    return total / float(J)


def new_buffers(B, T, J, R):
    return dict(id=np.full((B, T), -1, np.int32), hits=np.zeros((B, T), np.int32), misses=np.zeros((B, T), np.int32),
                born=np.zeros((B, T), np.int64), score=np.zeros((B, T), np.float32), pose=np.zeros((B, T, J, 3), np.float32),
                next_id=np.zeros((B,), np.int32), state=np.zeros((len(STATE),), np.int64),
                ids=np.full((B, R), -1, np.int32), slots=np.full((B, R), -1, np.int32))


def update(dets, count, buf, max_dist, max_misses, min_hits):
    """one tracker update of every batch element, in place on ``buf`` (new_buffers); dets (B, R, J, 5) fp32, count (B, 2) or None"""
    dets = np.asarray(dets, np.float32)
    B, R, J = dets.shape[:3]
    T = buf["id"].shape[1]
    st = buf["state"]
    frame = int(st[0])
    max_dist = float(max_dist)
    for b in range(B):
        rows = R if count is None else min(max(int(count[b, 0]), 0), R)
        det_rows = [r for r in range(rows) if dets[b, r, 0, 3] >= 0]
        st[5] += max(len(det_rows) - TRACK_MAX_D, 0)
        det_rows = det_rows[:TRACK_MAX_D]
        active = [t for t in range(T) if buf["id"][b, t] >= 0]
        na, nd = len(active), len(det_rows)
        c = np.zeros((max(na, 1), max(nd, 1)), np.float64)
        for a, t in enumerate(active):
            for d, r in enumerate(det_rows):
                c[a, d] = joint_cost(buf["pose"][b, t], dets[b, r])
        gated = np.where(c <= max_dist, c, max_dist)
        col, _ = solve(gated, na, nd)
        det_slot = [-1] * nd
        for a, t in enumerate(active):
            d = int(col[a]) if a < len(col) else -1
            if d >= 0 and c[a, d] <= max_dist:
                det_slot[d] = t
                buf["misses"][b, t] = 0
                buf["hits"][b, t] += 1
                st[1] += 1
            else:
                buf["misses"][b, t] += 1
                if buf["misses"][b, t] > max_misses:
                    buf["id"][b, t] = -1
                    st[3] += 1
                    st[6] -= 1
        for d in range(nd):
            if det_slot[d] >= 0:
                continue
            free = [t for t in range(T) if buf["id"][b, t] < 0]
            if not free:
                st[4] += 1
                continue
            t = free[0]
            det_slot[d] = t
            buf["id"][b, t] = buf["next_id"][b]
            buf["next_id"][b] += 1
            buf["hits"][b, t], buf["misses"][b, t], buf["born"][b, t] = 1, 0, frame
            st[2] += 1
            st[6] += 1
        buf["ids"][b], buf["slots"][b] = -1, -1
        for d, r in enumerate(det_rows):
            t = det_slot[d]
            if t < 0:
                continue
            buf["pose"][b, t] = dets[b, r, :, :3]
            buf["score"][b, t] = dets[b, r, 0, 4]
            buf["slots"][b, r] = t
            if buf["hits"][b, t] >= min_hits:
                buf["ids"][b, r] = buf["id"][b, t]
    st[0] += 1
    return buf["ids"], buf["slots"]
