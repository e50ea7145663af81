"""numpy restatement of mvg_track_bones (csrc/bones.hip, contract in include/mvg_decoder.h), written from the stated rules: scalar
Python floats (IEEE fp64, every operation rounded on its own) for the distances, one rounding to fp32 per length, ranks counted
as the contract counts them.  The device kernel must reproduce it bit for bit.

    new_buffers(B, T, J, R, W)                                     the caller's state and outputs, as ops.track_bones_buffers
    update(dets, count, slots, ident, parent, buf, min_frames, fallback)      one call, in place on ``buf``
        = advance(...) (steps 1-3, the state) + rows(...) (step 4, the outputs; depends on min_frames and fallback only)
    median(samples)                                                the estimate of one bone from the n samples of its ring
"""
import math

import numpy as np

BONES_MAX_W = 32
SEEN_CAP = 1 << 30
STATE = ("owner", "seen", "hist", "length")
OUTPUTS = ("row_length", "row_source")


def new_buffers(B, T, J, R, W):
    K = J - 1
    return dict(owner=np.full((B, T), -1, np.int32), seen=np.zeros((B, T), np.int32), hist=np.zeros((B, T, W, K), np.float32),
                length=np.zeros((B, T, K), np.float32), row_length=np.zeros((B, R, K), np.float32),
                row_source=np.full((B, R), -1, np.int32))


def bone(row, parent, k):
    """row (J, >= 3) fp32 -> the length of the bone that ends at joint k: sqrt((dx*dx + dy*dy) + dz*dz) in fp64 from the fp32
    inputs, rounded once to fp32"""
    p = int(parent[k])
    dx = float(row[k, 0]) - float(row[p, 0])
    dy = float(row[k, 1]) - float(row[p, 1])
    dz = float(row[k, 2]) - float(row[p, 2])
    sq = (dx * dx + dy * dy) + dz * dz
    d = math.sqrt(sq) if sq == sq else float("nan")
    with np.errstate(over="ignore"):
        return np.float32(d)


def bones_of(row, parent):
    return np.array([bone(row, parent, k) for k in range(1, len(parent))], np.float32)


def median(samples):
    """samples: n fp32 values -> fp32: selected by rank (the number of smaller samples plus the equal ones at a lower index); the
    middle value for n odd, (float)(((double) lo + (double) hi) * 0.5) of the two middle values for n even"""
    v = [np.float32(x) for x in samples]
    n = len(v)
    by_rank = [None] * n
    for i in range(n):
        rank = 0
        for j in range(n):
            if v[j] < v[i] or (v[j] == v[i] and j < i):
                rank += 1
        by_rank[rank] = v[i]
    if n % 2:
        return by_rank[n // 2]
    return np.float32((float(by_rank[n // 2 - 1]) + float(by_rank[n // 2])) * 0.5)


def median_columns(h):
    """h (n, K) fp32 -> (K) fp32: ``median`` of every column, the ranks counted for all columns at once"""
    h = np.asarray(h, np.float32)
    n = h.shape[0]
    lower = np.tri(n, k=-1, dtype=bool).T                                   # lower[j, i]: j < i
    rank = ((h[:, None, :] < h[None, :, :]) | ((h[:, None, :] == h[None, :, :]) & lower[:, :, None])).sum(axis=0)     # (i, K)
    pick = lambda r: np.take_along_axis(h, np.argmax(rank == r, axis=0)[None, :], axis=0)[0]
    if n % 2:
        return pick(n // 2)
    return ((pick(n // 2 - 1).astype(np.float64) + pick(n // 2).astype(np.float64)) * 0.5).astype(np.float32)


def detections(dets, count, b):
    R = dets.shape[1]
    rows = R if count is None else min(max(int(count[b, 0]), 0), R)
    return [i for i in range(rows) if dets[b, i, 0, 3] >= 0]


def advance(dets, count, slots, ident, parent, buf):
    """steps 1-3 on the state of ``buf``"""
    dets = np.asarray(dets, np.float32)
    B, R, J = dets.shape[:3]
    T, W = buf["owner"].shape[1], buf["hist"].shape[2]
    assert 1 <= W <= BONES_MAX_W and len(parent) == J
    for b in range(B):
        for t in range(T):                                                  # 1. ownership
            if ident[b, t] != buf["owner"][b, t]:
                buf["owner"][b, t] = ident[b, t]
                buf["seen"][b, t] = 0
                buf["length"][b, t] = 0.0
        named = set()
        for i in detections(dets, count, b):                                # 2. sample: the lowest detection row of every slot
            s = int(slots[b, i])
            if not 0 <= s < T or s in named:
                continue
            named.add(s)
            own = bones_of(dets[b, i], parent)
            if not np.all(np.isfinite(own)):
                continue
            buf["hist"][b, s, int(buf["seen"][b, s]) % W] = own
            buf["seen"][b, s] = min(int(buf["seen"][b, s]) + 1, SEEN_CAP)
            n = min(int(buf["seen"][b, s]), W)                              # 3. estimate
            buf["length"][b, s] = median_columns(buf["hist"][b, s, :n])
    return buf


def rows(dets, count, slots, parent, buf, min_frames=4, fallback=None):
    """step 4 -> (row_length, row_source) of ``buf``"""
    dets = np.asarray(dets, np.float32)
    B, T = dets.shape[0], buf["owner"].shape[1]
    assert min_frames >= 1
    buf["row_length"][:] = 0.0
    buf["row_source"][:] = -1
    for b in range(B):
        for i in detections(dets, count, b):
            s = int(slots[b, i])
            if 0 <= s < T and buf["seen"][b, s] >= min_frames:
                buf["row_length"][b, i], buf["row_source"][b, i] = buf["length"][b, s], 0
            elif fallback is not None:
                buf["row_length"][b, i], buf["row_source"][b, i] = np.asarray(fallback, np.float32), 1
            else:
                buf["row_length"][b, i], buf["row_source"][b, i] = bones_of(dets[b, i], parent), 2
    return buf["row_length"], buf["row_source"]


def update(dets, count, slots, ident, parent, buf, min_frames=4, fallback=None):
    """dets (B, R, J, 5) fp32, count (B, 2) or None, slots (B, R) and ident (B, T) int32 as the tracker leaves them"""
    advance(dets, count, slots, ident, parent, buf)
    return rows(dets, count, slots, parent, buf, min_frames, fallback)
