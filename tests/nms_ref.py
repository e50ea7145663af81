"""Plain-loop numpy restatement of the device NMS contract (include/mvg_decoder.h, mvg_pose_nms): the reference's
nearby-joints NMS (lib/core/nms.py:210-283) with the points the reference leaves open pinned down --

  * visiting order  descending score, among equal scores the higher row first: np.argsort(scores, kind="stable")[::-1]
                    (the reference's default argsort is unstable; same order wherever numpy uses insertion sort, N <= 16);
  * best            highest score of the neighbourhood, among equal scores the lowest row (np.argmax);
  * max_dets        np.argsort(scores[keep], kind="stable")[-1:-max_dets-1:-1];
  * empty row       a candidate whose own neighbourhood is empty (zero extent, NaN coordinate) is visited, counted, and neither
                    kept nor suppressing (the reference raises inside np.argmax).

Arithmetic: fp64 on whatever the array holds, every multiply and add rounded on its own, the squared distance summed as
(x^2 + y^2) + z^2 like np.sum over three elements, np.sqrt.  Pinned to tests/golden/eval.npz and to the product's and the
oracle's host NMS in tests/test_pose_nms_cpu.py."""
import numpy as np


def close_matrix(kpts, dist_thr, num_nearby_joints_thr):
    """kpts (M, J, 3) float64 -> bool (M, M); row a uses pose a's own limit (not symmetric)."""
    M = len(kpts)
    close = np.zeros((M, M), dtype=bool)
    for a in range(M):
        span = kpts[a].max(0) - kpts[a].min(0)                       # NaN propagates like the reference's np.max / np.min
        sq = span * span
        limit = np.sqrt((sq[0] + sq[1]) + sq[2]) * dist_thr
        d = kpts[a][None] - kpts                                     # (M, J, 3)
        sq = d * d
        dist = np.sqrt((sq[..., 0] + sq[..., 1]) + sq[..., 2])       # (M, J)
        with np.errstate(invalid="ignore"):
            close[a] = (dist < limit).sum(1) > num_nearby_joints_thr
    return close


def nms_core(kpts, scores, dist_thr, num_nearby_joints_thr=None, max_dets=-1):
    """-> (keep: list of indices into kpts in keep order, skipped, stats).  stats counts the branches the greedy pass took:
    asymmetric entries of `close`, visits whose best was another pose, visits whose best was already ignored."""
    assert dist_thr > 0, "`dist_thr` must be greater than 0."
    kpts = np.asarray(kpts, dtype=np.float64)
    scores = np.asarray(scores, dtype=np.float64)
    M, J = kpts.shape[:2]
    if num_nearby_joints_thr is None:
        num_nearby_joints_thr = J // 2
    assert num_nearby_joints_thr < J, "`num_nearby_joints_thr` must be less than the number of joints."
    close = close_matrix(kpts, dist_thr, num_nearby_joints_thr)
    stats = dict(asymmetric=int((close != close.T).sum()), best_is_other=0, best_ignored=0)
    ignored = np.zeros(M, dtype=bool)
    keep, skipped = [], 0
    for i in np.argsort(scores, kind="stable")[::-1]:
        if ignored[i]:
            continue
        nb = [b for b in range(M) if close[i, b]]
        if not nb:
            skipped += 1
            continue
        best = nb[0]
        for b in nb[1:]:                                             # first maximum = lowest row, a NaN score is a maximum
            if scores[b] > scores[best] or (np.isnan(scores[b]) and not np.isnan(scores[best])):
                best = b
        stats["best_is_other"] += int(best != i)
        if ignored[best]:
            stats["best_ignored"] += 1
            continue
        keep.append(int(best))
        ignored[nb] = True
    if max_dets > 0 and len(keep) > max_dets:
        order = np.argsort(scores[keep], kind="stable")[-1:-max_dets - 1:-1]
        keep = [keep[i] for i in order]
    return keep, skipped, stats


def nearby_joints_nms(db, dist_thr, num_nearby_joints_thr=None, max_dets=-1):
    """the host functions' interface: every row of db (N, J, >= 5) is a candidate; returns the keep list"""
    db = np.asarray(db, dtype=np.float64)
    if len(db) == 0:
        return []
    return nms_core(db[:, :, :3], db[:, 0, 4], dist_thr, num_nearby_joints_thr, max_dets)[0]


def pose_nms(pred, dist_thr=0.3, num_nearby_joints_thr=7, max_dets=-1):
    """one batch element of mvg_pose_nms: pred (N, J, 5) -> (keep: row indices of pred, count [kept, skipped], dets: the kept
    rows in pred's dtype, stats)"""
    pred = np.asarray(pred)
    rows = np.flatnonzero(pred[:, 0, 3] >= 0)
    if len(rows) == 0:
        return [], [0, 0], pred[:0], dict(asymmetric=0, best_is_other=0, best_ignored=0)
    cand = pred[rows].astype(np.float64)
    keep, skipped, stats = nms_core(cand[:, :, :3], cand[:, 0, 4], dist_thr, num_nearby_joints_thr, max_dets)
    keep = [int(rows[k]) for k in keep]
    return keep, [len(keep), skipped], pred[keep], stats
