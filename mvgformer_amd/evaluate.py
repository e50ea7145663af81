"""Evaluation post-processing of the decoder's predictions.

What ``run/validate_3d.py:204-284`` does with the packed predictions ``[x, y, z, (score > thr) - 1, score]``
(``mvgformer_amd.caller.pack_predictions``): classification filter + nearby-joints NMS
(``lib/core/nms.py:210-283``), then AP@25..150 mm / recall / MPJPE on Panoptic
(``lib/dataset/panoptic.py:493-574,711-764``) or PCP on Shelf / Campus (``lib/dataset/shelf.py:255-330``,
``lib/dataset/campus.py:250-320``).

The reference evaluates in nested Python loops over numpy arrays on the host (and its NMS builds an
(N, N, J, 3) fp64 temporary: 377 MB for 1024 candidates).  Here the two dense parts -- the pose-to-pose joint
distances of the NMS and the prediction-to-ground-truth MPJPE matrix -- are batched tensor ops that run on
whatever device the predictions live on (the MI355X when they come straight from the decoder), and only the
inherently sequential greedy steps (suppression order, first-match-wins AP bookkeeping) run on the host over
the small boolean / index results.  Numerics: distances are computed in fp64 like the reference's numpy code:
keep-lists and matches are identical, metrics agree to 1e-12 (summation order of the joint means differs;
tests/test_evaluate.py against golden vectors produced by the reference's own functions).
"""
from __future__ import annotations

import contextlib
from collections import OrderedDict

import numpy as np
import torch

__all__ = ["nearby_joints_nms", "filter_and_nms", "filter_and_nms_device", "match_predictions", "eval_list_to_ap", "eval_list_to_mpjpe",
           "eval_list_to_recall", "evaluate_panoptic", "evaluate_pcp", "MPJPE_THRESHOLDS", "PCP_LIMBS", "DeviceEvaluator"]

MPJPE_THRESHOLDS = tuple(range(25, 155, 25))            # panoptic.py:559
PCP_LIMBS = ((0, 1), (1, 2), (3, 4), (4, 5), (6, 7), (7, 8), (9, 10), (10, 11), (12, 13))   # shelf.py:270-271
PCP_BONE_GROUPS = OrderedDict([("Head", [8]), ("Torso", [9]), ("Upper arms", [5, 6]), ("Lower arms", [4, 7]),
                               ("Upper legs", [1, 2]), ("Lower legs", [0, 3])])              # shelf.py:316-319


def _as_tensor(x, device=None):
    if isinstance(x, torch.Tensor):
        return x.detach().to(torch.float64)
    return torch.as_tensor(np.asarray(x), dtype=torch.float64, device=device)


# --------------------------------------------------------------------------------------- NMS
def nearby_joints_nms(kpts_db, dist_thr, num_nearby_joints_thr=None, max_dets=-1):
    """lib/core/nms.py:210-283 for the combined input format used by validate_3d.py:231:
    ``kpts_db`` (N, J, >=5) rows ``[x, y, z, flag, score]`` (numpy or torch, any device).  Two poses are "close"
    when more than ``num_nearby_joints_thr`` of their joints are nearer than ``dist_thr`` x the diagonal of the
    first pose's bounding box; in descending score order every not-yet-ignored pose hands its slot to the best
    scored member of its neighbourhood and the whole neighbourhood is ignored from then on.
    Returns the list of kept indices in keep order."""
    if not dist_thr > 0:
        raise AssertionError("`dist_thr` must be greater than 0.")                   # nms.py:233
    if len(kpts_db) == 0:
        return []
    db = _as_tensor(kpts_db)
    scores = db[:, 0, 4]
    kpts = db[:, :, :3]
    n, J, _ = kpts.shape
    if num_nearby_joints_thr is None:
        num_nearby_joints_thr = J // 2
    if not num_nearby_joints_thr < J:
        raise AssertionError("`num_nearby_joints_thr` must be less than the number of joints.")
    # distance threshold per (row) pose: dist_thr x bounding-box diagonal (nms.py:255-260)
    area = torch.sqrt(((kpts.max(1).values - kpts.min(1).values) ** 2).sum(1))       # (N,)
    thr = area * dist_thr
    # joint-wise distances between all pose pairs, one joint at a time: (N, N) per joint instead of the
    # reference's (N, N, J, 3) temporary (nms.py:263-266)
    close_cnt = torch.zeros((n, n), dtype=torch.int32, device=kpts.device)
    for j in range(J):
        d = kpts[:, None, j, :] - kpts[None, :, j, :]
        close_cnt += (torch.sqrt((d ** 2).sum(-1)) < thr[:, None]).to(torch.int32)
    close = (close_cnt > num_nearby_joints_thr).cpu().numpy()
    sc = scores.cpu().numpy()
    # greedy suppression (nms.py:268-277); np.argsort(...)[::-1] as in the reference (tie order included)
    ignored, keep = set(), []
    for i in np.argsort(sc)[::-1]:
        if i in ignored:
            continue
        nb = close[i].nonzero()[0]
        best = nb[np.argmax(sc[nb])]
        if best not in ignored:
            keep.append(int(best))
            ignored.update(int(k) for k in nb)
    if max_dets > 0 and len(keep) > max_dets:                                         # nms.py:280-282
        sub = np.argsort(sc[keep])[-1:-max_dets - 1:-1]
        keep = [keep[i] for i in sub]
    return keep


def filter_and_nms(pred, dist_thr=0.3, num_nearby_joints_thr=7):
    """validate_3d.py:228-234: drop candidates below the classification threshold (flag column < 0), then NMS
    with the reference's default thresholds.  pred (N, J, 5) numpy or torch; returns the surviving rows."""
    keep_cls = pred[:, 0, 3] >= 0
    pred = pred[keep_cls]
    idx = nearby_joints_nms(pred, dist_thr, num_nearby_joints_thr)
    return pred[idx]


def filter_and_nms_device(pred, dist_thr=0.3, num_nearby_joints_thr=7, max_dets=-1):
    """``filter_and_nms`` as one device operator (``ops.pose_nms``: classification filter, closeness matrix and the greedy pass
    in three launches, no N x N matrix on the host, no Python loop).  pred (N, J, 5) or (B, N, J, 5) fp32 on the device;
    returns the surviving rows in keep order, as a list over the batch when batched.  One read-back for the whole batch: the
    kept counts; the rows are slices of the gathered ``dets``.
    Same arithmetic as ``nearby_joints_nms`` (numpy's fp64).  Candidates are visited in descending score and, among EQUAL scores,
    the higher row first (``np.argsort(scores, kind="stable")[::-1]``): the reference's default argsort is unstable, so its order
    among tied scores is unspecified; it coincides with this rule where numpy falls back to insertion sort (N <= 16).  A
    candidate whose own neighbourhood is empty (zero-extent pose, NaN coordinate) is ignored, where ``nearby_joints_nms`` raises
    inside ``np.argmax`` like the reference."""
    from . import ops
    batched = pred.dim() == 4
    p = (pred if batched else pred[None]).contiguous()
    with torch.cuda.device(p.device) if p.is_cuda else contextlib.nullcontext():
        _, count, dets = ops.pose_nms(p, dist_thr, num_nearby_joints_thr, max_dets)
    kept = count[:, 0].tolist()                                                       # the one read-back
    rows = [dets[b, :k] for b, k in enumerate(kept)]
    return rows if batched else rows[0]


# --------------------------------------------------------------------------------------- AP / MPJPE / recall
def match_predictions(preds, gts, gts_vis, method="score_sort"):
    """panoptic.py:497-556: for every frame, every (classification-filtered) prediction is aligned with the
    ground-truth person of smallest MPJPE over the visible joints.
    preds: list over frames of (N_f, J, 5); gts / gts_vis: lists over frames of (G_f, J, 3) / (G_f, J, >=1)
    (frames with G_f == 0 are skipped like panoptic.py:508).  Returns (eval_list, total_gt) with
    eval_list = dict(mpjpe, score, gt_id) of equal-length float64 / int64 arrays in the reference's append
    order."""
    mp, sc, gid = [], [], []
    total_gt = 0
    for pred, gt, vis in zip(preds, gts, gts_vis):
        if len(gt) == 0:
            continue
        p = _as_tensor(pred)
        g = _as_tensor(gt, p.device)[..., :3]
        v = (_as_tensor(vis, p.device)[..., 0] > 0)                                   # (G, J)
        if method != "mpjpe_sort":
            p = p[p[:, 0, 3] >= 0]                                                    # panoptic.py:544
        if len(p):
            d = torch.sqrt(((p[:, None, :, :3] - g[None]) ** 2).sum(-1))              # (N, G, J)
            w = v.to(d.dtype)[None]
            # mean over the visible joints only (np.mean of the masked selection, panoptic.py:548-550); a person
            # without visible joints gives nan there -- same here (0/0)
            m = (d * w).sum(-1) / w.sum(-1)
            best = torch.min(_nan_last(m), dim=1)
            m_np, b_np = m.cpu().numpy(), best.indices.cpu().numpy()
            s_np = p[:, 0, 4].cpu().numpy()
            seen = set()
            for i in range(len(p)):
                gt_id = int(total_gt + b_np[i])
                if method == "mpjpe_sort":                                            # one prediction per gt, first wins
                    if gt_id in seen:
                        continue
                    seen.add(gt_id)
                mp.append(float(m_np[i, b_np[i]]))
                sc.append(float(s_np[i]))
                gid.append(gt_id)
        total_gt += len(gt)
    return dict(mpjpe=np.asarray(mp, np.float64), score=np.asarray(sc, np.float64), gt_id=np.asarray(gid, np.int64)), total_gt


def _nan_last(m):
    """np.argmin returns the first nan if there is one; persons without visible joints do not occur in the
    datasets, keep torch.min's behaviour well defined anyway."""
    return torch.where(torch.isnan(m), torch.full_like(m, float("inf")), m)


def _order(ev, method):
    # list.sort is stable, also with reverse=True (panoptic.py:713-717)
    if method == "score_sort":
        return np.argsort(-ev["score"], kind="stable")
    if method == "mpjpe_sort":
        return np.argsort(ev["mpjpe"], kind="stable")
    return np.arange(len(ev["score"]))


def _first_hits(ev, order, threshold):
    """true positives in `order`: mpjpe below the threshold and the gt not matched before (panoptic.py:723-729)."""
    mp, gid = ev["mpjpe"][order], ev["gt_id"][order]
    ok = mp < threshold
    first = np.zeros(len(order), dtype=bool)
    if ok.any():
        idx = np.flatnonzero(ok)
        _, pos = np.unique(gid[idx], return_index=True)          # first qualifying occurrence of every gt
        first[idx[pos]] = True
    return first


def eval_list_to_ap(ev, total_gt, threshold, method="score_sort"):
    """panoptic.py:711-741 -> (ap, recall)."""
    order = _order(ev, method)
    tp = _first_hits(ev, order, threshold)
    n = len(order)
    tpc = np.cumsum(tp.astype(np.float64))
    fpc = np.cumsum((~tp).astype(np.float64))
    recall = tpc / (total_gt + 1e-5)
    precise = tpc / (tpc + fpc + 1e-5)
    if n:
        precise = np.maximum.accumulate(precise[::-1])[::-1]       # panoptic.py:733-734
    precise = np.concatenate(([0.0], precise, [0.0]))
    recall = np.concatenate(([0.0], recall, [1.0]))
    index = np.where(recall[1:] != recall[:-1])[0]
    ap = np.sum((recall[index + 1] - recall[index]) * precise[index + 1])
    return float(ap), float(recall[-2])


def eval_list_to_mpjpe(ev, threshold=500, method="score_sort"):
    """panoptic.py:743-758: mean MPJPE of the true positives at `threshold` (inf when there are none)."""
    order = _order(ev, method)
    tp = _first_hits(ev, order, threshold)
    return float(np.mean(ev["mpjpe"][order][tp])) if tp.any() else float("inf")


def eval_list_to_recall(ev, total_gt, threshold=500):
    """panoptic.py:760-764."""
    return len(np.unique(ev["gt_id"][ev["mpjpe"] < threshold])) / total_gt


def evaluate_panoptic(preds, gts, gts_vis, method="score_sort"):
    """Panoptic.evaluate (panoptic.py:493-709) -> (aps, recalls, mpjpe, recall500) at 25..150 mm."""
    ev, total_gt = match_predictions(preds, gts, gts_vis, method)
    aps, recs = [], []
    for t in MPJPE_THRESHOLDS:
        ap, rec = eval_list_to_ap(ev, total_gt, t, method)
        aps.append(ap)
        recs.append(rec)
    return aps, recs, eval_list_to_mpjpe(ev, method=method), eval_list_to_recall(ev, total_gt)


# --------------------------------------------------------------------------------------- PCP (Shelf / Campus)
def evaluate_pcp(preds, actor_gts, recall_threshold=500, alpha=0.5):
    """Shelf.evaluate / Campus.evaluate (shelf.py:255-330) on in-memory ground truth.
    preds: list over evaluated frames of (N_f, J, 5); actor_gts: list over actors of lists over the same frames of
    (14, 3) arrays in mm, or None / empty where the actor is not annotated (the reference reads them from
    actorsGT.mat and skips empty entries, shelf.py:288-290).
    Returns (actor_pcp, avg_pcp, bone_person_pcp, recall)."""
    num_person = len(actor_gts)
    correct = np.zeros(num_person)
    total = np.zeros(num_person)
    bone_correct = np.zeros((num_person, 10))
    total_gt = match_gt = 0
    li = torch.as_tensor([k[0] for k in PCP_LIMBS])
    lj = torch.as_tensor([k[1] for k in PCP_LIMBS])
    for f, pred in enumerate(preds):
        p = _as_tensor(pred)
        p = p[p[:, 0, 3] >= 0][:, :, :3]                                              # shelf.py:281
        for person in range(num_person):
            gt = actor_gts[person][f]
            if gt is None or len(gt) == 0:
                continue
            if len(p) == 0:
                raise ValueError(_NO_PREDICTION % f)
            g = _as_tensor(gt, p.device)
            mp = torch.sqrt(((g[None] - p) ** 2).sum(-1)).mean(-1)                    # shelf.py:292-294
            n = int(torch.argmin(mp))
            if float(mp[n]) < recall_threshold:
                match_gt += 1
            total_gt += 1
            best = p[n]
            e_s = torch.linalg.norm(best[li] - g[li], dim=-1)
            e_e = torch.linalg.norm(best[lj] - g[lj], dim=-1)
            length = torch.linalg.norm(g[li] - g[lj], dim=-1)
            ok = ((e_s + e_e) / 2.0 <= alpha * length).cpu().numpy()
            total[person] += len(PCP_LIMBS)
            correct[person] += ok.sum()
            bone_correct[person, :len(PCP_LIMBS)] += ok
            p_hip, g_hip = (best[2] + best[3]) / 2.0, (g[2] + g[3]) / 2.0             # shelf.py:308-315
            total[person] += 1
            if float((torch.linalg.norm(p_hip - g_hip) + torch.linalg.norm(best[12] - g[12])) / 2.0) <= \
                    alpha * float(torch.linalg.norm(g_hip - g[12])):
                correct[person] += 1
                bone_correct[person, 9] += 1
    return _pcp_from_counters(correct, total, bone_correct, match_gt, total_gt)


_NO_PREDICTION = ("frame %d has ground truth but no prediction passed the classification filter "
                  "(the reference fails in np.stack here, shelf.py:284)")


def _pcp_from_counters(correct, total, bone_correct, match_gt, total_gt):
    """shelf.py:316-330: the counters -> (actor_pcp, avg_pcp, bone_person_pcp, recall)"""
    actor_pcp = correct / (total + 1e-8)
    avg_pcp = float(np.mean(actor_pcp[:3]))
    bone_person_pcp = OrderedDict((k, np.sum(bone_correct[:, v], axis=-1) / (total / 10 * len(v) + 1e-8))
                                  for k, v in PCP_BONE_GROUPS.items())
    return actor_pcp, avg_pcp, bone_person_pcp, match_gt / (total_gt + 1e-8)


# --------------------------------------------------------------------------------------- scoring on the device
def ground_truth_buffers(batch, max_persons, num_joints, device):
    """zeroed static inputs (joints_3d, joints_3d_vis, num_person) for ``max_persons`` person slots: what ``DeviceEvaluator`` and
    ``tracking.TrackEvaluator`` read under graph capture"""
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=device)
    return (z((batch, max_persons, num_joints, 3), torch.float32), z((batch, max_persons, num_joints), torch.float32),
            z((batch,), torch.int32))


class DeviceEvaluator:
    """``match_predictions`` (kind "panoptic") or the counters of ``evaluate_pcp`` (kind "pcp") accumulated in device memory by
    ``ops.eval_match`` / ``ops.eval_pcp``: ``update`` only launches (two launches / one, nothing read back, fixed shapes, so it can
    be captured in a HIP graph behind ``ops.pose_nms``), the metrics are read back once, by ``eval_list`` / ``panoptic`` / ``pcp``.

    update(dets, count, joints_3d, joints_3d_vis, num_person): ``dets`` (B, R, J, 5) fp32 and ``count`` (B, 2) int32 or None as
    ``ops.pose_nms`` leaves them (row i of element b takes part when its flag is >= 0 and i < count[b, 0]); the ground truth in the
    criterion's layout, (B, Gmax, J, 3) fp32, (B, Gmax, J) fp32 and (B) int32 with Gmax <= ``max_persons``.  Elements are frames,
    in call order.  ``capacity`` bounds the Panoptic entry list (one entry per kept pose of a frame with ground truth): entries
    past it are counted, not stored, and ``eval_list`` then raises with the capacity the run needs.  ``actors`` is the number of
    actor slots of the PCP counters.  ``method="mpjpe_sort"`` (per-frame de-duplication of the list) stays on the host path."""

    def __init__(self, kind="panoptic", capacity=65536, max_persons=10, actors=4, device="cuda", recall_threshold=500, alpha=0.5):
        if kind not in ("panoptic", "pcp"):
            raise ValueError("DeviceEvaluator: kind must be 'panoptic' or 'pcp' (got %r)" % (kind,))
        from . import ops
        if not 1 <= int(max_persons) <= ops.EVAL_MAX_G:
            raise ValueError("DeviceEvaluator: 1 <= max_persons <= %d expected (got %r)" % (ops.EVAL_MAX_G, max_persons))
        self.kind, self.capacity, self.max_persons, self.actors = kind, int(capacity), int(max_persons), int(actors)
        self.recall_threshold, self.alpha = float(recall_threshold), float(alpha)
        self.device = torch.device(device)
        self.buffers = ops.eval_buffers(self.capacity, self.actors, self.device)

    def ground_truth_buffers(self, batch, num_joints):
        """zeroed static inputs (joints_3d, joints_3d_vis, num_person) for ``max_persons`` person slots (graph capture)"""
        return ground_truth_buffers(batch, self.max_persons, num_joints, self.device)

    def update(self, dets, count, joints_3d, joints_3d_vis, num_person):
        from . import ops
        if joints_3d.dim() == 4 and joints_3d.shape[1] > self.max_persons:
            raise ValueError("DeviceEvaluator: %d person slots, built for max_persons = %d" % (joints_3d.shape[1], self.max_persons))
        with torch.cuda.device(dets.device) if dets.is_cuda else contextlib.nullcontext():
            if self.kind == "panoptic":
                ops.eval_match(dets, count, joints_3d, joints_3d_vis, num_person, self.buffers)
            else:
                ops.eval_pcp(dets, count, joints_3d, joints_3d_vis, num_person, self.buffers, self.recall_threshold, self.alpha)
        return self

    def reset(self):
        for t in self.buffers.values():
            t.zero_()
        return self

    def tensors(self):
        """every device tensor ``update`` addresses besides its arguments (what a captured graph must keep alive)"""
        return list(self.buffers.values())

    def snapshot(self):
        """clones of the accumulators (``restore`` puts them back: a graph capture's warm-up forwards must count no frame)"""
        return {k: t.clone() for k, t in self.buffers.items()}

    def restore(self, saved):
        for k, t in self.buffers.items():
            t.copy_(saved[k])
        return self

    def state(self):
        """the state block as a dict of ints (a read-back)"""
        from . import ops
        return dict(zip(ops.EVAL_STATE, self.buffers["state"].cpu().tolist()))

    def eval_list(self):
        """-> (dict(mpjpe, score, gt_id), total_gt) as numpy, like ``match_predictions``: the one read-back of a Panoptic run"""
        if self.kind != "panoptic":
            raise ValueError("DeviceEvaluator: eval_list belongs to kind 'panoptic'")
        st = self.state()
        if st["overflow"]:
            raise RuntimeError("DeviceEvaluator: %d entries do not fit capacity %d; build it with capacity >= %d"
                               % (st["n_entries"], self.capacity, st["n_entries"]))
        n = st["n_entries"]
        return {k: self.buffers[k][:n].cpu().numpy() for k in ("mpjpe", "score", "gt_id")}, st["total_gt"]

    def panoptic(self, method="score_sort"):
        """the tuple of ``evaluate_panoptic`` from the device's list"""
        if method == "mpjpe_sort":
            raise ValueError("DeviceEvaluator: mpjpe_sort de-duplicates per frame on the host; use evaluate_panoptic")
        ev, total_gt = self.eval_list()
        aps, recs = [], []
        for t in MPJPE_THRESHOLDS:
            ap, rec = eval_list_to_ap(ev, total_gt, t, method)
            aps.append(ap)
            recs.append(rec)
        return aps, recs, eval_list_to_mpjpe(ev, method=method), eval_list_to_recall(ev, total_gt)

    def pcp(self):
        """the tuple of ``evaluate_pcp`` from the device's counters; raises its ValueError for a frame that has an annotated actor
        and no prediction"""
        if self.kind != "pcp":
            raise ValueError("DeviceEvaluator: pcp belongs to kind 'pcp'")
        st = self.state()
        if st["empty_frame"]:
            raise ValueError(_NO_PREDICTION % (st["empty_frame"] - 1))
        f64 = lambda k: self.buffers[k].cpu().numpy().astype(np.float64)
        return _pcp_from_counters(f64("correct"), f64("total"), f64("bone_correct"), st["match_gt"], st["total_gt"])
