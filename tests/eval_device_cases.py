"""Shared set-up of tests/test_eval_device_gpu.py: the scenes of tests/golden/eval_cases.py rounded to fp32, the host reference on
them, a numpy restatement of the PCP counters, and the preconditions that keep a tie from hiding a defect.  No GPU is needed to
build or to check a case (`python -m tests.eval_device_cases` prints the margins of every seed)."""
import functools

import numpy as np
import torch

from mvgformer_amd import evaluate as E
from tests.golden.eval_cases import panoptic_scene, pcp_scene

PANOPTIC_SEEDS = (11, 12)            # the seeds of tests/test_evaluate.py
PCP_SEEDS = (21, 22)
THRESHOLDS = tuple(E.MPJPE_THRESHOLDS) + (500,)


def round32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def mean_matrix(p, g, v):
    """(N, G) mean over the visible joints of the joint distances, fp64 numpy (NaN for a person without visible joint)"""
    d = np.sqrt(((p[:, None, :, :3] - g[None, :, :, :3]) ** 2).sum(-1))
    w = (v[..., 0] > 0).astype(np.float64)[None]
    with np.errstate(invalid="ignore"):
        return (d * w).sum(-1) / w.sum(-1)


def pad_rows(rows, R, J, filler_flag=-1.0):
    """kept rows (k, J, 5) -> dets (1, R, J, 5) fp32 and count (1, 2) int32 the way ops.pose_nms leaves them; filler_flag 0 makes
    the rows behind the count look like candidates, so that only `count` keeps them out"""
    rows = np.asarray(rows, np.float64).reshape(-1, J, 5)
    dets = np.zeros((1, R, J, 5), np.float32)
    dets[0, :, :, 3] = filler_flag
    dets[0, :len(rows)] = rows
    return torch.from_numpy(dets), torch.tensor([[len(rows), 0]], dtype=torch.int32)


def pad_ground_truth(gt, vis, G, J):
    """(g, J, 3) / (g, J, >= 1) -> joints_3d (1, G, J, 3), joints_3d_vis (1, G, J) fp32, num_person (1) int32"""
    g = len(gt)
    j3d, v = np.zeros((1, G, J, 3), np.float32), np.zeros((1, G, J), np.float32)
    if g:
        j3d[0, :g] = np.asarray(gt)[..., :3]
        v[0, :g] = np.asarray(vis)[..., 0]
    return torch.from_numpy(j3d), torch.from_numpy(v), torch.tensor([g], dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def panoptic_case(seed, J=15):
    """the scene in fp32-representable numbers, the rows the host filter + NMS keeps, the host list and the margins"""
    preds, gts, vis = panoptic_scene(seed, frames=6, J=J)
    preds, gts = [round32(p) for p in preds], [round32(g) for g in gts]
    kept = [E.filter_and_nms(torch.as_tensor(p)).numpy() for p in preds]
    ev, total_gt = E.match_predictions(kept, gts, vis)
    gap = np.inf
    for k, g, v in zip(kept, gts, vis):
        if len(g) > 1 and len(k):
            m = np.sort(mean_matrix(k, g, v), axis=1)
            gap = min(gap, float((m[:, 1] - m[:, 0]).min()))
    edge = min(float(np.abs(ev["mpjpe"] - t).min()) for t in THRESHOLDS)
    return dict(preds=preds, gts=gts, vis=vis, kept=kept, ev=ev, total_gt=total_gt, best_gap=gap, threshold_gap=edge,
                metrics=E.evaluate_panoptic(kept, gts, vis))


def pcp_counters(kept, actor_gts, recall_threshold=500.0, alpha=0.5):
    """shelf.py:255-330 in numpy: the counters evaluate_pcp keeps to itself, and the smallest margins met on the way"""
    A = len(actor_gts)
    correct, total, bones = np.zeros(A, np.int64), np.zeros(A, np.int64), np.zeros((A, 10), np.int64)
    match_gt = total_gt = 0
    row_gap = limb_gap = recall_gap = np.inf
    for f, rows in enumerate(kept):
        p = np.asarray(rows, np.float64)
        p = p[p[:, 0, 3] >= 0][:, :, :3]
        for a in range(A):
            g = actor_gts[a][f]
            if g is None:
                continue
            m = np.sqrt(((g[None] - p) ** 2).sum(-1)).mean(-1)
            n = int(np.argmin(m))
            if len(m) > 1:
                s = np.sort(m)
                row_gap = min(row_gap, float(s[1] - s[0]))
            recall_gap = min(recall_gap, abs(float(m[n]) - recall_threshold))
            match_gt += int(m[n] < recall_threshold)
            total_gt += 1
            best = p[n]
            for k, (i, j) in enumerate(E.PCP_LIMBS):
                err = (np.linalg.norm(best[i] - g[i]) + np.linalg.norm(best[j] - g[j])) / 2.0
                lim = alpha * np.linalg.norm(g[i] - g[j])
                limb_gap = min(limb_gap, abs(float(err - lim)))
                bones[a, k] += int(err <= lim)
            p_hip, g_hip = (best[2] + best[3]) / 2.0, (g[2] + g[3]) / 2.0
            err = (np.linalg.norm(p_hip - g_hip) + np.linalg.norm(best[12] - g[12])) / 2.0
            lim = alpha * np.linalg.norm(g_hip - g[12])
            limb_gap = min(limb_gap, abs(float(err - lim)))
            bones[a, 9] += int(err <= lim)
            total[a] += 10
        correct = bones.sum(1)
    return dict(correct=correct, total=total, bone_correct=bones, match_gt=match_gt, total_gt=total_gt, row_gap=row_gap,
                limb_gap=limb_gap, recall_gap=recall_gap)


@functools.lru_cache(maxsize=None)
def pcp_case(seed):
    preds, actors, _, _ = pcp_scene(seed)
    preds = [round32(p) for p in preds]
    actors = [[None if g is None else round32(g) for g in a] for a in actors]
    kept = [E.filter_and_nms(torch.as_tensor(p)).numpy() for p in preds]
    return dict(preds=preds, actors=actors, kept=kept, host=E.evaluate_pcp(kept, actors), counters=pcp_counters(kept, actors),
                host_unfiltered=E.evaluate_pcp(preds, actors), counters_unfiltered=pcp_counters(preds, actors))


def pad_ground_truth_pcp(actors, f):
    """frame f of evaluate_pcp's actor_gts in the device layout: slot a is actor a, visibility 1 where it is annotated"""
    A = len(actors)
    j3d, vis = np.zeros((1, A, 14, 3), np.float32), np.zeros((1, A, 14), np.float32)
    for a in range(A):
        if actors[a][f] is not None:
            j3d[0, a], vis[0, a] = actors[a][f], 1.0
    return torch.from_numpy(j3d), torch.from_numpy(vis), torch.tensor([A], dtype=torch.int32)


def flat_pcp(result):
    actor, avg, bones, recall = result
    return np.concatenate([np.asarray(actor), [avg, recall], np.concatenate([np.asarray(v) for v in bones.values()])])


def flat_panoptic(result):
    aps, recs, mpjpe, rec500 = result
    return np.asarray(list(aps) + list(recs) + [mpjpe, rec500])


if __name__ == "__main__":
    import os
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "eval.npz"))
    for s in PANOPTIC_SEEDS:
        for J in (15, 14):
            c = panoptic_case(s, J)
            print("panoptic", s, "J", J, "entries", len(c["ev"]["mpjpe"]), "total_gt", c["total_gt"], "best gap %.3g" % c["best_gap"],
                  "threshold gap %.3g" % c["threshold_gap"], "kept", [len(k) for k in c["kept"]])
        c = panoptic_case(s)
        print("   vs golden (AP, recall, recall500):", np.abs(np.delete(flat_panoptic(c["metrics"]), 12) - np.delete(gold["pan_%d_nms" % s], 12)).max())
    for s in PCP_SEEDS:
        c = pcp_case(s)
        k = c["counters"]
        print("pcp", s, "row gap %.3g limb gap %.3g recall gap %.3g" % (k["row_gap"], k["limb_gap"], k["recall_gap"]),
              "restatement vs host", np.abs(flat_pcp(E._pcp_from_counters(k["correct"].astype(float), k["total"].astype(float),
                                                                           k["bone_correct"].astype(float), k["match_gt"], k["total_gt"]))
                                            - flat_pcp(c["host"])).max(),
              "unfiltered vs golden", np.abs(flat_pcp(c["host_unfiltered"]) - gold["pcp_%d" % s]).max(),
              "unfiltered gaps", [c["counters_unfiltered"][k] for k in ("row_gap", "limb_gap", "recall_gap")], "kept", [len(x) for x in c["kept"]],
              "cands", [int((p[:, 0, 3] >= 0).sum()) for p in c["preds"]])
