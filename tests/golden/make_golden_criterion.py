"""Training-criterion fixtures produced by RUNNING THE REFERENCE's own matcher and criterion on CPU.

Build container only (needs the reference tree, imported through ref_harness.load_reference(); nothing is copied):

    python -m tests.golden.make_golden_criterion

What runs, unmodified: ``HungarianMatcher`` (lib/models/matcher.py, methods KNN / multiple) on the initial query poses as
``dq_transformer.py:496-502`` calls it, and ``SetCriterion.forward`` (lib/models/multi_view_pose_transformer.py:810-932) once per
layer with that match (``outputs_origin``), under autograd for the gradients with respect to logits, 3D poses and 2D points.
Every case (tests/golden/criterion_cases.py) runs twice: in fp32 and, the fp64 column, with all inputs in double.  The reference
casts to ``torch.float`` / ``.float()`` in a dozen places; for the fp64 run those two names are pointed at float64 for the
duration of the call, so the same statements run in double.  Stored per case: a checksum of the inputs, the pair lists, every
loss and metric of every layer in both precisions, the three gradients in both precisions, and the crop affine the reference built.
The maker asserts that both precisions select the same pairs and that the cost margin around the selection is far above fp32
rounding.
"""
import contextlib
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden import criterion_cases as cc  # noqa: E402
from tests.golden.ref_harness import load_reference  # noqa: E402

KEYS = ("loss_ce", "class_error", "class_recall", "class_precision", "cardinality_error", "loss_pose_perjoint",
        "loss_pose_perprojection_2d")


@contextlib.contextmanager
def float_means(dtype):
    """inside: torch.float and Tensor.float() give `dtype` (the reference's hard-coded casts follow the run's precision)"""
    old = torch.float, torch.Tensor.float
    if dtype == torch.float64:
        torch.float = torch.float64
        torch.Tensor.float = lambda self, *a, **k: self.double()
    try:
        yield
    finally:
        torch.float, torch.Tensor.float = old


def run_case(mvpt, matcher_mod, transforms, name, dtype):
    c = cc.CASES[name]
    inp = cc.make_inputs(name)
    cfg = SimpleNamespace(
        MULTI_PERSON=SimpleNamespace(SPACE_SIZE=list(cc.SPACE_SIZE), SPACE_CENTER=list(cc.SPACE_CENTER)),
        NETWORK=SimpleNamespace(IMAGE_SIZE=list(cc.IMG_WH)),
        DECODER=SimpleNamespace(loss_joint_type="l1", use_loss_pose_perbone=False, use_loss_pose_perprojection=False,
                                use_loss_pose_perprojection_2d=True, loss_pose_normalize=False,
                                pred_conf_threshold=cc.PRED_CONF_THRESHOLD, num_instance=c["NQ"], use_ce_match=False))
    matcher = matcher_mod.HungarianMatcher(match_coord_est="abs", match_coord_gt="norm", cost_class=2.0, cost_pose=5.0,
                                           method=c["method"], method_value=c["value"])
    crit = mvpt.SetCriterion(2, matcher, {}, ["joints", "labels", "cardinality"], cfg, focal_alpha=0.25)
    if dtype == torch.float64:
        crit.double()
        for o in (crit, matcher):
            o.grid_size, o.grid_center = o.grid_size.double(), o.grid_center.double()
    res = {}
    with float_means(dtype):
        meta = cc.make_meta(inp, dtype=dtype)
        size = torch.tensor(cc.SPACE_SIZE, dtype=dtype)
        cen = torch.tensor(cc.SPACE_CENTER, dtype=dtype)
        meta[0]["joints_3d_norm"] = (meta[0]["joints_3d"] - cen + size / 2.0) / size      # dq_transformer.py:499-500
        init = torch.from_numpy(inp["init_poses"]).to(dtype)
        B, NQ = c["B"], c["NQ"]
        origin = {"pred_logits": torch.ones((B, NQ, 2), dtype=dtype), "pred_poses": {"outputs_coord": init}}
        pairs = matcher(origin, meta)
        # selection margin: the gap between the last selected and the first rejected cost of every person / query
        tgt = (meta[0]["joints_3d_norm"] * size + cen - size / 2.0).reshape(B, -1, cc.J * 3)
        cost = 0.01 * torch.cdist(init.reshape(B, NQ, -1), tgt, p=1)
        margin = np.inf
        for b in range(B):
            for g in range(int(inp["num_person"][b])):
                col = cost[b, :, g].sort()[0]
                if c["method"] == "KNN":
                    margin = min(margin, float(col[c["value"]] - col[c["value"] - 1]), float((col[1:c["value"]] - col[:c["value"] - 1]).min()))
            if c["method"] == "multiple" and int(inp["num_person"][b]):
                best = cost[b, :, :int(inp["num_person"][b])].min(-1)[0]
                margin = min(margin, float((best - c["value"]).abs().min()))
        res["margin"] = np.float64(margin)
        for b, (q, g) in enumerate(pairs):
            res["pairs/%d/query" % b] = q.numpy().astype(np.int64)
            res["pairs/%d/gt" % b] = g.numpy().astype(np.int64)
        logits = torch.from_numpy(inp["logits"]).to(dtype).requires_grad_(True)
        poses = torch.from_numpy(inp["poses"]).to(dtype).requires_grad_(True)
        poses_2d = torch.from_numpy(inp["poses_2d"]).to(dtype).requires_grad_(True)
        table = np.zeros((c["L"], len(KEYS)), np.float64)
        total = 0
        for l in range(c["L"]):
            out = {"pred_logits": logits[l], "pred_poses": {"outputs_coord": poses[l]},
                   "pred_poses_2d": {"outputs_coord_2d": poses_2d[l]}}
            losses, _ = crit(out, meta, origin)
            for i, k in enumerate(KEYS):
                table[l, i] = float(losses[k])
            total = total + losses["loss_ce"] + losses["loss_pose_perjoint"] + losses["loss_pose_perprojection_2d"]
        gl, gp, g2 = torch.autograd.grad(total, [logits, poses, poses_2d], allow_unused=True)
        res["table"] = table
        res["grad_logits"] = gl.numpy()
        res["grad_poses"] = np.zeros(poses.shape) if gp is None else gp.numpy()
        res["grad_poses_2d"] = np.zeros(poses_2d.shape) if g2 is None else g2.numpy()
        res["affine"] = np.asarray(transforms.get_affine_transform(inp["center"][0], inp["scale"][0], 0, list(cc.IMG_WH)), np.float64)
    res["checksum"] = cc.checksum(inp)
    return res


def main():
    load_reference()
    import models.multi_view_pose_transformer as mvpt
    import models.matcher as matcher_mod
    import utils.transforms as transforms
    out = {}
    for name in cc.CASES:
        r32 = run_case(mvpt, matcher_mod, transforms, name, torch.float32)
        r64 = run_case(mvpt, matcher_mod, transforms, name, torch.float64)
        shared = 0
        for k in r32:
            if k.startswith("pairs/"):
                assert np.array_equal(r32[k], r64[k]), (name, k)            # both precisions select the same pairs
                out["%s/%s" % (name, k)] = r64[k].astype(np.int32)
                if k.endswith("/query"):
                    shared += len(r64[k]) - len(np.unique(r64[k]))
        assert r64["margin"] > 1e-2, (name, r64["margin"])                  # costs ~1e2..1e3: fp32 rounding ~1e-4
        out[name + "/checksum"] = r64["checksum"]
        out[name + "/affine"] = r64["affine"]
        out[name + "/shared_queries"] = np.int64(shared)
        for k in ("table", "grad_logits", "grad_poses", "grad_poses_2d"):
            out["%s/%s/f64" % (name, k)] = r64[k]
            out["%s/%s/f32" % (name, k)] = r32[k].astype(np.float32)
        print(name, "margin %.3g shared %d" % (r64["margin"], shared))
        print("   f64", np.array2string(r64["table"], precision=6))
        print("   rel |f32 - f64|", np.array2string(np.abs(r32["table"] - r64["table"]) / np.maximum(np.abs(r64["table"]), 1e-30), precision=2))
    np.savez_compressed(os.path.join(HERE, "criterion.npz"), **out)
    print("criterion.npz %.0f KB" % (os.path.getsize(os.path.join(HERE, "criterion.npz")) / 1024))


if __name__ == "__main__":
    main()
