"""Joint-map fixtures of the training criterion (Shelf / Campus joint format), produced by RUNNING THE REFERENCE's own matcher and
criterion on CPU, in the manner of make_golden_criterion.py.

Build container only (needs the reference tree, imported through ref_harness.load_reference(); nothing is copied):

    python -m tests.golden.make_golden_criterion_jm

What runs, unmodified: ``construct_output_from_origin`` (lib/models/dq_transformer.py:90-104) on the UNconverted initial poses
with the case's ``convert_joint_format_indices``, ``HungarianMatcher`` (methods KNN / multiple) on its output, and
``SetCriterion.forward`` once per layer on predictions gathered exactly as ``dq_transformer.py:582-590`` gathers them -- view to
(…, NQ, 15, C), index ``[..., indices, :]``, flatten -- under autograd, so the stored gradients are with respect to the
UNconverted 15-joint tensors (zeros at joints the map does not name).  Every case (tests/golden/criterion_jm_cases.py) runs in
fp32 and in fp64 as in make_golden_criterion.py; both precisions must select the same pairs and the selection margin must be
above 1e-2.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from types import SimpleNamespace  # noqa: E402

from tests.golden import criterion_jm_cases as jc  # noqa: E402
from tests.golden.make_golden_criterion import KEYS, float_means  # noqa: E402
from tests.golden.ref_harness import load_reference  # noqa: E402


def run_case(mvpt, matcher_mod, dq, transforms, name, dtype):
    c = jc.CASES[name]
    jm = list(c["joint_map"])
    Jc = len(jm)
    inp = jc.make_inputs(name)
    cfg = SimpleNamespace(
        MULTI_PERSON=SimpleNamespace(SPACE_SIZE=list(jc.SPACE_SIZE), SPACE_CENTER=list(jc.SPACE_CENTER)),
        NETWORK=SimpleNamespace(IMAGE_SIZE=list(jc.IMG_WH)),
        DECODER=SimpleNamespace(loss_joint_type="l1", use_loss_pose_perbone=False, use_loss_pose_perprojection=False,
                                use_loss_pose_perprojection_2d=True, loss_pose_normalize=False,
                                pred_conf_threshold=jc.PRED_CONF_THRESHOLD, num_instance=c["NQ"], use_ce_match=False))
    matcher = matcher_mod.HungarianMatcher(match_coord_est="abs", match_coord_gt="norm", cost_class=2.0, cost_pose=5.0,
                                           method=c["method"], method_value=c["value"])
    crit = mvpt.SetCriterion(2, matcher, {}, ["joints", "labels", "cardinality"], cfg, focal_alpha=0.25)
    if dtype == torch.float64:
        crit.double()
        for o in (crit, matcher):
            o.grid_size, o.grid_center = o.grid_size.double(), o.grid_center.double()
    res = {}
    with float_means(dtype):
        meta = jc.make_meta(inp, dtype=dtype)
        size = torch.tensor(jc.SPACE_SIZE, dtype=dtype)
        cen = torch.tensor(jc.SPACE_CENTER, dtype=dtype)
        meta[0]["joints_3d_norm"] = (meta[0]["joints_3d"] - cen + size / 2.0) / size      # dq_transformer.py:499-500
        init = torch.from_numpy(inp["init_poses"]).to(dtype)                               # (B, NQ*15, 3), unconverted
        B, NQ = c["B"], c["NQ"]
        origin = dq.construct_output_from_origin(init, "cpu", num_joints=jc.JP, convert_joint_format_indices=jm)
        origin["pred_logits"] = origin["pred_logits"].to(dtype)
        conv = origin["pred_poses"]["outputs_coord"]
        assert tuple(conv.shape) == (B, NQ * Jc, 3) and conv.dtype == dtype
        pairs = matcher(origin, meta)
        tgt = (meta[0]["joints_3d_norm"] * size + cen - size / 2.0).reshape(B, -1, Jc * 3)
        cost = 0.01 * torch.cdist(conv.reshape(B, NQ, -1), tgt, p=1)
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
        poses = torch.from_numpy(inp["poses"]).to(dtype).requires_grad_(True)              # (L, B, NQ*15, 3)
        poses_2d = torch.from_numpy(inp["poses_2d"]).to(dtype).requires_grad_(True)        # (L, B, V, NQ*15, 2)
        table = np.zeros((c["L"], len(KEYS)), np.float64)
        total = 0
        for l in range(c["L"]):
            # dq_transformer.py:582-590
            oc = poses[l].view(B, NQ, jc.JP, -1)[..., jm, :].flatten(1, 2)
            nv = poses_2d[l].shape[1]
            oc2 = poses_2d[l].view(B, nv, NQ, jc.JP, -1)[..., jm, :].flatten(2, 3)
            out = {"pred_logits": logits[l], "pred_poses": {"outputs_coord": oc}, "pred_poses_2d": {"outputs_coord_2d": oc2}}
            losses, _ = crit(out, meta, origin)
            for i, k in enumerate(KEYS):
                table[l, i] = float(losses[k])
            total = total + losses["loss_ce"] + losses["loss_pose_perjoint"] + losses["loss_pose_perprojection_2d"]
        gl, gp, g2 = torch.autograd.grad(total, [logits, poses, poses_2d], allow_unused=True)
        res["table"] = table
        res["grad_logits"] = gl.numpy()
        res["grad_poses"] = np.zeros(poses.shape) if gp is None else gp.numpy()
        res["grad_poses_2d"] = np.zeros(poses_2d.shape) if g2 is None else g2.numpy()
        res["affine"] = np.asarray(transforms.get_affine_transform(inp["center"][0], inp["scale"][0], 0, list(jc.IMG_WH)), np.float64)
    res["checksum"] = jc.checksum(inp)
    return res


def main():
    load_reference()
    import models.dq_transformer as dq
    import models.matcher as matcher_mod
    import models.multi_view_pose_transformer as mvpt
    import utils.transforms as transforms
    out = {}
    for name in jc.CASES:
        r32 = run_case(mvpt, matcher_mod, dq, transforms, name, torch.float32)
        r64 = run_case(mvpt, matcher_mod, dq, transforms, name, torch.float64)
        shared = npairs = 0
        for k in r32:
            if k.startswith("pairs/"):
                assert np.array_equal(r32[k], r64[k]), (name, k)            # both precisions select the same pairs
                out["%s/%s" % (name, k)] = r64[k].astype(np.int32)
                if k.endswith("/query"):
                    shared += len(r64[k]) - len(np.unique(r64[k]))
                    npairs += len(r64[k])
        assert r64["margin"] > 1e-2, (name, r64["margin"])
        out[name + "/checksum"] = r64["checksum"]
        out[name + "/affine"] = r64["affine"]
        out[name + "/shared_queries"] = np.int64(shared)
        for k in ("table", "grad_logits", "grad_poses", "grad_poses_2d"):
            out["%s/%s/f64" % (name, k)] = r64[k]
            out["%s/%s/f32" % (name, k)] = r32[k].astype(np.float32)
        print(name, "margin %.3g pairs %d shared %d" % (r64["margin"], npairs, shared))
        print("   f64", np.array2string(r64["table"], precision=6))
        print("   rel |f32 - f64|", np.array2string(np.abs(r32["table"] - r64["table"]) / np.maximum(np.abs(r64["table"]), 1e-30), precision=2))
    np.savez_compressed(os.path.join(HERE, "criterion_jm.npz"), **out)
    print("criterion_jm.npz %.0f KB" % (os.path.getsize(os.path.join(HERE, "criterion_jm.npz")) / 1024))


if __name__ == "__main__":
    main()
