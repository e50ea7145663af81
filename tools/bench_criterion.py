"""Time of match + criterion forward + backward at cfg-2 size (5 views, 1024 queries, 4 layers, B = 1, 5 persons, K = 5): the fused
kernels against tests/criterion_ref.py run in fp32 on the GPU as plain torch ops.  Median of the timed repetitions after warm-up,
wall clock around a device synchronisation (the torch composition synchronises on its own, the fused path does not)."""
import statistics
import sys
import time

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from tests import criterion_ref as R  # noqa: E402
from tests.golden import criterion_cases as cc  # noqa: E402


def main(reps=30, warm=5):
    from types import SimpleNamespace as NS
    from mvgformer_amd import ops
    from mvgformer_amd.criterion import KNNMatcher, SetCriterion, criterion_all_layers
    dev = "cuda:0"
    inp = cc.make_inputs(dict(B=1, NQ=1024, Gmax=10, num_person=[5], V=5, L=4, method="KNN", value=5, vis=True, scale2d=1.0, seed=2))
    meta = cc.make_meta(inp, dev)
    cams = ops.pack_cameras(meta, list(cc.IMG_WH), dev)
    cfg = NS(MULTI_PERSON=NS(SPACE_SIZE=list(cc.SPACE_SIZE), SPACE_CENTER=list(cc.SPACE_CENTER)), NETWORK=NS(IMAGE_SIZE=list(cc.IMG_WH)),
             DECODER=NS(pred_conf_threshold=cc.PRED_CONF_THRESHOLD, num_instance=1024))
    crit = SetCriterion(2, KNNMatcher("abs", "norm", method="KNN", method_value=5), {}, ["joints", "labels", "cardinality"], cfg)
    t, cam, aff = R.tensors_of(inp, torch.float32, dev)
    size, cen = torch.tensor(cc.SPACE_SIZE, device=dev), torch.tensor(cc.SPACE_CENTER, device=dev)
    lg, ps, p2 = (t[k].clone().requires_grad_(True) for k in ("logits", "poses", "poses_2d"))

    def fused():
        ld, _ = criterion_all_layers(crit, lg, ps, p2, meta, t["init_poses"], "none", cams)
        return torch.autograd.grad(ld["loss_ce"] + ld["loss_pose_perjoint"] + ld["loss_pose_perprojection_2d"], [lg, ps, p2])

    def composed():
        pairs = R.match(t["init_poses"], t["joints_3d"], t["num_person"], size, cen, "KNN", 5)
        total = 0
        for l in range(4):
            o = R.criterion_layer(lg[l], ps[l], p2[l], pairs, t["joints_3d"], t["joints_3d_vis"], t["joints_vis"], t["num_person"], cam,
                                  aff, size, cen, cc.PRED_CONF_THRESHOLD)
            total = total + o["loss_ce"] + o["loss_pose_perjoint"] + o["loss_pose_perprojection_2d"]
        return torch.autograd.grad(total, [lg, ps, p2])

    for name, fn in (("fused", fused), ("torch composition (fp32)", composed)):
        times = []
        for i in range(warm + reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= warm:
                times.append((time.perf_counter() - t0) * 1e3)
        print("%-28s median %.3f ms  min %.3f  max %.3f  (%d reps)" % (name, statistics.median(times), min(times), max(times), reps))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    dts = []
    for i in range(warm + reps):
        ev[0].record()
        fused()
        ev[1].record()
        torch.cuda.synchronize()
        if i >= warm:
            dts.append(ev[0].elapsed_time(ev[1]))
    print("fused, device time between events: median %.3f ms" % statistics.median(dts))


if __name__ == "__main__":
    main()
