"""Time of the device NMS (ops.pose_nms) next to the host path (evaluate.filter_and_nms) at serving size, and what it adds to the
replayed decoder graph.

  1. ops.pose_nms at (1, 1024, 15) with ~10 % of the rows candidates (the regime a trained checkpoint lives in) and with every
     row a candidate: device time between events around the three launches, and host wall time to the synchronised result;
     evaluate.filter_and_nms on the same device tensor: host wall time including its copies.  Medians after warm-up.
  2. cfg-2 decoder (bf16, ~10 % valid queries) as serving.GraphedDecoder with and without postprocess: host wall time of
     replay() + synchronise, the two runners alternating in one process, plus the frame's read-back of the count.

    python tools/bench_nms.py [--reps 60] [--graph 1]
"""
import argparse
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from tests import nms_cases, nms_ref  # noqa: E402

DEV = "cuda:0"


def _median(xs):
    return "median %8.3f ms  min %8.3f  max %8.3f" % (statistics.median(xs), min(xs), max(xs))


def operator(reps, warm):
    from mvgformer_amd import evaluate as E
    from mvgformer_amd import ops
    for label, flagged in (("~10 % candidates", 0.9), ("100 % candidates", 0.0)):
        pred_np = nms_cases.scene(1024, 1124, 15, flagged)
        pred = torch.from_numpy(pred_np)[None].to(DEV)
        out = ops.pose_nms_buffers(1, 1024, 15, None, DEV)
        want = nms_ref.pose_nms(pred_np)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        dev_ms, wall_ms, host_ms = [], [], []
        for i in range(warm + reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev[0].record()
            keep, count, dets = ops.pose_nms(pred, out=out)
            ev[1].record()
            k = int(count[0, 0])                                     # the frame's read-back (synchronises)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            if i >= warm:
                dev_ms.append(ev[0].elapsed_time(ev[1]))
                wall_ms.append((t1 - t0) * 1e3)
        assert keep[0, :k].tolist() == want[0] and np.array_equal(dets[0, :k].cpu().numpy(), want[2])
        for i in range(warm + max(reps // 4, 10)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows = E.filter_and_nms(pred[0])
            torch.cuda.synchronize()
            if i >= warm:
                host_ms.append((time.perf_counter() - t0) * 1e3)
        assert torch.equal(rows, dets[0, :k])
        cand = int((pred_np[:, 0, 3] >= 0).sum())
        print("(1, 1024, 15) %-17s %4d candidates, %3d kept" % (label, cand, k))
        print("    ops.pose_nms, device time between events   %s  (%d reps)" % (_median(dev_ms), len(dev_ms)))
        print("    ops.pose_nms, host wall to the read count  %s" % _median(wall_ms))
        print("    evaluate.filter_and_nms, host wall         %s  (%d reps)" % (_median(host_ms), len(host_ms)))


def graph(reps, warm):
    from mvgformer_amd.factory import build_decoder_for_case, case_to_device
    from mvgformer_amd.serving import GraphedDecoder
    from mvgformer_amd.synthetic import build_case
    c = case_to_device(build_case("cfg2", seed=0, valid_fraction=0.1), DEV)
    dec = build_decoder_for_case(c, DEV, dtype=torch.bfloat16)
    runners = {}
    for name, pp in (("decoder graph", None), ("decoder + postprocess graph", dict(dist_thr=0.3, num_nearby_joints_thr=7))):
        r = GraphedDecoder(dec, c.meta, c.spatial_shapes, c.level_start_index, 1, c.NQ, 0.1, postprocess=pp)
        r.load(src_views=c.src_views, tgt=c.tgt, query_pos=c.query_pos, reference_points=c.reference_points).capture()
        runners[name] = r
    times = {k: [] for k in runners}
    times["decoder + postprocess graph + count read-back"] = []
    for i in range(warm + reps):
        for name, r in runners.items():                              # alternating in one process
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r.replay()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if i >= warm:
                times[name].append((t1 - t0) * 1e3)
            if r.detections is not None:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r.replay()
                k = int(r.detections[1][0, 0])
                t1 = time.perf_counter()
                if i >= warm:
                    times["decoder + postprocess graph + count read-back"].append((t1 - t0) * 1e3)
    post = runners["decoder + postprocess graph"]
    cand = int((post.pred[0, :, 0, 3] >= 0).sum())
    print("cfg2 bf16 valid10, replay() + synchronise, host wall (%d candidates, %d kept)" % (cand, k))
    for name, xs in times.items():
        print("    %-46s %s  (%d reps)" % (name, _median(xs), len(xs)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--graph", type=int, default=1)
    a = ap.parse_args()
    operator(a.reps, a.warmup)
    if a.graph:
        graph(a.reps, a.warmup)
