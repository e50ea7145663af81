"""Per-frame cost of scoring a validation frame: on the host behind a read-back (what validate does with --device-eval 0) against
the evaluator inside the replayed graph (--device-eval 1), and the evaluator kernels' own device time.

  1. cfg-2 decoder (bf16, ~10 % valid queries, 5 ground-truth persons) as serving.GraphedDecoder, host wall time per frame, the
     two cases alternating in one process, medians after warm-up:
       (a) replay of the decoder + postprocess graph, the frame's read-back of the kept count, the clone of the kept rows, and
           evaluate.match_predictions on that frame (three .cpu() calls and a handful of fp64 tensor ops);
       (b) load of the frame's ground truth into the static inputs (three device copies), replay of the decoder + postprocess +
           evaluation graph, one synchronise.  Nothing is read back.
     The two lists are compared at the end.
  2. ops.eval_match at (1, 1024, 15) and ops.eval_pcp at (1, 1024, 14), device time between events around the call: with the
     rows one frame keeps, and with all 1024 rows taking part against 10 persons / 4 actors (the most work the shapes allow).

    python tools/bench_eval.py [--reps 200] [--warmup 20] [--out profiles/eval_device.txt]
"""
import argparse
import json
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from tests.golden.eval_cases import _person  # noqa: E402

DEV = "cuda:0"
LINES = []


def say(text):
    print(text)
    LINES.append(text)


def _stats(xs):
    return "median %8.3f ms  min %8.3f  max %8.3f" % (statistics.median(xs), min(xs), max(xs))


def _ground_truth(persons, J, seed=0):
    rng = np.random.default_rng(seed)
    gt = np.stack([_person(rng, J) for _ in range(persons)]).astype(np.float32)
    vis = np.ones((persons, J, 3), np.float32)
    dev = (torch.from_numpy(gt)[None].to(DEV), torch.ones((1, persons, J), device=DEV), torch.tensor([persons], dtype=torch.int32, device=DEV))
    return gt.astype(np.float64), vis, dev


def frames(reps, warm):
    from mvgformer_amd import evaluate as E
    from mvgformer_amd.factory import build_decoder_for_case, case_to_device
    from mvgformer_amd.serving import GraphedDecoder
    from mvgformer_amd.synthetic import build_case
    c = case_to_device(build_case("cfg2", seed=0, valid_fraction=0.1), DEV)
    dec = build_decoder_for_case(c, DEV, dtype=torch.bfloat16)
    gt, vis, gt_dev = _ground_truth(5, 15)
    pp = dict(dist_thr=0.3, num_nearby_joints_thr=7)
    host = GraphedDecoder(dec, c.meta, c.spatial_shapes, c.level_start_index, 1, c.NQ, 0.1, postprocess=pp)
    dev = GraphedDecoder(dec, c.meta, c.spatial_shapes, c.level_start_index, 1, c.NQ, 0.1, postprocess=pp,
                         evaluation=dict(kind="panoptic", capacity=(warm + reps) * c.NQ, max_persons=10))
    for r in (host, dev):
        r.load(src_views=c.src_views, tgt=c.tgt, query_pos=c.query_pos, reference_points=c.reference_points).capture()
    t_host, t_dev, t_replay, lists, k = [], [], [], [], 0
    for i in range(warm + reps):                                         # alternating in one process
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host.replay()
        dets, count, _ = host.detections
        kept = [dets[b, :k].clone() for b, k in enumerate(count[:, 0].tolist())]      # the frame's read-back
        t1 = time.perf_counter()
        lists.append(E.match_predictions(kept, [gt], [vis]))
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        dev.load(ground_truth=gt_dev).replay()
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        if i >= warm:
            t_replay.append((t1 - t0) * 1e3)
            t_host.append((t2 - t0) * 1e3)
            t_dev.append((t3 - t2) * 1e3)
        k = len(kept[0])
    got, total_gt = dev.evaluator.eval_list()
    want = {key: np.concatenate([l[0][key] for l in lists]) for key in got}
    assert total_gt == sum(l[1] for l in lists) and got["gt_id"].tolist() == (want["gt_id"] + 5 * np.repeat(np.arange(len(lists)), k)).tolist()
    assert np.array_equal(got["score"], want["score"]) and np.allclose(got["mpjpe"], want["mpjpe"], rtol=1e-12, atol=0)
    cand = int((dev.pred[0, :, 0, 3] >= 0).sum())
    say("cfg2 bf16 valid10, per frame, host wall (%d candidates, %d kept, 5 persons; lists equal over %d frames)" % (cand, k, len(lists)))
    say("    (a) replay + count read-back + clone of the kept rows              %s" % _stats(t_replay))
    say("    (a) ... + evaluate.match_predictions of the frame (parent's path)  %s  (%d reps)" % (_stats(t_host), len(t_host)))
    say("    (b) ground-truth load + replay with the evaluator + synchronise    %s  (%d reps)" % (_stats(t_dev), len(t_dev)))
    return dict(frame_ms_host_scoring=statistics.median(t_host), frame_ms_device_scoring=statistics.median(t_dev),
                frame_ms_replay_readback=statistics.median(t_replay), kept=k, candidates=cand)


def kernels(reps, warm, kept):
    from mvgformer_amd import ops
    out = {}
    rng = np.random.default_rng(1)
    for name, J, persons in (("eval_match", 15, 10), ("eval_pcp", 14, 4)):
        _, _, gt_dev = _ground_truth(persons, J)
        dets = torch.from_numpy(rng.normal(0, 1500.0, size=(1, 1024, J, 5)).astype(np.float32)).to(DEV)
        dets[..., 3] = 0.0
        for label, count in (("%d rows" % kept, torch.tensor([[kept, 0]], dtype=torch.int32, device=DEV)), ("1024 rows", None)):
            buffers = ops.eval_buffers((warm + reps) * 1024, persons, DEV)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ms = []
            for i in range(warm + reps):
                torch.cuda.synchronize()
                ev[0].record()
                getattr(ops, name)(dets, count, *gt_dev, buffers)
                ev[1].record()
                torch.cuda.synchronize()
                if i >= warm:
                    ms.append(ev[0].elapsed_time(ev[1]))
            say("    ops.%-10s (1, 1024, %d), %2d persons, %-9s device time between events  %s  (%d reps)"
                % (name, J, persons, label, _stats(ms), len(ms)))
            out["%s_ms_%s" % (name, label.replace(" ", "_"))] = statistics.median(ms)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the printed lines to this file")
    a = ap.parse_args()
    res = frames(a.reps, a.warmup)
    res.update(kernels(a.reps, a.warmup, max(res["kept"], 1)))
    say(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")
