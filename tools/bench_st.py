"""Cost of structural triangulation on the device (ops.structural_triangulate, csrc/structural.hip; structural.StructuralRefiner).

  1. The launch alone at 10, 64 and 1024 persons (V = 5 views, J = 15, dense mode, 2 px of pixel noise, every person's own bone
     lengths), methods LS, ST with 1 step and ST with 3 steps: device time between events around the call, eager (two output
     allocations included) and as a replay of a HIP graph that holds only the launch.
  2. cfg-2 decoder (bf16, ~10 % valid queries) as serving.GraphedDecoder with postprocess, with and without refine=, alternating
     in one process: host wall time of replay + synchronise per frame, medians after warm-up.  The runner without refine is the
     behaviour without this feature.

    python tools/bench_st.py [--reps 200] [--warmup 20] [--out profiles/st_device.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda:0"
LINES = []
V, J = 5, 15


def say(text):
    print(text)
    LINES.append(text)


def _stats(xs):
    return "median %8.3f ms  min %8.3f  max %8.3f" % (statistics.median(xs), min(xs), max(xs))


def _timed(fn, reps, warm):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for i in range(warm + reps):
        torch.cuda.synchronize()
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        if i >= warm:
            ms.append(ev[0].elapsed_time(ev[1]))
    return ms


def launches(reps, warm):
    from mvgformer_amd import ops
    from mvgformer_amd.structural import PANOPTIC15_PARENT
    from tests.golden.st_cases import scene
    out = {}
    for n in (10, 64, 1024):
        sc = scene(n, V, PANOPTIC15_PARENT, persons=n, noise=2.0)
        ud = torch.from_numpy(np.ascontiguousarray(sc["ud"].transpose(1, 0, 2, 3).reshape(1, V, n * J, 2))).to(DEV)
        Pm = torch.from_numpy(sc["Pm"][None].copy()).to(DEV)
        lengths = torch.from_numpy(sc["bone_len"][None].copy()).to(DEV)
        for name, method, steps in (("LS ", "LS", 1), ("ST1", "ST", 1), ("ST3", "ST", 3)):
            call = lambda o=None: ops.structural_triangulate(ud, None, Pm, PANOPTIC15_PARENT, lengths, n_steps=steps,   # noqa: E731
                                                             method=method, out=o)
            eager = _timed(call, reps, warm)
            buf = ops.structural_buffers(1, n, J, DEV)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                call(buf)
            replay = _timed(graph.replay, reps, warm)
            solved = int((buf["status"] == 0).sum())
            say("    structural_triangulate %4d persons, V = %d, %s  eager %s   replay %s  (%d solved)"
                % (n, V, name, _stats(eager), _stats(replay), solved))
            out["launch_ms_replay_%s_%d" % (name.strip(), n)] = statistics.median(replay)
            out["launch_ms_eager_%s_%d" % (name.strip(), n)] = statistics.median(eager)
    return out


def frames(reps, warm):
    from mvgformer_amd.factory import build_decoder_for_case, case_to_device
    from mvgformer_amd.serving import GraphedDecoder
    from mvgformer_amd.synthetic import build_case
    c = case_to_device(build_case("cfg2", seed=0, valid_fraction=0.1), DEV)
    dec = build_decoder_for_case(c, DEV, dtype=torch.bfloat16)
    pp = dict(dist_thr=0.3, num_nearby_joints_thr=7)
    args = (dec, c.meta, c.spatial_shapes, c.level_start_index, 1, c.NQ, 0.1)
    plain = GraphedDecoder(*args, postprocess=pp)
    fine = GraphedDecoder(*args, postprocess=pp, refine=dict(bone_lengths=[250.0] * (J - 1), n_steps=1))
    for r in (plain, fine):
        r.load(src_views=c.src_views, tgt=c.tgt, query_pos=c.query_pos, reference_points=c.reference_points).capture()
    t_plain, t_fine = [], []
    for i in range(warm + reps):                                         # alternating in one process
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plain.replay()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        fine.replay()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if i >= warm:
            t_plain.append((t1 - t0) * 1e3)
            t_fine.append((t2 - t1) * 1e3)
    assert torch.equal(plain.detections[0], fine.detections[0])
    kept = int(fine.detections[1][0, 0])
    solved = int((fine.refined[1][0, :kept] == 0).sum())
    a, b = statistics.median(t_plain), statistics.median(t_fine)
    say("cfg2 bf16 valid10, replay + synchronise per frame, host wall (%d kept poses, %d solved)" % (kept, solved))
    say("    GraphedDecoder(postprocess)                  %s" % _stats(t_plain))
    say("    GraphedDecoder(postprocess, refine)          %s  (%d reps)" % (_stats(t_fine), len(t_fine)))
    say("      -> added by refine: %+.3f ms per frame, %.1f %% of a replay" % (b - a, 100.0 * (b - a) / b))
    return dict(frame_ms_plain=a, frame_ms_refine=b, kept=kept, solved=solved)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the printed lines to this file")
    a = ap.parse_args()
    res = frames(a.reps, a.warmup)
    res.update(launches(a.reps, a.warmup))
    say(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")
