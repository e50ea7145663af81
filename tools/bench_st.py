"""Cost of structural triangulation on the device (ops.structural_triangulate, csrc/structural.hip; structural.StructuralRefiner).

  1. The launch alone at 10, 64 and 1024 persons (V = 5 views, J = 15, dense mode, 2 px of pixel noise, every person's own bone
     lengths), methods LS, ST with 1 step and ST with 3 steps: device time between events around the call, eager (two output
     allocations included) and as a replay of a HIP graph that holds only the launch.
  2. cfg-2 decoder (bf16, ~10 % valid queries) as serving.GraphedDecoder with postprocess, with and without refine=, alternating
     in one process: host wall time of replay + synchronise per frame, medians after warm-up.  The runner without refine is the
     behaviour without this feature.
  3. With --track-lengths 1 instead: the per-track bone-length estimator (ops.track_bones, csrc/bones.hip) -- its launch alone as a
     replay of a graph that holds only the launch (T = 32, R = 1024, B = 1 and 8, W = 8 and 32), the cfg-2 replay with refine on
     track lengths against refine on given lengths (both behind the tracker, alternating), and the synthetic LS / ST table for
     W = 4, 8, 16 (numpy restatements on the CPU).

    python tools/bench_st.py [--reps 200] [--warmup 20] [--out profiles/st_device.txt]
    python tools/bench_st.py --track-lengths 1 --out profiles/track_bones.txt
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


def bones_launches(reps, warm):
    """mvg_track_bones alone, as a replay of a graph that holds only the launch: T = 32 slots, R = 1024 rows of which 10 are
    tracked detections whose rings are full, no fallback"""
    from mvgformer_amd import ops
    from mvgformer_amd.structural import PANOPTIC15_PARENT
    from tests.bones_cases import posed
    out = {}
    T, R, n = 32, 1024, 10
    for B in (1, 8):
        for W in (8, 32):
            rng = np.random.default_rng(B * 100 + W)
            dets = np.zeros((B, R, J, 5), np.float32)
            dets[..., 3] = -1.0
            for b in range(B):
                for i in range(n):
                    dets[b, i, :, :3] = posed(rng, PANOPTIC15_PARENT, rng.uniform(150.0, 450.0, J - 1), rng.normal(0, 800, 3))
                    dets[b, i, :, 3] = 1.0
            d = torch.from_numpy(dets).to(DEV)
            count = torch.tensor([[n, 0]] * B, dtype=torch.int32, device=DEV)
            track = ops.track_buffers(B, T, J, R, DEV)
            track["slots"][:, :n] = torch.arange(n, dtype=torch.int32, device=DEV)
            track["id"][:, :n] = torch.arange(n, dtype=torch.int32, device=DEV)
            buf = ops.track_bones_buffers(B, T, J, R, W, DEV)
            call = lambda: ops.track_bones(d, count, track, PANOPTIC15_PARENT, buf, 4, None)      # noqa: E731
            for _ in range(W + 1):
                call()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                call()
            replay = _timed(graph.replay, reps, warm)
            assert int((buf["row_source"] == 0).sum()) == B * n
            say("    track_bones B = %d, T = %d, R = %d, W = %2d, %d tracked rows per stream   replay %s"
                % (B, T, R, W, n, _stats(replay)))
            out["bones_launch_ms_replay_B%d_W%d" % (B, W)] = statistics.median(replay)
    return out


def frames_track(reps, warm):
    """cfg-2 replay with refine under per-track lengths against refine under the lengths of a file, both behind the tracker"""
    from mvgformer_amd.factory import build_decoder_for_case, case_to_device
    from mvgformer_amd.serving import GraphedDecoder
    from mvgformer_amd.synthetic import build_case
    c = case_to_device(build_case("cfg2", seed=0, valid_fraction=0.1), DEV)
    dec = build_decoder_for_case(c, DEV, dtype=torch.bfloat16)
    pp = dict(dist_thr=0.3, num_nearby_joints_thr=7)
    args = (dec, c.meta, c.spatial_shapes, c.level_start_index, 1, c.NQ, 0.1)
    tracking = dict(max_tracks=32)
    out = {}
    for W in (8, 32):
        filed = GraphedDecoder(*args, postprocess=pp, tracking=tracking, refine=dict(bone_lengths=[250.0] * (J - 1), n_steps=1))
        tracked = GraphedDecoder(*args, postprocess=pp, tracking=tracking,
                                 refine=dict(bone_lengths="track", window=W, min_frames=4, n_steps=1))
        for r in (filed, tracked):
            r.load(src_views=c.src_views, tgt=c.tgt, query_pos=c.query_pos, reference_points=c.reference_points).capture()
        t_file, t_track = [], []
        for i in range(warm + reps):                                     # alternating in one process
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            filed.replay()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            tracked.replay()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if i >= warm:
                t_file.append((t1 - t0) * 1e3)
                t_track.append((t2 - t1) * 1e3)
        assert torch.equal(filed.detections[0], tracked.detections[0]) and torch.equal(filed.track_ids[0], tracked.track_ids[0])
        kept = int(tracked.detections[1][0, 0])
        own = int((tracked.bone_source[0, :kept] == 0).sum())
        solved = int((tracked.refined[1][0, :kept] == 0).sum())
        a, b = statistics.median(t_file), statistics.median(t_track)
        say("cfg2 bf16 valid10, replay + synchronise per frame, host wall, W = %d (%d kept poses, %d on their track's lengths, "
            "%d solved)" % (W, kept, own, solved))
        say("    GraphedDecoder(postprocess, tracking, refine on given lengths)   %s" % _stats(t_file))
        say("    GraphedDecoder(postprocess, tracking, refine on track lengths)   %s  (%d reps)" % (_stats(t_track), len(t_track)))
        say("      -> added by the estimator: %+.3f ms per frame, %.2f %% of a replay" % (b - a, 100.0 * (b - a) / b))
        out.update({"frame_ms_refine_file_W%d" % W: a, "frame_ms_refine_track_W%d" % W: b})
    return out


def synthetic_table():
    """the statement the stage is built on, on the CPU with the numpy restatements (tests/bones_cases.study): LS poses as samples,
    uniform view weights, synthetic scenes -- no statement about a dataset"""
    from tests.bones_cases import study
    say("4 persons with fixed bones of 150-450 mm, a fresh pose per frame, 2 px noise, uniform weights; LS poses are the samples;")
    say("one ST step under the median of the last W frames; mean over 4 scored frames (numpy restatements, CPU)")
    say("    V  seed   W   bone residual vs TRUE lengths, mm: LS -> ST      mean joint error, mm: LS -> ST")
    out = {}
    for W in (4, 8, 16):
        for views in (3, 5):
            for seed in (0, 1, 2):
                r = study(seed, views, W=W, persons=4, noise=2.0)
                say("    %d   %d    %2d        %6.2f -> %5.2f                                 %6.2f -> %5.2f"
                    % (views, seed, W, r["ls_bone_mm"], r["st_bone_mm"], r["ls_joint_mm"], r["st_joint_mm"]))
                out["study_V%d_s%d_W%d" % (views, seed, W)] = [round(r[k], 3) for k in ("ls_bone_mm", "st_bone_mm", "ls_joint_mm",
                                                                                         "st_joint_mm")]
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the printed lines to this file")
    ap.add_argument("--track-lengths", type=int, default=0, choices=[0, 1],
                    help="1: the per-track bone-length estimator instead (ops.track_bones): its launch alone, the cfg-2 replay with "
                         "refine on track lengths against refine on given lengths, and the synthetic LS / ST table")
    a = ap.parse_args()
    if a.track_lengths:
        res = bones_launches(a.reps, a.warmup)
        res.update(frames_track(a.reps, a.warmup))
        res.update(synthetic_table())
    else:
        res = frames(a.reps, a.warmup)
        res.update(launches(a.reps, a.warmup))
    say(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")
