"""Cost of person tracking on the device (tracking.PoseTracker, csrc/track.hip) at the cfg-2 serving shapes (R = 1024, J = 15,
max_tracks = 32).

  1. PoseTracker.update with 4, 10 and 64 detections in steady state (every track is matched in every frame: two detection sets
     20 mm apart alternate, so the solver has real costs to work on; with 64 detections and 32 slots the other 32 overflow, and
     one more line gives 64 detections on 64 slots, the largest solve), device time between events around the call: eager, and
     as a replay of a HIP graph that holds only the update.  ops.linear_assignment on one random 64 x 64 problem next to it.
  2. cfg-2 decoder (bf16, ~10 % valid queries) as serving.GraphedDecoder with postprocess, with and without tracking=, alternating
     in one process: host wall time of replay + synchronise per frame, medians after warm-up.  The runner without tracking is the
     behaviour without this feature.

    python tools/bench_track.py [--reps 200] [--warmup 20] [--out profiles/track_device.txt]

``--motion 1`` measures the constant-velocity motion model instead (PoseTracker(motion=True): predict + update + correct), each
time against the motion-free path in the same process: the update of 1. with 4, 10 and 64 detections, eager and replayed, and
the cfg-2 replay of 2. with tracking= against tracking= plus motion.

    python tools/bench_track.py --motion 1 [--reps 200] [--warmup 20] [--out profiles/track_motion.txt]

``--eval 1`` measures the tracking scores (tracking.TrackEvaluator, mvg_track_eval): its update alone with 4, 10 and 64 persons,
eager and replayed; the cfg-2 replay with tracking= against tracking= plus track_evaluation=, alternating; and it runs seeded
SYNTHETIC detection-level sequences (walkers with a mid-sequence occlusion, two people crossing) through tracker + scorer with
the motion model off and on and prints MOTA / MOTP / IDF1 / switches for both.

    python tools/bench_track.py --eval 1 --reps 20 [--warmup 20] [--out profiles/track_eval.txt]
"""
import argparse
import json
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))

DEV = "cuda:0"
LINES = []
R, J = 1024, 15


def say(text):
    print(text)
    LINES.append(text)


def _stats(xs):
    return "median %8.3f ms  min %8.3f  max %8.3f" % (statistics.median(xs), min(xs), max(xs))


def _detections(n, seed=0):
    """two frames of n persons 2 m apart on a grid, the second moved by 20 mm and re-noised -> (dets (2, 1, R, J, 5), count)"""
    rng = np.random.default_rng(seed)
    skel = rng.uniform(-300.0, 300.0, size=(n, J, 3))
    centre = np.array([[2000.0 * (k % 8), 2000.0 * (k // 8), 900.0] for k in range(n)])[:, None, :]
    dets = np.zeros((2, 1, R, J, 5), np.float32)
    dets[..., 3] = -1.0
    for f in range(2):
        dets[f, 0, :n, :, :3] = centre + 20.0 * f + skel + rng.normal(scale=5.0, size=(n, J, 3))
        dets[f, 0, :n, :, 3] = 0.0
        dets[f, 0, :n, :, 4] = np.linspace(0.9, 0.3, n)[:, None]
    return torch.from_numpy(dets).to(DEV), torch.tensor([[n, 0]], dtype=torch.int32, device=DEV)


def _timed(fn, before, reps, warm):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for i in range(warm + reps):
        before(i)
        torch.cuda.synchronize()
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        if i >= warm:
            ms.append(ev[0].elapsed_time(ev[1]))
    return ms


def updates(reps, warm):
    from mvgformer_amd import ops
    from mvgformer_amd.tracking import PoseTracker
    out = {}
    for n, slots in ((4, 32), (10, 32), (64, 32), (64, 64)):
        frames, count = _detections(n)
        dets = frames[0].clone()
        tracker = PoseTracker(batch=1, rows=R, num_joints=J, max_tracks=slots, device=DEV)
        feed = lambda i: dets.copy_(frames[i % 2])                                   # noqa: E731
        eager = _timed(lambda: tracker.update(dets, count), feed, reps, warm)
        st = tracker.state()
        assert st["births"] == min(n, slots) and st["deaths"] == 0 and st["matches"] == min(n, slots) * (warm + reps - 1), st
        tracker.reset()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            tracker.update(dets, count)
        replay = _timed(graph.replay, feed, reps, warm)
        st = tracker.state()
        assert st["births"] == min(n, slots) and st["matches"] == min(n, slots) * (warm + reps - 1), st
        say("    PoseTracker.update (1, %d, %d), %2d slots, %2d detections  eager   %s" % (R, J, slots, n, _stats(eager)))
        say("                                                            replay  %s  (%d reps)" % (_stats(replay), len(replay)))
        out["update_ms_eager_%d_of_%d" % (n, slots)] = statistics.median(eager)
        out["update_ms_replay_%d_of_%d" % (n, slots)] = statistics.median(replay)
    cost = torch.from_numpy(np.random.default_rng(1).uniform(0.0, 1000.0, size=(1, 64, 64))).to(DEV)
    ms = _timed(lambda: ops.linear_assignment(cost), lambda i: None, reps, warm)
    say("    ops.linear_assignment (1, 64, 64) random costs, eager (two output allocations included)  %s" % _stats(ms))
    out["linear_assignment_ms_64"] = statistics.median(ms)
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
    track = GraphedDecoder(*args, postprocess=pp, tracking=dict(max_tracks=32))
    for r in (plain, track):
        r.load(src_views=c.src_views, tgt=c.tgt, query_pos=c.query_pos, reference_points=c.reference_points).capture()
    t_plain, t_track = [], []
    for i in range(warm + reps):                                         # alternating in one process
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plain.replay()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        track.replay()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if i >= warm:
            t_plain.append((t1 - t0) * 1e3)
            t_track.append((t2 - t1) * 1e3)
    assert torch.equal(plain.detections[0], track.detections[0])
    kept = int(track.detections[1][0, 0])
    st = track.tracker.state()
    assert st["frames"] == warm + reps and st["births"] == min(kept, 32)
    say("cfg2 bf16 valid10, replay + synchronise per frame, host wall (%d kept poses, %d tracks)" % (kept, st["active"]))
    say("    GraphedDecoder(postprocess)                  %s" % _stats(t_plain))
    say("    GraphedDecoder(postprocess, tracking)        %s  (%d reps)" % (_stats(t_track), len(t_track)))
    return dict(frame_ms_plain=statistics.median(t_plain), frame_ms_tracking=statistics.median(t_track), kept=kept)


def motion_updates(reps, warm):
    """PoseTracker.update without and with the motion model (predict + update + correct), the same detections, one process"""
    from mvgformer_amd.tracking import PoseTracker
    out = {}
    for n, slots in ((4, 32), (10, 32), (64, 64)):
        frames, count = _detections(n)
        dets = frames[0].clone()
        feed = lambda i: dets.copy_(frames[i % 2])                                   # noqa: E731
        med = {}
        for motion in (None, True, None, True):                                      # each twice, interleaved
            tracker = PoseTracker(batch=1, rows=R, num_joints=J, max_tracks=slots, device=DEV, motion=motion)
            eager = _timed(lambda: tracker.update(dets, count), feed, reps, warm)
            st = tracker.state()
            assert st["births"] == n and st["deaths"] == 0 and st["matches"] == n * (warm + reps - 1), st
            tracker.reset()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                tracker.update(dets, count)
            replay = _timed(graph.replay, feed, reps, warm)
            st = tracker.state()
            assert st["births"] == n and st["matches"] == n * (warm + reps - 1), st
            name = "motion" if motion else "plain "
            say("    PoseTracker.update (1, %d, %d), %2d slots, %2d detections, %s  eager   %s" % (R, J, slots, n, name, _stats(eager)))
            say("                                                                    replay  %s  (%d reps)"
                % (_stats(replay), len(replay)))
            med.setdefault((name.strip(), "eager"), []).append(statistics.median(eager))
            med.setdefault((name.strip(), "replay"), []).append(statistics.median(replay))
        for how in ("eager", "replay"):
            plain, motion = min(med[("plain", how)]), min(med[("motion", how)])
            say("      -> %2d of %2d %-6s  added by the motion model: %+.3f ms per frame (%.3f -> %.3f, the lower median of two passes)"
                % (n, slots, how, motion - plain, plain, motion))
            out["update_ms_%s_%d_of_%d" % (how, n, slots)] = plain
            out["update_ms_%s_motion_%d_of_%d" % (how, n, slots)] = motion
    return out


def motion_frames(reps, warm):
    """cfg-2 GraphedDecoder replay with tracking= against tracking= plus motion, alternating in one process"""
    from mvgformer_amd.factory import build_decoder_for_case, case_to_device
    from mvgformer_amd.serving import GraphedDecoder
    from mvgformer_amd.synthetic import build_case
    c = case_to_device(build_case("cfg2", seed=0, valid_fraction=0.1), DEV)
    dec = build_decoder_for_case(c, DEV, dtype=torch.bfloat16)
    pp = dict(dist_thr=0.3, num_nearby_joints_thr=7)
    args = (dec, c.meta, c.spatial_shapes, c.level_start_index, 1, c.NQ, 0.1)
    track = GraphedDecoder(*args, postprocess=pp, tracking=dict(max_tracks=32))
    motion = GraphedDecoder(*args, postprocess=pp, tracking=dict(max_tracks=32, motion=True))
    for r in (track, motion):
        r.load(src_views=c.src_views, tgt=c.tgt, query_pos=c.query_pos, reference_points=c.reference_points).capture()
    t_track, t_motion = [], []
    for i in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        track.replay()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        motion.replay()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if i >= warm:
            t_track.append((t1 - t0) * 1e3)
            t_motion.append((t2 - t1) * 1e3)
    assert torch.equal(track.detections[0], motion.detections[0]) and torch.equal(track.track_ids[0], motion.track_ids[0])
    kept = int(motion.detections[1][0, 0])
    st = motion.tracker.state()
    assert st["frames"] == warm + reps and st == track.tracker.state()
    say("cfg2 bf16 valid10, replay + synchronise per frame, host wall (%d kept poses, %d tracks)" % (kept, st["active"]))
    say("    GraphedDecoder(postprocess, tracking)          %s" % _stats(t_track))
    say("    GraphedDecoder(postprocess, tracking + motion) %s  (%d reps)" % (_stats(t_motion), len(t_motion)))
    say("      -> added by the motion model: %+.3f ms per frame" % (statistics.median(t_motion) - statistics.median(t_track)))
    return dict(frame_ms_tracking=statistics.median(t_track), frame_ms_tracking_motion=statistics.median(t_motion), kept=kept)


def eval_launches(reps, warm):
    """TrackEvaluator.update alone behind a tracker that has seen the frame: 4, 10 and 64 persons, each with a detection 5 mm off"""
    from mvgformer_amd.tracking import PoseTracker, TrackEvaluator
    out = {}
    for n in (4, 10, 64):
        frames, count = _detections(n)
        dets = frames[0].clone()
        tracker = PoseTracker(batch=1, rows=R, num_joints=J, max_tracks=64, device=DEV)
        tracker.update(dets, count)
        scorer = TrackEvaluator(batch=1, max_persons=64, max_ids=1024, device=DEV)
        j3d = dets[:, :64, :, :3].contiguous()
        vis = torch.ones((1, 64, J), device=DEV)
        num = torch.tensor([n], dtype=torch.int32, device=DEV)
        run = lambda: scorer.update(tracker, dets, count, j3d, vis, num)           # noqa: E731
        eager = _timed(run, lambda i: None, reps, warm)
        st = scorer.state()
        assert st["matches"] == n * (warm + reps) and st["kept"] == n * (warm + reps - 1) and st["misses"] == 0, st
        scorer.reset()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            run()
        replay = _timed(graph.replay, lambda i: None, reps, warm)
        assert scorer.state()["matches"] == n * (warm + reps)
        say("    TrackEvaluator.update (1, %d, %d), 64 identities, %2d persons and hypotheses  eager   %s" % (R, J, n, _stats(eager)))
        say("                                                                            replay  %s  (%d reps)"
            % (_stats(replay), len(replay)))
        out["eval_ms_eager_%d" % n] = statistics.median(eager)
        out["eval_ms_replay_%d" % n] = statistics.median(replay)
    return out


def eval_frames(reps, warm):
    """cfg-2 GraphedDecoder replay with tracking= (the behaviour without this feature) against tracking= plus track_evaluation=,
    alternating in one process"""
    from mvgformer_amd.factory import build_decoder_for_case, case_to_device
    from mvgformer_amd.serving import GraphedDecoder
    from mvgformer_amd.synthetic import build_case
    c = case_to_device(build_case("cfg2", seed=0, valid_fraction=0.1), DEV)
    dec = build_decoder_for_case(c, DEV, dtype=torch.bfloat16)
    pp = dict(dist_thr=0.3, num_nearby_joints_thr=7)
    args = (dec, c.meta, c.spatial_shapes, c.level_start_index, 1, c.NQ, 0.1)
    track = GraphedDecoder(*args, postprocess=pp, tracking=dict(max_tracks=32))
    scored = GraphedDecoder(*args, postprocess=pp, tracking=dict(max_tracks=32), track_evaluation=dict(max_persons=10))
    for r in (track, scored):
        r.load(src_views=c.src_views, tgt=c.tgt, query_pos=c.query_pos, reference_points=c.reference_points).capture()
    track.replay()
    torch.cuda.synchronize()
    G = min(int(track.detections[1][0, 0]), 10)                          # the ground truth: the first kept poses themselves
    scored.load(ground_truth=(track.detections[0][:, :G, :, :3].clone(), torch.ones((1, G, J), device=DEV),
                              torch.tensor([G], dtype=torch.int32, device=DEV)))
    t_track, t_scored = [], []
    for i in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        track.replay()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        scored.replay()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if i >= warm:
            t_track.append((t1 - t0) * 1e3)
            t_scored.append((t2 - t1) * 1e3)
    assert torch.equal(track.detections[0], scored.detections[0]) and torch.equal(track.track_ids[0], scored.track_ids[0])
    st = scored.track_evaluator.state()
    assert st["frames"] == warm + reps and st["matches"] == G * (warm + reps), st
    say("cfg2 bf16 valid10, replay + synchronise per frame, host wall (%d persons, all matched in every frame)" % G)
    say("    GraphedDecoder(postprocess, tracking)                    %s" % _stats(t_track))
    say("    GraphedDecoder(postprocess, tracking, track_evaluation)  %s  (%d reps)" % (_stats(t_scored), len(t_scored)))
    say("      -> added by the scoring: %+.3f ms per frame" % (statistics.median(t_scored) - statistics.median(t_track)))
    return dict(frame_ms_tracking=statistics.median(t_track), frame_ms_tracking_eval=statistics.median(t_scored), persons=G)


def _synthetic(kind, seeds, n_frames=60, noise=20.0):
    """seeded detection-level sequences, one stream per seed -> (dets (F, B, 16, J, 5), count (F, B, 2), truth (F, B, G, J, 3), G).
    'occlusion': four walkers 2.5 m apart at 70 mm a frame; walker 0 is undetected for 8 frames (fewer than max_misses = 10, but
    560 mm of travel: more than max_dist), walker 1 for 14 frames (more than max_misses), mid-sequence.  'crossing': two people
    walk towards each other at 60 mm a frame on lanes 150 mm apart and pass in the middle of the sequence."""
    B, rows = len(seeds), 16
    G = 4 if kind == "occlusion" else 2
    dets = np.zeros((n_frames, B, rows, J, 5), np.float32)
    dets[..., 3] = -1.0
    count = np.zeros((n_frames, B, 2), np.int32)
    truth = np.zeros((n_frames, B, G, J, 3), np.float32)
    for b, seed in enumerate(seeds):
        rng = np.random.default_rng(seed)
        skel = rng.uniform(-300.0, 300.0, size=(G, J, 3))
        if kind == "occlusion":
            start = np.array([[2500.0 * k, 0.0, 900.0] for k in range(G)])
            angle = rng.uniform(0.0, 2.0 * np.pi, size=G)
            vel = 70.0 * np.stack([np.cos(angle), np.sin(angle), np.zeros(G)], axis=1)
            hidden = {0: range(26, 34), 1: range(23, 37)}
        else:
            start = np.array([[-60.0 * n_frames / 2, 0.0, 900.0], [60.0 * n_frames / 2, 150.0, 900.0]])
            vel = np.array([[60.0, 0.0, 0.0], [-60.0, 0.0, 0.0]])
            hidden = {}
        for f in range(n_frames):
            shown = 0
            for k in range(G):
                pose = start[k] + vel[k] * f + skel[k]
                truth[f, b, k] = pose
                if f in hidden.get(k, ()):
                    continue
                dets[f, b, shown, :, :3] = pose + rng.normal(scale=noise, size=(J, 3))
                dets[f, b, shown, :, 3] = 0.0
                dets[f, b, shown, :, 4] = 0.9 - 0.1 * k
                shown += 1
            count[f, b, 0] = shown
    return dets, count, truth, G


def eval_sequences():
    """tracker + scorer over the synthetic sequences with the tracker's defaults, motion off and on -> the scores.  SYNTHETIC
    detection-level sequences: nothing here says anything about Panoptic."""
    from mvgformer_amd.tracking import PoseTracker, TrackEvaluator
    out = {}
    seeds = list(range(100, 108))
    say("synthetic detection-level sequences, %d seeds (one stream each), 60 frames, 20 mm detection noise, tracker defaults "
        "(max_dist 500, max_misses 10, min_hits 1; motion: dt 1, q 25, r 400, v0 2500), dist_thr 500" % len(seeds))
    say("    %-10s %-7s %6s %8s %6s %9s %7s %10s %5s %5s" % ("sequence", "motion", "MOTA", "MOTP mm", "IDF1", "switches", "misses",
                                                         "false_pos", "MT", "ML"))
    for kind in ("occlusion", "crossing"):
        dets, count, truth, G = _synthetic(kind, seeds)
        B = len(seeds)
        vis = torch.ones((B, G, J), device=DEV)
        num = torch.full((B,), G, dtype=torch.int32, device=DEV)
        for motion in (None, True):
            tracker = PoseTracker(batch=B, rows=dets.shape[2], num_joints=J, max_tracks=32, device=DEV, motion=motion)
            scorer = TrackEvaluator(batch=B, max_persons=G, max_ids=256, device=DEV)
            for f in range(dets.shape[0]):
                d, c = torch.from_numpy(dets[f]).to(DEV), torch.from_numpy(count[f]).to(DEV)
                tracker.update(d, c)
                scorer.update(tracker, d, c, torch.from_numpy(truth[f]).to(DEV), vis, num)
            t = scorer.report()["total"]
            name = "on" if motion else "off"
            say("    %-10s %-7s %6.4f %8.2f %6.4f %9d %7d %10d %5d %5d" % (kind, name, t["mota"], t["motp"], t["idf1"], t["switches"],
                                                                       t["misses"], t["false_pos"], t["mostly_tracked"],
                                                                       t["mostly_lost"]))
            out["%s_motion_%s" % (kind, name)] = {k: t[k] for k in ("mota", "motp", "idf1", "switches", "misses", "false_pos", "gt")}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--eval", type=int, default=0, choices=[0, 1],
                    help="1: measure the tracking scores instead (TrackEvaluator.update alone, GraphedDecoder tracking= with and without "
                         "track_evaluation=) and print MOTA / MOTP / IDF1 of the tracker with motion off and on over seeded synthetic "
                         "sequences, e.g. --reps 20 --out profiles/track_eval.txt")
    ap.add_argument("--motion", type=int, default=0, choices=[0, 1],
                    help="1: measure the constant-velocity motion model instead (PoseTracker(motion=True) against motion=None, and "
                         "GraphedDecoder tracking= with and without motion), e.g. --out profiles/track_motion.txt")
    ap.add_argument("--out", default=None, help="also write the printed lines to this file")
    a = ap.parse_args()
    if a.eval:
        res = eval_frames(a.reps, a.warmup)
        res.update(eval_launches(a.reps, a.warmup))
        res.update(eval_sequences())
    elif a.motion:
        res = motion_frames(a.reps, a.warmup)
        res.update(motion_updates(a.reps, a.warmup))
    else:
        res = frames(a.reps, a.warmup)
        res.update(updates(a.reps, a.warmup))
    say(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")
