"""Replay time of the cfg-2 bf16 forward with and without the live-view table (profiles/live_views.txt): three variants taken
alternating in one process -- a runner captured with the live kernels and all views live, a runner without the table, the live
runner with two of its five views dead.  Device events around `--steps` replays per round, `--rounds` rounds per variant; prints
each variant's median round mean and the spread of its rounds.

    python tools/bench_live_views.py [--rounds 7] [--steps 200] [--config cfg2]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--dead", default="1,3", help="views switched off in the third variant")
    args = ap.parse_args()
    from mvgformer_amd.factory import build_decoder_for_case, case_to_device
    from mvgformer_amd.serving import GraphedDecoder
    from mvgformer_amd.synthetic import build_case
    dev = "cuda:0"
    c = case_to_device(build_case(args.config, seed=0), dev)
    dec = build_decoder_for_case(c, dev, dtype=torch.bfloat16)
    dead = [int(v) for v in args.dead.split(",")]
    runners = {}
    for live in (False, True):
        run = GraphedDecoder(dec, c.meta, c.spatial_shapes, c.level_start_index, batch=1, num_queries=c.NQ, threshold=0.1,
                             live_views=live)
        run.load(src_views=c.src_views, tgt=c.tgt, query_pos=c.query_pos, reference_points=c.reference_points).capture()
        runners[live] = run
    variants = [("live kernels, all %d views live" % c.V, True, [True] * c.V), ("no table", False, None),
                ("live kernels, views %s dead" % dead, True, [v not in dead for v in range(c.V)])]
    times = {name: [] for name, _, _ in variants}
    for rnd in range(args.rounds + 1):                  # round 0 warms every variant up and is dropped
        for name, live, mask in variants:
            run = runners[live]
            if mask is not None:
                run.load(view_live=mask)
            run.replay()
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.steps):
                run.replay()
            t1.record()
            torch.cuda.synchronize()
            if rnd:
                times[name].append(t0.elapsed_time(t1) / args.steps)
    out = {"config": args.config, "dtype": "bf16", "rounds": args.rounds, "steps": args.steps}
    for name, _, _ in variants:
        ms = times[name]
        out[name] = {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}
        print("%-40s median %.4f ms  (rounds %.4f .. %.4f)" % (name, statistics.median(ms), min(ms), max(ms)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
