"""Time of the one-to-one ground-truth matcher (mvg_hungarian_match) on the GPU, next to the reference's host path on the same box.
python tools/bench_hungarian.py [--reps n] [--no-step]

  device launch   ops.hungarian_match: one launch for all Lm * B problems.  Device time between two events on the launch stream,
                  median of `reps` after warm-up; and wall clock around a device synchronisation.
  host path       what lib/models/matcher.py does: the fp32 cost matrix on the device (torch ops), .cpu(), and
                  scipy.optimize.linear_sum_assignment per problem -- or, if scipy is not installed on the box, the numpy
                  restatement tests/hungarian_ref.solve (the line says which).  Wall clock, median of `reps`.
  shapes          the training shape NQ = 1024, G = 10 persons (Gmax = 10) at B = 1 and 8 with Lm = 1 (the match on the initial
                  poses) and Lm = 4 (every layer's own outputs); and the largest problem, NQ = 4096 with Gmax = G = 64 (costs in
                  the workspace, 16 columns per lane, the longest searches).
  graphed step    unless --no-step: tools/train_step_probe.py cfg2 <reps> fp32 --criterion --optimizer fused --graph, once with
                  --match hungarian and once with --match knn (K = 5), each in a fresh process.  The Hungarian step triangulates
                  one query per person, the KNN-5 step five: the two times are reported side by side, not compared.
"""
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import hungarian_cases as HC  # noqa: E402
from tests import hungarian_ref as H  # noqa: E402

DEV = "cuda:0"


def host_solver():
    try:
        from scipy.optimize import linear_sum_assignment
        return "scipy.optimize.linear_sum_assignment", lambda c: linear_sum_assignment(c)
    except ImportError:
        return "numpy restatement tests/hungarian_ref.solve (scipy is not installed here)", lambda c: H.solve(np.ascontiguousarray(c.T))


def class_cost(logits):
    """matcher.py:151-162 in torch, fp32, every target in class 1"""
    p = logits.sigmoid()[..., 1]
    return 0.25 * (1 - p) ** 2 * (-(p + 1e-8).log()) - 0.75 * p ** 2 * (-(1 - p + 1e-8).log())


def median_ms(fn, reps, warm=5, events=False):
    out = []
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for i in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if events:
            ev[0].record()
        fn()
        if events:
            ev[1].record()
        torch.cuda.synchronize()
        if i >= warm:
            out.append(ev[0].elapsed_time(ev[1]) if events else (time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out)


def bench_shape(B, Lm, NQ, Gmax, reps, solver):
    from mvgformer_amd import ops
    c = {**HC.CASES["train"], "B": B, "Lm": Lm, "NQ": NQ, "Gmax": Gmax, "num_person": [Gmax] * B, "seed": 300 + B + Lm}
    inp = HC.make_inputs(c)
    t = {k: torch.from_numpy(v).to(DEV) for k, v in inp.items()}
    size, cen = torch.tensor(HC.SPACE_SIZE, device=DEV), torch.tensor(HC.SPACE_CENTER, device=DEV)

    def device():
        return ops.hungarian_match(t["poses"], t["joints_3d"], t["num_person"], HC.SPACE_SIZE, HC.SPACE_CENTER, logits=t["logits"],
                                   cost_class=2.0, cost_pose=5.0)

    def host():
        gt = t["joints_3d"]
        tgt = (((gt - cen + size / 2.0) / size) * size + cen - size / 2.0).reshape(B, Gmax, -1)
        pairs = []
        for l in range(Lm):
            cost = 5.0 * 0.01 * torch.cdist(t["poses"][l].reshape(B, NQ, -1), tgt, p=1) + 2.0 * class_cost(t["logits"][l])[..., None]
            cost = cost.cpu()                                          # the round trip the device path does not have
            pairs += [solver(cost[b].numpy()) for b in range(B)]
        return pairs
    pq = device()[0].cpu().numpy().reshape(Lm * B, Gmax)
    agree = sum(np.array_equal(np.asarray(h[0]), pq[i]) for i, h in enumerate(host()) if len(h) == 2)
    dev_ev, dev_ev_min = median_ms(device, reps, events=True)
    dev_wall, _ = median_ms(device, reps)
    host_wall, host_min = median_ms(host, reps)
    print("B %d  Lm %d  NQ %4d  G %2d : device launch %.3f ms (min %.3f; wall clock with sync %.3f ms) | host path %.3f ms (min %.3f) | "
          "%d / %d problems with the same queries" % (B, Lm, NQ, Gmax, dev_ev, dev_ev_min, dev_wall, host_wall, host_min, agree, Lm * B),
          flush=True)


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 30
    name, solver = host_solver()
    print("host path: fp32 cost on the device, .cpu(), %s per problem; %d repetitions each, medians" % (name, reps), flush=True)
    for B, Lm, NQ, Gmax in ((1, 1, 1024, 10), (8, 1, 1024, 10), (1, 4, 1024, 10), (8, 4, 1024, 10), (1, 1, 4096, 64), (8, 1, 4096, 64)):
        bench_shape(B, Lm, NQ, Gmax, reps, solver)
    if "--no-step" in sys.argv:
        return
    probe = os.path.join(ROOT, "tools", "train_step_probe.py")
    for match in ("hungarian", "knn"):
        cmd = [sys.executable, probe, "cfg2", "10", "fp32", "--criterion", "--optimizer", "fused", "--graph", "--match", match]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            print("train_step_probe --match %s failed (%d):\n%s" % (match, r.returncode, r.stderr[-2000:]), flush=True)
            sys.exit(1)                                                # a failed step ends the run: nothing more goes to the GPU
        lines = [l for l in r.stdout.splitlines() if "training step" in l or l.startswith("device time")]
        print("\n".join(lines), flush=True)


if __name__ == "__main__":
    main()
