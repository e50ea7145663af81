"""Backward of the sampling op at the size of one cfg-2 view-layer: deterministic (csrc/msda_bwd.hip), balanced and atomic form.
python tools/bench_bwd.py [modes] [reps] [fp32|bf16] [--dist uniform|clustered:<f>] [--N n] [--chunk c] [--rounds r]
  modes   det | atomic | balanced | balanced:<chunk>, or several of them separated by commas: they then ALTERNATE inside one process,
          `--rounds` times, and every round prints one figure per mode (A/B on the same device in the same minute)
  bf16    a bf16 value (mvg_msda_backward_det_bf16 / _bal_bf16)
  --dist  uniform: every query has its own centre (the default); clustered:<f>: the first round(f * Lq) queries of an image share one
          centre -- training with the matcher, where every unmatched query re-enters at the world origin and projects to one pixel per
          view; f = 0.976 is 999 of 1 024 persons
  --N     images per call (training calls the op with N = V * B = 5); default 1
  --chunk entries per work item of `balanced` where the mode does not name one; default: the library's
Run under `rocprofv3 --kernel-trace --stats` for the per-kernel split."""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mvgformer_amd import ops  # noqa: E402


def _option(argv, name, default):
    if name in argv:
        i = argv.index(name)
        if i + 1 >= len(argv):
            raise SystemExit(name + " needs a value")
        value = argv[i + 1]
        del argv[i:i + 2]
        return value
    return default


argv = sys.argv[1:]
dist = _option(argv, "--dist", "uniform")
N = int(_option(argv, "--N", "1"))
chunk_default = _option(argv, "--chunk", None)
rounds = int(_option(argv, "--rounds", "1"))
modes = (argv[0] if len(argv) > 0 else "det").split(",")
reps = int(argv[1]) if len(argv) > 1 else 10
vdt = argv[2] if len(argv) > 2 else "fp32"
frac = 0.0
if dist.startswith("clustered:"):
    frac = float(dist.split(":", 1)[1])
    if not 0.0 <= frac <= 1.0:
        raise SystemExit("clustered:<f> needs 0 <= f <= 1")
elif dist != "uniform":
    raise SystemExit("--dist uniform|clustered:<f>")
specs = []
for m in modes:
    name, _, c = m.partition(":")
    if name not in ("det", "atomic", "balanced") or (c and name != "balanced"):
        raise SystemExit("mode: det | atomic | balanced[:chunk]")
    specs.append((m, name, int(c) if c else (int(chunk_default) if chunk_default and name == "balanced" else None)))

dev = "cuda:0"
shapes = torch.tensor([(128, 240), (64, 120), (32, 60)], dtype=torch.long)
starts = torch.cat([shapes.new_zeros(1), (shapes[:, 0] * shapes[:, 1]).cumsum(0)[:-1]])
M, D, Lq, P, L = 8, 32, 15360, 8, 3
S = int((shapes[:, 0] * shapes[:, 1]).sum())
g = torch.Generator().manual_seed(21)
value = torch.randn((N, S, M, D), generator=g).to(dev)
if vdt == "bf16":
    value = value.to(torch.bfloat16)
centre = torch.rand((N, Lq, 1, 1, 1, 2), generator=g) * 1.1 - 0.05
n_clustered = int(round(frac * Lq))
if n_clustered:
    centre[:, :n_clustered] = 0.2 + 0.6 * torch.rand((N, 1, 1, 1, 1, 2), generator=g)
loc = (centre + torch.randn((N, Lq, M, L, P, 2), generator=g) * 0.03).contiguous().to(dev)
wgt = torch.softmax(torch.randn((N, Lq, M, L * P), generator=g), -1).view(N, Lq, M, L, P).contiguous().to(dev)
go = torch.randn((N, Lq, M * D), generator=g).to(dev)
shapes, starts = shapes.to(dev), starts.to(dev)


def run(name, chunk, count):
    ops.BACKWARD_MODE, ops.BACKWARD_CHUNK = name, chunk
    out = None
    for _ in range(count):
        out = ops.msda_backward(value, shapes, starts, loc, wgt, go)
    return out


first = None
for label, name, chunk in specs:
    out = run(name, chunk, 2)
    torch.cuda.synchronize()
    if name != "atomic":                   # the deterministic forms agree on every bit
        if first is None:
            first = (label, [t.clone() for t in out])
        elif not all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(out, first[1])):
            raise SystemExit("%s and %s differ" % (label, first[0]))
a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
what = "%s value, N = %d, %s" % (vdt, N, dist)
for r in range(rounds):
    for label, name, chunk in specs:
        a.record()
        run(name, chunk, reps)
        b.record()
        torch.cuda.synchronize()
        print("%s backward (%s), %s cfg-2 view-layer%s: %.0f us%s" % (label, what, "one" if N == 1 else "%d" % N, "" if N == 1 else "s",
                                                                   a.elapsed_time(b) / reps * 1e3,
                                                                   "  (round %d)" % (r + 1) if rounds > 1 else ""))
