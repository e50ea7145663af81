"""Time of one training step of the decoder at cfg-2 size: forward under autograd (torch geometry +
ProjAttn with the HIP sampling forward / backward kernels) + backward to every parameter.  GPU only.
python tools/train_step_probe.py [config] [steps] [fp32|bf16] [--criterion] [--optimizer fused|torch] [--graph]
                                 [--backward det|balanced] [--chunk c] [--shelf] [--match knn|hungarian]
(bf16: DQDecoder.set_training_dtype(torch.bfloat16))
--criterion: the real step -- DecoderHead.forward_train (ground-truth match, decoder with the matched mask, fused criterion) on
synthetic ground truth (5 persons, K = 5) and total_loss(...).backward() -- instead of the made-up loss of the default run.
--shelf (with --criterion): the step in the Shelf / Campus joint format -- the head carries the shelf_campus YAMLs'
convert_joint_format_indices, the ground truth is the synthetic 15-joint persons gathered with that map (14 joints), matcher and
criterion run through their joint-map entry points.
--match (with --criterion): knn (default) -- KNNMatcher with K = 5 -- or hungarian -- factory.build_matcher_from_cfg's
HungarianMatcher, the reference's default match_method: one query per person on the device (mvg_hungarian_match), so the decoder
triangulates 5 queries per batch element, not 25.
--optimizer: the step includes the weight update (lr 4e-4, clip 0.1, the reference's two parameter groups).  torch: `if loss > 0`
on the host, clip_grad_norm_ and torch.optim.Adam, gradients zeroed in place; fused: optim.FusedAdam.step(loss=loss), the guard
on the device.  Without the option the step ends at backward() and drops the gradients, as before.
--graph (with --criterion --optimizer fused): the same step captured once as a HIP graph (training.GraphedTrainStep) and replayed,
timed next to the eager step in the same process.  Three figures: the plain step of this script (a DecoderContext per call; a block
of `steps` runs before the runner is built), runner.eager() (the identical step the graph holds: static context, bf16 operands kept by
the device) and runner.replay(); the last two alternate, each figure is the median over `steps` rounds.
--backward: the mode of the sampling op's backward (ops.BACKWARD_MODE; default: the library's, det); --chunk: ops.BACKWARD_CHUNK of
the balanced mode.  The --graph run also prints the device time of the bw_reduce* kernels in its profiled eager step."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from mvgformer_amd.factory import build_decoder_for_case, case_to_device  # noqa: E402
from mvgformer_amd.synthetic import build_case  # noqa: E402

with_criterion = "--criterion" in sys.argv
with_graph = "--graph" in sys.argv
with_shelf = "--shelf" in sys.argv
SHELF_MAP = [14, 13, 12, 6, 7, 8, 11, 10, 9, 3, 4, 5, 0, 1]       # configs/shelf_campus/*.yaml
argv = [a for a in sys.argv if a not in ("--criterion", "--graph", "--shelf")]
if with_shelf and not with_criterion:
    raise SystemExit("--shelf needs --criterion")
optimizer = None
if "--optimizer" in argv:
    i = argv.index("--optimizer")
    optimizer = argv[i + 1] if i + 1 < len(argv) else ""
    if optimizer not in ("fused", "torch"):
        raise SystemExit("--optimizer fused|torch")
    del argv[i:i + 2]
match = "knn"
if "--match" in argv:
    i = argv.index("--match")
    match = argv[i + 1] if i + 1 < len(argv) else ""
    if match not in ("knn", "hungarian") or not with_criterion:
        raise SystemExit("--match knn|hungarian (with --criterion)")
    del argv[i:i + 2]
backward = chunk = None
if "--backward" in argv:
    i = argv.index("--backward")
    backward = argv[i + 1] if i + 1 < len(argv) else ""
    if backward not in ("det", "balanced"):
        raise SystemExit("--backward det|balanced")
    del argv[i:i + 2]
if "--chunk" in argv:
    i = argv.index("--chunk")
    if i + 1 >= len(argv) or not argv[i + 1].isdigit():
        raise SystemExit("--chunk needs a number (0 or a positive multiple of 256)")
    chunk = int(argv[i + 1])
    del argv[i:i + 2]
    if backward != "balanced":
        raise SystemExit("--chunk needs --backward balanced")
if with_graph and not (with_criterion and optimizer == "fused"):
    raise SystemExit("--graph needs --criterion --optimizer fused")
cfg = argv[1] if len(argv) > 1 else "cfg2"
steps = int(argv[2]) if len(argv) > 2 else 5
tdt = argv[3] if len(argv) > 3 else "fp32"
if tdt not in ("fp32", "bf16"):
    raise SystemExit("training dtype must be fp32 or bf16")
from mvgformer_amd import ops  # noqa: E402
if backward is not None:
    ops.BACKWARD_MODE, ops.BACKWARD_CHUNK = backward, chunk
case = build_case(cfg, seed=0)
dec = build_decoder_for_case(case, "cuda", torch.float32)
if tdt == "bf16":
    dec.set_training_dtype(torch.bfloat16)
g = case_to_device(case, "cuda")
for p in dec.parameters():
    p.requires_grad_(True)
dec.train()
head = weight_dict = None
if with_criterion:
    from types import SimpleNamespace as NS
    from mvgformer_amd.caller import DecoderHead, total_loss
    from mvgformer_amd.factory import build_criterion_from_cfg, build_matcher_from_cfg
    from mvgformer_amd.synthetic import add_ground_truth, convert_ground_truth
    add_ground_truth(g, 5, Gmax=10, seed=0)
    if with_shelf:
        convert_ground_truth(g, SHELF_MAP)
    ccfg = NS(DECODER=NS(match_method="KNN" if match == "knn" else "hungarian", match_method_value=5), NETWORK=NS(IMAGE_SIZE=list(case.img_size)),
              MULTI_PERSON=NS(SPACE_SIZE=list(case.space_size), SPACE_CENTER=list(case.space_center)))
    criterion, weight_dict, decay = build_criterion_from_cfg(ccfg, matcher=None if match == "knn" else build_matcher_from_cfg(ccfg))
    head = DecoderHead(dec, case.NQ, 15, 256, case.space_size, case.space_center,
                       convert_joint_format_indices=SHELF_MAP if with_shelf else None).to("cuda").set_criterion(criterion, decay)
    head.train()
opt = None
if optimizer is not None:
    from types import SimpleNamespace as NS
    from mvgformer_amd.factory import build_optimizer_from_cfg
    model = head if head is not None else dec
    ocfg = NS(DECODER=NS(optimizer="adam", lr_linear_proj_mult=0.1), TRAIN=NS(LR=0.0004, clip_max_norm=0.1))
    opt = build_optimizer_from_cfg(model, ocfg)
    if optimizer == "torch":
        opt = torch.optim.Adam([{"params": gr["params"], "lr": gr["lr"]} for gr in opt.param_groups], lr=0.0004)
        trained = [p for gr in opt.param_groups for p in gr["params"]]


def update(loss):
    if optimizer == "fused":
        opt.step(loss=loss)                            # clip, Adam, the loss guard and the zeroing of the gradients: 3 launches
    elif loss > 0:                                     # lib/core/function.py:167-178
        torch.nn.utils.clip_grad_norm_(trained, 0.1)
        opt.step()
        opt.zero_grad(set_to_none=False)


def step():
    if opt is None:
        for p in dec.parameters():
            p.grad = None
    if head is not None:
        _, loss_dict = head.forward_train(g.src_views, g.meta, g.spatial_shapes, g.level_start_index, threshold=0.1)
        loss = total_loss(loss_dict, weight_dict)
        loss.backward()
        if opt is not None:
            update(loss.detach())
        return loss
    out = dec(g.tgt, g.reference_points, g.src_views, g.meta, g.spatial_shapes, g.level_start_index, None,
              query_pos=g.query_pos, threshold=0.1)
    loss = out[0].float().pow(2).mean() + 1e-6 * out[1].float().pow(2).mean() + sum(c.float().sum() for c in out[4]) * 1e-3
    loss.backward()
    if opt is not None:
        update(loss.detach())
    return loss


def graph_run():
    """eager step and replayed step alternating in one process: median times, device launches of one eager step, peak memory"""
    import statistics
    from mvgformer_amd.factory import build_graphed_train_step
    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out
    for _ in range(2):
        step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    # the plain step of this script (what the run without --graph times): a context per call -- host camera packing and its H2D
    # copy --, in bf16 the weights cast by torch.  Before the runner exists: building it attaches the device-kept operands.
    tp = [timed(step)[0] for _ in range(steps)]
    peak_eager = torch.cuda.max_memory_allocated() / 2 ** 30
    runner = build_graphed_train_step(head, opt, g, weight_dict)
    torch.cuda.synchronize()
    te, tr = [], []
    for _ in range(steps):
        ms, _ = timed(runner.eager)
        te.append(ms)
        ms, out = timed(runner.replay)
        tr.append(ms)
    peak_all = torch.cuda.max_memory_allocated() / 2 ** 30
    from torch.autograd import DeviceType
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
        runner.eager()
        torch.cuda.synchronize()
    events = list(prof.events())
    host = {e.name for e in events if e.device_type == DeviceType.CPU}
    launches = sum(1 for e in events if e.device_type == DeviceType.CUDA and e.name not in host)
    total = out[0]
    dev_ev = [e for e in events if e.device_type == DeviceType.CUDA and e.name not in host]
    by_name = {}
    for e in dev_ev:
        n, t = by_name.get(e.name, (0, 0.0))
        by_name[e.name] = (n + 1, t + e.time_range.elapsed_us())
    busy = sum(t for _, t in by_name.values())
    print("device time of one runner.eager() step: %.2f ms in %d launches; the largest:" % (busy / 1e3, len(dev_ev)))
    for name, (n, t) in sorted(by_name.items(), key=lambda kv: -kv[1][1])[:8]:
        print("  %8.3f ms  %4d x  %s" % (t / 1e3, n, name[:110]))
    reduce = [(n, t) for name, (n, t) in by_name.items() if "bw_reduce" in name]
    print("bw_reduce* kernels of that step (backward mode %s): %.3f ms in %d launches"
          % (ops.BACKWARD_MODE + ("" if ops.BACKWARD_CHUNK is None else ", chunk %d" % ops.BACKWARD_CHUNK), sum(t for _, t in reduce) / 1e3, sum(n for n, _ in reduce)))
    print(("%s training step (%s, " + match + " match + criterion%s + fused optimizer): plain step %.2f ms (context per call; median of %d in a block); "
          "runner.eager() %.2f ms (static context, operands kept by the device), graph replay %.2f ms (medians of %d, alternating; "
          "min %.2f / %.2f); %d device launches per runner.eager() step, 1 graph launch per replay; loss %.4f; peak memory %.2f GB "
          "plain, %.2f GB with the graph's pool") % (cfg, tdt, " in the Shelf joint format" if with_shelf else "", statistics.median(tp), steps, statistics.median(te), statistics.median(tr),
                                                   steps, min(te), min(tr), launches, float(total), peak_eager, peak_all))


if with_graph:
    graph_run()
    sys.exit(0)
for _ in range(2):
    step()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(steps):
    loss = step()
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / steps
# one multi-tensor launch instead of five per parameter: a profile of this script counts the steps' launches, not this check's
grads = [p.grad for p in dec.parameters() if p.grad is not None]
n_grad = int(torch.isfinite(torch.stack(torch._foreach_norm(grads))).sum())
print("%s training step (%s%s, forward + backward%s): %.1f ms; loss %.4f; %d / %d parameters with finite gradients; peak memory %.1f GB"
      % (cfg, tdt, (", match + criterion" + (" in the Shelf joint format" if with_shelf else "")) if with_criterion else "", " + %s optimizer" % optimizer if optimizer else "", dt * 1e3, float(loss), n_grad, sum(1 for _ in dec.parameters()), torch.cuda.max_memory_allocated() / 2 ** 30))
