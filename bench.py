#!/usr/bin/env python
"""bench.py -- MVGFormer decoder hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A "step" = ONE decoder forward (DQDecoder.forward-equivalent: pyramid packing, all layers, all
views, 2D refinement, triangulation, output scatter/stack; backbone and data loading excluded)
over one synthetic sample already resident in HBM.  Workload = BASELINE.json configs[1]:
Panoptic CMU0 geometry, 5 views, 1024 queries x 15 joints, 4 layers, feature maps
(128,240)/(64,120)/(32,60) x 256 ch, bf16 storage + bf16 MFMA with fp32 accumulation
(geometry fp32/fp64).  With N > 1 the person-queries are sharded over the ranks
(BASELINE.json configs[2]) and the pose set is assembled with one RCCL all-gather per forward.

Rank 0 prints ONE JSON line (contract in the task statement).  A plain run does only what the headline
figure needs: set up, warm up, time the K steps, print the line.  With --full it also fills
  roofline     : the sampling kernel (msda_gsamp / msda_fused), HIP-event timed per launch on its stream
  cpu_baseline : the CPU oracle (oracle/decoder_ref.py, "port") timed on <= 32 host threads on a
                 bounded sample (as many of the 4 layers as fit in ~30 s), scaled to samples/s
and the other objects of the line (roofline_mfma, kernels, rank_time_split, secondary), which stay null / empty
in a plain run.  --dump-outputs DIR writes what the timed forward returned in its last step (dump_outputs).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def algorithmic_bytes_per_view_layer(S, C, Lq, M, L, P, elem):
    """value read once + locations + weights + output."""
    return S * C * elem + Lq * M * L * P * 2 * elem + Lq * M * L * P * elem + Lq * C * elem


def dense_flops(S, C, Lq, M, L, P, F, V, B, layers, exec_rows_a=None):
    """SURVEY.md section 8(d), dense (MFMA) regime, per forward.  nominal: the reference's decomposition -- value, offsets and
    logits Linears on the gathered rows, output projection, pose MLP (all pairs), update Linear, FFN.  executed: what this
    build's bf16 / fp32 kernels multiply -- the offsets / logits Linear applied to the pyramid (G, V*S rows instead of V*Lq*L) +
    the query term (Lq rows), chain A on the rows of the tiles it does not skip (exec_rows_a per layer; None = all pairs)."""
    per_view = 2 * S * C * C + 2 * Lq * L * C * (M * P * 2) + 2 * Lq * L * C * (M * P) + 2 * Lq * C * C + 2 * Lq * (2 * C * C + 3 * C)
    nominal = layers * B * (V * per_view + 2 * Lq * C * C + 4 * Lq * C * F)
    rows_a = [V * B * Lq] * layers if exec_rows_a is None else list(exec_rows_a)
    value = 2 * V * B * S * C * C
    g = 2 * V * B * S * C * (M * P * 3)
    xw = 2 * B * Lq * C * (M * P * 3)
    chain_a = [2 * r * (3 * C * C + 3 * C) for r in rows_a]
    chain_b = 2 * B * Lq * (C * C + 2 * C * F + 2 * C)
    executed = layers * (value + g + xw + chain_b) + sum(chain_a)
    return {"nominal": nominal, "executed": executed, "value": value, "G": g, "query_term": xw,
            "chain_a": sum(chain_a) / max(len(chain_a), 1), "chain_b": chain_b}


SAMPLER_SOURCES = ("mvgformer_amd/csrc/msda.hip", "mvgformer_amd/csrc/gsamp_dev.h", "mvgformer_amd/csrc/common.h")


def sampler_source_hash():
    """sha256 over the sources of the sampling kernel: a committed PMC figure is only quoted for the code it was measured on"""
    import hashlib
    h = hashlib.sha256()
    for rel in SAMPLER_SOURCES:
        with open(os.path.join(ROOT, rel), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def pmc_child_pass(counters, argv_tail, kernel_prefix):
    """One rocprofv3 --pmc child pass (its own run: --pmc with --kernel-trace only) over a few eager forwards of this very
    configuration -> ({counter: mean per launch of the kernels whose name contains kernel_prefix}, None) or (None, reason)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3")
    if exe is None:
        return None, "rocprofv3 not on PATH"
    tmp = tempfile.mkdtemp(prefix="mvg_pmc_", dir="/tmp")
    try:
        cmd = [exe, "--pmc"] + list(counters) + ["--kernel-trace", "-d", tmp, "-o", "pmc", "--output-format", "csv", "--",
                                                 sys.executable, os.path.abspath(__file__), "--pmc-child", "1"] + argv_tail
        env = dict(os.environ, TMPDIR="/tmp", MVG_OVERLAP_PYRAMID="0")
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
            env.pop(k, None)
        p = subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        got = {c: [] for c in counters}
        for f in glob.glob(os.path.join(tmp, "**", "*counter_collection.csv"), recursive=True):
            with open(f) as fh:
                for r in csv.DictReader(fh):
                    if r["Counter_Name"] in got and kernel_prefix in r["Kernel_Name"]:
                        got[r["Counter_Name"]].append(float(r["Counter_Value"]))
        missing = [c for c, v in got.items() if not v]
        if missing:
            return None, "no %s samples for %s (rc %d: %s)" % ("/".join(missing), kernel_prefix, p.returncode, p.stderr[-300:])
        return {c: sum(v) / len(v) for c, v in got.items()}, None
    except Exception as e:      # profiler trouble must never cost the bench line
        return None, "%s pass failed: %s: %s" % ("/".join(counters), type(e).__name__, e)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def measure_traffic_live(argv_tail, kernel_prefix):
    """HBM-side bytes per launch of the sampling kernel, measured NOW: two rocprofv3 --pmc child passes (FETCH_SIZE and WRITE_SIZE
    do not fit one pass; MI355X_MICROARCH.md, "rocprofv3 PMC slots"), FETCH_SIZE doubled per the guide's gfx950 correction.
    Returns (bytes, detail) or (None, reason)."""
    vals = {}
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        got, why = pmc_child_pass([counter], argv_tail, kernel_prefix)
        if got is None:
            return None, why
        vals.update(got)
    total = (2.0 * vals["FETCH_SIZE"] + vals["WRITE_SIZE"]) * 1024.0
    return int(total), {"FETCH_SIZE_KB_per_launch": vals["FETCH_SIZE"], "WRITE_SIZE_KB_per_launch": vals["WRITE_SIZE"],
                        "fetch_correction": 2.0}


def measure_issue_shares(argv_tail, kernel_prefix, n_cu=256):
    """What the sampling kernel's launch keeps busy (a third PMC child pass): the vector ALUs -- SQ_ACTIVE_INST_VALU counts
    quad-cycles, x 4 / (GRBM_GUI_ACTIVE / 8 XCDs) / (4 SIMDs x n_cu) -- and the texture-address path, which accepts the lane
    addresses of one 64-lane 16-byte load in ~18.3 clk per CU (tools/probes/l1_gather_probe: 56 B/clk/CU): SQ_INSTS_VMEM_RD x 18.3 /
    n_cu / (GRBM_GUI_ACTIVE / 8).  Returns ({valu_busy, l1_addr_busy, ...}, None) or (None, reason)."""
    got, why = pmc_child_pass(["SQ_ACTIVE_INST_VALU", "SQ_INSTS_VALU", "SQ_INSTS_VMEM_RD", "SQ_WAVES", "GRBM_GUI_ACTIVE"], argv_tail, kernel_prefix)
    if got is None:
        return None, why
    clk = got["GRBM_GUI_ACTIVE"] / 8.0
    return {"valu_busy": round(got["SQ_ACTIVE_INST_VALU"] * 4.0 / clk / (4 * n_cu), 4),
            "l1_addr_busy": round(got["SQ_INSTS_VMEM_RD"] * 18.3 / n_cu / clk, 4),
            "valu_insts_per_wave": round(got["SQ_INSTS_VALU"] / got["SQ_WAVES"], 1),
            "vmem_rd_per_wave": round(got["SQ_INSTS_VMEM_RD"] / got["SQ_WAVES"], 2),
            "launch_clk": round(clk, 0)}, None


def measure_sampler_in_forward(argv_tail, kernel_prefix, launches_per_forward, replays=8):
    """Duration of the sampling kernel INSIDE the graph-replayed forward (what the timed region runs): one rocprofv3 --kernel-trace
    child pass over `replays` replays of this configuration, the kernel's launches of those replays taken from the end of the trace.
    (The eager profile pass times every kernel alone; in the forward the sampler finds its planes written just before it.)
    Returns (mean us, n launches) or (None, reason)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3")
    if exe is None:
        return None, "rocprofv3 not on PATH"
    tmp = tempfile.mkdtemp(prefix="mvg_kt_", dir="/tmp")
    try:
        cmd = [exe, "--kernel-trace", "-d", tmp, "-o", "kt", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
               "--steps", str(replays), "--warmup", "2", "--secondary", "0", "--traffic", "off", "--profile-steps", "0"] + argv_tail
        env = dict(os.environ, TMPDIR="/tmp")
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
            env.pop(k, None)
        p = subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        rows = []
        for f in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            with open(f) as fh:
                for r in csv.DictReader(fh):
                    if kernel_prefix in r["Kernel_Name"]:
                        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
        need = launches_per_forward * replays
        if len(rows) < need:
            return None, "%d launches of %s in the trace, %d expected (rc %d: %s)" % (len(rows), kernel_prefix, need, p.returncode, p.stderr[-300:])
        rows.sort()
        last = rows[-need:]
        return sum(e - s for s, e in last) / len(last) * 1e-3, len(last)
    except Exception as e:      # profiler trouble must never cost the bench line
        return None, "kernel-trace pass failed: %s: %s" % (type(e).__name__, e)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


SAMPLER_KERNELS = {"msda_gsamp": "msda_gsamp_kernel",
                   "msda_gfused_f32": "msda_gfused_f32_hp_kernel", "msda_fused": "msda_fused_kernel"}


def sampler_kernel_name(key, n_pairs):
    """the kernel a profile label of the sampling step stands for: the bf16 G-sampling launch runs its double-buffered build from
    32 768 pairs per launch on (csrc/msda.hip: mvg_msda_gsamp), unless a tuning knob says otherwise"""
    if key == "msda_gsamp":
        from mvgformer_amd import _lib
        pipe = _lib.TUNING.get("gsamp_pipe", 0)
        if pipe == 1 or (pipe == 0 and n_pairs >= 32768):
            return "msda_gsamp_pipe_kernel"
    return SAMPLER_KERNELS[key]

# the workloads measured next to the headline in the driver's one command: (name, config, dtype, inside, batch)
SECONDARY = (("cfg2_fp32", "cfg2", "fp32", "grid", 1), ("cfg4_fp32", "cfg4", "fp32", "grid", 1),
             ("cfg2_bf16_inside_all", "cfg2", "bf16", "all", 1), ("cfg5_bf16", "cfg5", "bf16", "grid", 1),
             ("cfg2_bf16_batch2", "cfg2", "bf16", "grid", 2), ("cfg2_bf16_batch4", "cfg2", "bf16", "grid", 4),
             ("cfg2_bf16_valid10", "cfg2", "bf16", "valid10", 1), ("cfg2_bf16_producer_inplace", "cfg2", "bf16", "inplace", 1))
FP32_FORM = "2xfp16x3"      # fp32 kernels: operands as two fp16 parts x a power-of-two scale, three fp16 MFMA products, fp32 accumulation


def measure_train_step(dev, steps=5, warmup=2):
    """cfg-2 fp32 training step (run/train_3d.py's decoder share): forward under autograd + backward to every
    parameter of the 4-layer decoder, `steps` timed steps after `warmup`, then a finite-gradient check and the kernel launches
    of one step (torch.profiler device activities)."""
    import gc
    from mvgformer_amd.factory import build_decoder_for_case, case_to_device
    from mvgformer_amd.synthetic import build_case
    case = build_case("cfg2", seed=0)
    dec = build_decoder_for_case(case, dev, torch.float32)
    g = case_to_device(case, dev)
    for p in dec.parameters():
        p.requires_grad_(True)
    dec.train()

    def step():
        for p in dec.parameters():
            p.grad = None
        out = dec(g.tgt, g.reference_points, g.src_views, g.meta, g.spatial_shapes, g.level_start_index, None,
                  query_pos=g.query_pos, threshold=0.1)
        loss = out[0].float().pow(2).mean() + 1e-6 * out[1].float().pow(2).mean() + sum(c.float().sum() for c in out[4]) * 1e-3
        loss.backward()
        return loss
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    params = list(dec.parameters())
    grads = [p.grad for p in params if p.grad is not None]
    finite = int(torch.isfinite(torch.stack(torch._foreach_norm(grads))).sum())
    launches = None
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        launches = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
    except Exception as e:      # the count is a diagnostic
        launches = "n/a (%s)" % type(e).__name__
    rec = {"workload": "cfg2: training step of the 4-layer decoder, fp32, forward under autograd + backward to every parameter",
           "dtype": "fp32", "fp32_form": FP32_FORM, "steps": steps, "ms_per_step": round(elapsed / steps * 1e3, 3),
           "value": round(steps / elapsed, 3), "unit": "steps/s", "hip_graph": False, "loss": round(float(loss), 5),
           "parameters_with_finite_gradients": "%d / %d" % (finite, len(grads)), "parameters": len(params), "device_activities_per_step": launches,
           "peak_memory_GB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}
    assert finite == len(grads) and finite > 0, "non-finite gradients"
    del dec, g, case, grads, params, loss
    gc.collect()
    torch.cuda.empty_cache()
    return rec


def measure_secondary(config, dtype_name, inside, batch, dev, steps=20, warmup=3, profile_steps=2):
    """One more workload in this process, after the headline's timed region: `steps` graph-replayed forwards of a batch of
    `batch` samples (barrier-free single GPU: synchronize on both sides), then `profile_steps` eager forwards with the side
    stream off for the sampling kernel's own duration.  No PMC passes, no CPU leg.  inside = "inplace": the default poses with the
    pyramid produced in the packed layout (DecoderContext.pyramid_buffers(): SURVEY 8 f3's hand-off, no per-step pack)."""
    import gc
    from mvgformer_amd import ops
    from mvgformer_amd.decoder import DecoderContext
    from mvgformer_amd.factory import build_decoder_for_case, case_to_device
    from mvgformer_amd.synthetic import build_case
    dtype = torch.bfloat16 if dtype_name == "bf16" else torch.float32
    elem = 2 if dtype_name == "bf16" else 4
    case = build_case(config, B=batch, seed=0, ref_extent=0.3 if inside == "all" else 1.0,
                      valid_fraction=0.1 if inside == "valid10" else None)
    dec = build_decoder_for_case(case, dev, dtype)
    g = case_to_device(case, dev)
    ctx = DecoderContext.prepare(g.spatial_shapes, g.level_start_index, g.meta, case.img_size, dtype, batch, dev)
    src_views = g.src_views
    if inside == "inplace":
        src_views = ctx.pyramid_buffers(channels=g.src_views[0].shape[1])
        for dst, s_ in zip(src_views, g.src_views):
            dst.copy_(s_)

    def forward():
        ctx.feat = None
        return dec(g.tgt, g.reference_points, src_views, g.meta, g.spatial_shapes, g.level_start_index, None,
                   query_pos=g.query_pos, threshold=0.1, context=ctx)
    with torch.no_grad():
        for _ in range(2):
            out = forward()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = forward()
        for _ in range(warmup):
            graph.replay()
        torch.cuda.synchronize()
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
        t0 = time.perf_counter()
        evs[0].record()
        for i in range(steps):
            graph.replay()
            evs[i + 1].record()
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        per_step = sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(steps))
        median = per_step[steps // 2] if steps % 2 else 0.5 * (per_step[steps // 2 - 1] + per_step[steps // 2])
        assert torch.isfinite(out[1]).all(), "non-finite poses"
        valid_share = float((out[4][-1][..., 1] > 0.1).float().mean())
        saved, ops.PROFILE = ops.PROFILE, {}
        overlap, dec.overlap_pyramid = dec.overlap_pyramid, False
        for _ in range(profile_steps):
            forward()
        torch.cuda.synchronize()
        prof = ops.profile_summary()
        ops.PROFILE, dec.overlap_pyramid = saved, overlap
    S = int(sum(h * w for h, w in case.shapes))
    bytes_launch = batch * case.V * algorithmic_bytes_per_view_layer(S, 256, case.NQ * 15, 8, len(case.shapes), 8, elem)
    key = next((k for k in SAMPLER_KERNELS if k in prof), None)
    rec = {"workload": "%s: %d views, %d queries x 15 joints, %d layers, maps %s x 256ch, batch %d, initial poses %s"
                       % (config, case.V, case.NQ, case.layers, case.shapes, batch,
                          "grid, ~10 % of the queries pass the 0.1 threshold" if inside == "valid10" else
                          "grid, pyramid handed over in the packed layout (no per-step pack)" if inside == "inplace" else inside),
           "dtype": dtype_name, "steps": steps, "ms_per_step": round(median, 4),
           "ms_per_step_median": round(median, 4), "ms_per_step_mean": round(elapsed / steps * 1e3, 4),
           "ms_per_step_min_max": [round(per_step[0], 4), round(per_step[-1], 4)],
           "ms_per_sample": round(median / batch, 4), "value": round(batch * steps / elapsed, 3),
           "unit": "samples/s", "hip_graph": True, "valid_query_share_last_layer": round(valid_share, 4),
           "note": "as in the headline: ms_per_step (= ms_per_step_median) and ms_per_sample from the median of the per-replay HIP-event "
                   "intervals, ms_per_step_mean = wall clock / steps, which `value` is computed from"}
    if dtype_name == "fp32":
        rec["fp32_form"] = FP32_FORM
    if key is not None:
        us = prof[key][1] * 1e3
        rec.update({"sampler_kernel": sampler_kernel_name(key, batch * case.V * case.NQ * 15), "sampler_us": round(us, 2),
                    "frac": round(bytes_launch / (us * 1e-6) / 8e12, 4), "algorithmic_bytes_per_launch": bytes_launch})
    rec["kernels_us"] = {k: round(ms * 1e3, 1) for k, (n, ms) in sorted(prof.items())}
    del graph, out, dec, g, ctx, case
    gc.collect()
    torch.cuda.empty_cache()
    return rec


DUMP_LIMIT = 64 << 20       # bytes a --dump-outputs directory may take in all
DUMP_SAMPLED = 32 << 20     # what a dump over DUMP_LIMIT is cut down to


def dump_outputs(out, path):
    """--dump-outputs: what a caller of the timed forward receives from its last step, as <path>/<name>.npy -- hs, refs, refs2d,
    projs2d (DQDecoder.forward's per-layer stacks; hs is absent where the query-sharded path does not gather it) and class_prob (its
    per-layer class probabilities, stacked) -- in float32 (float64 stays float64).  If the arrays take more than DUMP_LIMIT bytes,
    every one keeps the same fixed, seeded sample of its query axis (axis -2), about DUMP_SAMPLED bytes in all; the sample depends
    only on the shapes, so two runs with the same arguments compare row for row.  Returns {name: shape written}."""
    import numpy as np
    named = list(zip(("hs", "refs", "refs2d", "projs2d"), out[:4])) + [("class_prob", torch.stack(list(out[4])))]
    host = {name: t.detach().to(torch.float64 if t.dtype == torch.float64 else torch.float32).cpu().numpy()
            for name, t in named if t is not None}
    total = sum(a.nbytes for a in host.values())
    if total > DUMP_LIMIT:
        frac = DUMP_SAMPLED / total
        for name, a in host.items():
            n = a.shape[-2]
            rows = np.sort(np.random.RandomState(0).choice(n, max(1, int(n * frac)), replace=False))
            host[name] = np.ascontiguousarray(np.take(a, rows, axis=-2))
    os.makedirs(path, exist_ok=True)
    for name, a in host.items():
        np.save(os.path.join(path, name + ".npy"), a)
    return {name: list(a.shape) for name, a in host.items()}


def rccl_preflight(rank, world, dev):
    """First contact with the collectives BEFORE anything is timed: one all_gather_into_tensor and one MAX all_reduce on tiny
    tensors, the library version and every rank's device.  A failure prints a line that says where it happened instead of
    leaving the job hanging inside the timed region."""
    info = {"ranks": world, "backend": dist.get_backend()}
    try:
        t0 = time.perf_counter()
        mine = torch.tensor([rank, torch.cuda.current_device()], dtype=torch.int32, device=dev)
        seen = torch.empty((world * 2,), dtype=torch.int32, device=dev)
        dist.all_gather_into_tensor(seen, mine)
        top = torch.tensor([rank], dtype=torch.int32, device=dev)
        dist.all_reduce(top, op=dist.ReduceOp.MAX)
        torch.cuda.synchronize()
        seen = seen.view(world, 2).tolist()
        info.update({"ranks_seen": [r for r, _ in seen], "local_devices": [d for _, d in seen], "max_rank": int(top.item()),
                     "first_collectives_s": round(time.perf_counter() - t0, 3), "device_name": torch.cuda.get_device_name(dev)})
        try:
            info["version"] = ".".join(str(v) for v in torch.cuda.nccl.version())
        except Exception as e:           # gloo plumbing runs
            info["version"] = "n/a (%s)" % type(e).__name__
        if info["ranks_seen"] != list(range(world)) or info["max_rank"] != world - 1:
            raise RuntimeError("ranks seen %s, max %s" % (info["ranks_seen"], info["max_rank"]))
        info["ok"] = True
    except Exception as e:
        info.update({"ok": False, "error": "%s: %s" % (type(e).__name__, e)})
        print("# rank %d/%d: collective preflight FAILED on %s (backend %s): %s" % (rank, world, dev, dist.get_backend(), info["error"]),
              file=sys.stderr, flush=True)
    return info


def measure_replicas(config, dtype_name, rank, world, dev, steps, warmup):
    """N GPUs, one sample per rank and step (batch-parallel replicas, weak scaling): every rank's own full forward as a HIP
    graph + one all-gather of the final pose sets per step; barrier + synchronize on both sides, MAX over the ranks."""
    import gc
    from mvgformer_amd.decoder import DecoderContext
    from mvgformer_amd.factory import build_decoder_for_case, case_to_device
    from mvgformer_amd.synthetic import build_case
    dtype = torch.bfloat16 if dtype_name == "bf16" else torch.float32
    case = build_case(config, seed=100 + rank)
    dec = build_decoder_for_case(case, dev, dtype)
    g = case_to_device(case, dev)
    ctx = DecoderContext.prepare(g.spatial_shapes, g.level_start_index, g.meta, case.img_size, dtype, 1, dev)

    def forward():
        ctx.feat = None
        return dec(g.tgt, g.reference_points, g.src_views, g.meta, g.spatial_shapes, g.level_start_index, None,
                   query_pos=g.query_pos, threshold=0.1, context=ctx)
    with torch.no_grad():
        for _ in range(2):
            out = forward()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = forward()
        send = torch.cat([out[1][-1].reshape(-1), out[4][-1].reshape(-1)])
        recv = send.new_empty((world * send.numel(),))

        def step():
            graph.replay()
            torch.cat([out[1][-1].reshape(-1), out[4][-1].reshape(-1)], out=send)
            dist.all_gather_into_tensor(recv, send)
        for _ in range(warmup):
            step()
        dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        dist.barrier()
        elapsed = time.perf_counter() - t0
    tmax = torch.tensor([elapsed], dtype=torch.float64, device=dev)
    dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    elapsed = float(tmax.item())
    rec = {"workload": "%s, one sample per rank and step, all-gather of the final pose sets" % config, "dtype": dtype_name,
           "scaling": "weak", "n_gpus": world, "steps": steps, "ms_per_step": round(elapsed / steps * 1e3, 4),
           "value": round(world * steps / elapsed, 3), "unit": "samples/s", "hip_graph": True}
    del graph, out, dec, g, ctx, case
    gc.collect()
    torch.cuda.empty_cache()
    return rec


def self_launch(n):
    """Re-run this command line as n ranks under torch.distributed.run (one process per GPU); returns its exit code."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 1) // n)))
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--config", default="cfg2", help="cfg2 (headline) | cfg4 | cfg5 | cfg1 | mini5")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--graph", type=int, default=-1,
                    help="replay the forward as a captured HIP graph (-1 = auto: on for 1 GPU, off when the forward "
                         "contains RCCL collectives)")
    ap.add_argument("--valid-fraction", type=float, default=None,
                    help="fraction of queries passing the 0.1 threshold (default: all valid -- every query is refined, "
                         "scattered sampling locations; with a fraction the failing queries sit on reference point "
                         "0 like the reference's, all of them inside every view)")
    ap.add_argument("--producer", default="nchw", choices=["nchw", "nhwc", "inplace"],
                    help="layout the feature pyramid is handed over in (SURVEY 8 f3): nchw = fp32 NCHW maps as the "
                         "reference's backbone emits them (default, the headline configuration); nhwc = channels-last "
                         "maps in the compute dtype; inplace = the producer wrote into DecoderContext.pyramid_buffers()")
    ap.add_argument("--shard", default="queries", choices=["queries", "samples"],
                    help="N > 1: queries = ONE sample per step, its person-queries sharded over the ranks + all-gather of "
                         "the pose set (BASELINE configs[2], strong scaling; default); samples = one sample per rank and "
                         "step, all-gather of the final pose sets (batch-parallel replicas, weak scaling)")
    ap.add_argument("--inflight", type=int, default=1,
                    help="samples in flight per GPU (serving mode, 1 GPU / --shard samples): K independent decoder "
                         "instances, each forward a HIP graph on its own stream, replayed concurrently; a step is then "
                         "K samples.  Default 1 = the single-sample forward the headline number is quoted on")
    ap.add_argument("--queries", type=int, default=None,
                    help="override the configuration's query count (diagnostics: --queries 128 is the per-rank workload "
                         "of the 8-GPU query-sharded run; the metric name then no longer applies)")
    ap.add_argument("--emulate-rank", type=int, default=None,
                    help="one GPU runs the workload of rank R of an --of N query-sharded job: ITS contiguous block of the person grid "
                         "(dist.shard_bounds), not --queries persons spread over the whole space; no collectives.  Adds "
                         "config.emulated_rank and the share of 16 x 16-pixel pyramid tiles its samples can touch per layer")
    ap.add_argument("--of", type=int, default=8, help="rank count of --emulate-rank")
    ap.add_argument("--speculative", type=int, default=1,
                    help="query-sharded runs: 1 = the whole forward as one graph, assuming every layer has a valid query "
                         "somewhere, verified after the forward and redone exactly on a miss (dist.SpeculativeShardedDecoder); "
                         "0 = graph segments with a MAX all-reduce of the flag between the layers")
    ap.add_argument("--full", action="store_true",
                    help="also measure what goes beyond the headline figure: the eager per-kernel profile pass (roofline, "
                         "roofline_mfma, kernels, rank_time_split), the rocprofv3 child passes of roofline.traffic, the secondary "
                         "workloads and the CPU oracle baseline; --profile-steps / --traffic / --secondary / --cpu-baseline "
                         "still select among them.  Off (default): set up, warm up, time the steps, print the line")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps write what the timed forward returned in its last step as DIR/<name>.npy "
                         "(float32, at most 64 MB in all: a fixed, seeded sample of the query axis when larger)")
    ap.add_argument("--traffic", default="auto", choices=["auto", "live", "cached", "off"],
                    help="roofline.traffic (HBM bytes per launch of the sampling kernel from the PMC counters): live = two "
                         "rocprofv3 --pmc child passes of this command now (~20 s); cached = the committed "
                         "profiles/*_pmc_msda.json, only if it was measured on these kernel sources (hash) and this "
                         "configuration; auto (default) = with --full live when rocprofv3 is on PATH, else cached, "
                         "without --full off; off = null")
    ap.add_argument("--inside", default="grid", choices=["grid", "all"],
                    help="where the initial query poses sit: grid = the model's 'sample_space' grid over the whole space "
                         "(SURVEY 8(d); ~1/3 of the (view, query) pairs project outside their image and are skipped); all = the "
                         "grid shrunk to 30 %% of the space so that > 99 %% of the pairs are inside every view (nothing skipped: "
                         "the regime of a trained model's later layers)")
    ap.add_argument("--f32-gemm", default="split", choices=["split", "exact"],
                    help="--dtype fp32 only: split = every fp32 operand value as three bf16 parts, six v_mfma_f32_32x32x16_bf16 "
                         "products per 16 k, fp32 accumulation (error against fp64 not above the exact form's, "
                         "profiles/r03_f32_split_gemm.txt); exact = v_mfma_f32_32x32x2_f32, bitwise an fp32 fmaf chain")
    ap.add_argument("--pmc-child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--cpu-baseline", type=int, default=-1, help="-1 = auto: on with --full")
    ap.add_argument("--secondary", type=int, default=-1,
                    help="1 GPU: after the headline's timed region also measure cfg-2 fp32, cfg-4 fp32, cfg-2 --inside all, cfg-5 bf16 "
                         "and cfg-2 bf16 with 2 / 4 samples per forward (>= 10 graph replays each, ~20 s) and attach them as "
                         "`secondary`; N GPUs, query-sharded: also time one-sample-per-rank replicas (`shard_samples`).  -1 = auto: "
                         "on for the default headline command with --full, off without it or when a diagnostic override is given")
    ap.add_argument("--batch", type=int, default=1,
                    help="samples per forward (the decoder batches natively); the headline is quoted at 1")
    ap.add_argument("--profile-steps", type=int, default=-1, help="eager forwards of the per-kernel profile pass; -1 = auto: 5 with --full, else 0")
    args = ap.parse_args()
    if args.profile_steps < 0:
        args.profile_steps = 5 if args.full else 0
    if args.cpu_baseline < 0:
        args.cpu_baseline = int(args.full)
    if args.traffic == "auto" and not args.full:
        args.traffic = "off"

    if args.gpus > 1 and "RANK" not in os.environ and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: start the N ranks ourselves (one process per GPU, rendezvous on 127.0.0.1),
        # exactly the way the driver's torch.distributed.run command does; rank 0's JSON line passes through
        raise SystemExit(self_launch(args.gpus))
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d: launch with torch.distributed.run --nproc-per-node %d (or plainly, "
                         "without RANK/WORLD_SIZE in the environment)" % (args.gpus, world, args.gpus))
    have_gpu = torch.cuda.is_available()
    dev = None
    if have_gpu:
        ndev = torch.cuda.device_count()
        torch.cuda.set_device(local_rank % ndev)
        dev = torch.device("cuda", local_rank % ndev)
    if world > 1:
        # bring-up as lib/models/util/misc.py:504-543 (init_process_group('nccl') from RANK / WORLD_SIZE / LOCAL_RANK)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("MVG_DIST_BACKEND", "nccl")      # "nccl" == RCCL on ROCm; gloo only for plumbing tests
        if backend == "nccl" and have_gpu:
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
        print("# rank %d/%d: process group up (%s)" % (rank, world, dist.get_backend()), file=sys.stderr, flush=True)
    if not have_gpu:
        raise SystemExit("bench.py needs an MI355X (no GPU visible); there is no CPU path")

    from mvgformer_amd import _lib, ops
    from mvgformer_amd import dist as mdist
    from mvgformer_amd.decoder import DecoderContext
    from mvgformer_amd.factory import build_decoder_for_case, case_to_device
    from mvgformer_amd.synthetic import build_case

    arch, cus = _lib.device_info()
    rccl = rccl_preflight(rank, world, dev) if world > 1 else None
    if rccl is not None and not rccl["ok"]:
        raise SystemExit("collective preflight failed: %s" % rccl["error"])
    _lib.check(_lib.load().mvg_set_tuning(b"f32_split", 1 if args.f32_gemm == "split" else 0), "mvg_set_tuning(f32_split)")
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    elem = 2 if args.dtype == "bf16" else 4
    thr = 0.1

    sharded = world > 1 and args.shard == "queries"       # one sample, queries split over the ranks
    replicas = world > 1 and args.shard == "samples"      # one sample per rank
    ref_extent = 0.3 if args.inside == "all" else 1.0
    case = build_case(args.config, B=args.batch, seed=rank if replicas else 0, valid_fraction=args.valid_fraction,
                      NQ=args.queries, ref_extent=ref_extent)
    NQ, J, V, Ly = case.NQ, 15, case.V, case.layers
    cpu_case = None
    if rank == 0 and args.cpu_baseline and world == 1:
        import copy
        cpu_case = copy.copy(case)      # keeps the host tensors; case_to_device() rebinds `case`'s attributes
    dec = build_decoder_for_case(case, dev, dtype)
    g = case_to_device(case, dev)
    emul = args.emulate_rank is not None
    if emul and (world != 1 or not 0 <= args.emulate_rank < args.of):
        raise SystemExit("--emulate-rank R --of N needs one GPU and 0 <= R < N")
    sh_world, sh_rank = (args.of, args.emulate_rank) if emul else ((world, rank) if sharded else (1, 0))
    lo, hi = mdist.shard_bounds(NQ, sh_world, sh_rank)
    tgt, qpos, ref, _ = mdist.shard_queries(g.tgt, g.query_pos, g.reference_points, J, sh_world, sh_rank)
    if sharded:
        mdist.install_any_valid_sync(dec, None)

    # host-side, per-sample preparation that belongs to data loading (camera records)
    ctx = DecoderContext.prepare(g.spatial_shapes, g.level_start_index, g.meta, case.img_size, dtype, args.batch, dev)

    src_views = g.src_views
    if args.producer == "nhwc":
        src_views = [s.to(dtype).to(memory_format=torch.channels_last) for s in g.src_views]
    elif args.producer == "inplace":
        src_views = ctx.pyramid_buffers(channels=g.src_views[0].shape[1])
        for dst, s in zip(src_views, g.src_views):
            dst.copy_(s)

    def forward():
        ctx.feat = None
        out = dec(tgt, ref, src_views, g.meta, g.spatial_shapes, g.level_start_index, None, query_pos=qpos,
                  threshold=thr, context=ctx)
        if sharded:
            out = mdist.gather_outputs(out, NQ, J, None, gather_hidden=False)
        return out

    pose_recv = None

    def exchange_poses(o):
        """replica mode: the final pose sets of all ranks' samples on every rank (one small all-gather per step)"""
        nonlocal pose_recv
        send = torch.cat([o[1][-1].reshape(-1), o[4][-1].reshape(-1)])
        if pose_recv is None:
            pose_recv = send.new_empty((world * send.numel(),))
        dist.all_gather_into_tensor(pose_recv, send)

    use_graph = True if args.graph < 0 else bool(args.graph)
    graph = None
    with torch.no_grad():
        for _ in range(3):
            out = forward()
        torch.cuda.synchronize()
        if args.pmc_child:      # counter-collection child of measure_traffic_live: eager forwards only
            for _ in range(3):
                forward()
            torch.cuda.synchronize()
            return
        if use_graph and sharded:
            # segments between the collectives are graphs, the RCCL calls stay eager (mvgformer_amd.dist)
            for layer in dec.layers:
                layer._any_valid_hook = None
            ok = 1
            try:
                runner_cls = mdist.SpeculativeShardedDecoder if args.speculative else mdist.GraphedShardedDecoder
                graph = runner_cls(dec, tgt, ref, src_views, qpos, ctx, thr, NQ)
            except Exception as e:   # keep the job alive: every rank falls back to the eager sharded forward
                print("# rank %d: segmented graph capture failed (%s: %s)" % (rank, type(e).__name__, e), file=sys.stderr)
                ok, graph = 0, None
                torch.cuda.synchronize()
            flag = torch.tensor([ok], dtype=torch.int32, device=dev)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            if int(flag.item()) == 0:
                graph = None
                mdist.install_any_valid_sync(dec, None)
            else:
                out = graph.replay()
                torch.cuda.synchronize()
        elif use_graph:
            try:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    out = forward()
                graph.replay()
                torch.cuda.synchronize()
            except Exception as e:   # capture not possible (e.g. collective in capture): run eagerly
                if rank == 0:
                    print("# graph capture failed (%s: %s); running eagerly" % (type(e).__name__, e), file=sys.stderr)
                graph = None
                torch.cuda.synchronize()
        step = (lambda: graph.replay()) if graph is not None else forward
        extra = []
        if args.inflight > 1:
            if sharded or graph is None or args.producer != "nchw":
                raise SystemExit("--inflight needs HIP graphs, the default producer and no query sharding")
            # more samples in flight: own decoder instance (own vh / G buffers), own stream, own graph each; the graphs
            # hold raw pointers, so `extra` keeps their owners alive
            for k in range(args.inflight):
                if k == 0:          # the decoder built above, re-captured on its own stream like the others
                    case_k, dec_k, g_k, ctx_k = case, dec, g, ctx
                else:
                    case_k = build_case(args.config, seed=1000 * k + rank, valid_fraction=args.valid_fraction,
                                        ref_extent=ref_extent)
                    dec_k = build_decoder_for_case(case_k, dev, dtype)
                    g_k = case_to_device(case_k, dev)
                    ctx_k = DecoderContext.prepare(g_k.spatial_shapes, g_k.level_start_index, g_k.meta, case_k.img_size,
                                                   dtype, 1, dev)

                def fwd_k(dec_k=dec_k, g_k=g_k, ctx_k=ctx_k):
                    ctx_k.feat = None
                    return dec_k(g_k.tgt, g_k.reference_points, g_k.src_views, g_k.meta, g_k.spatial_shapes,
                                 g_k.level_start_index, None, query_pos=g_k.query_pos, threshold=thr, context=ctx_k)
                torch.cuda.synchronize()
                s_k = torch.cuda.Stream()    # never the NULL stream: it would order the replays one after the other
                with torch.cuda.stream(s_k):
                    for _ in range(3):
                        fwd_k()
                    s_k.synchronize()
                    graph_k = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph_k, stream=s_k):
                        out_k = fwd_k()
                extra.append((s_k, graph_k, out_k, dec_k, g_k, ctx_k, case_k))
            torch.cuda.synchronize()
            out = extra[0][2]

            def step():
                for slot in extra:
                    with torch.cuda.stream(slot[0]):
                        slot[1].replay()
        if replicas:
            inner = step

            def step():
                res = inner()
                exchange_poses(out if graph is not None else res)
                return res

        for _ in range(args.warmup):
            step()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        # every step also gets its own HIP-event pair on the launch stream (median of the device-synchronised
        # iterations); the wall clock around all K steps stays the contract's timed region and gives `value`
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)] if args.inflight == 1 else None
        t0 = time.perf_counter()
        if evs:
            evs[0].record()
        last = None
        for i in range(args.steps):
            last = step()
            if evs:
                evs[i + 1].record()
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        elapsed = time.perf_counter() - t0
        step_ms = sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(args.steps)) if evs else None
        if world > 1:
            tmax = torch.tensor([elapsed], dtype=torch.float64, device=dev)
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            elapsed = float(tmax.item())
        if last is not None:        # eager steps return their outputs; a replayed graph refreshes `out` in place
            out = last
        dumped = dump_outputs(out, args.dump_outputs) if (args.dump_outputs and rank == 0) else None

        # ---- per-kernel timing (HIP events on the launch stream), eager, outside the timed region
        prof = {}
        live_frac = None
        exec_rows_a = None
        if sharded:
            mdist.install_any_valid_sync(dec, None)
        if args.profile_steps > 0:                 # every rank runs it (the sharded forward contains collectives)
            if rank == 0:
                ops.PROFILE = {}
            # kernels are timed one at a time: the side-stream issue of the pyramid GEMMs is off for this pass, so
            # that the roofline figure is the sampling kernel's own duration (as in the rocprofv3 kernel trace of
            # tools/prof.sh), not its duration while sharing the GPU with a GEMM
            overlap, dec.overlap_pyramid = getattr(dec, "overlap_pyramid", False), False
            for _ in range(args.profile_steps):
                forward()
            torch.cuda.synchronize()
            if rank == 0:
                prof = ops.profile_summary()
                ops.PROFILE = None
            # fraction of (image, query) pairs inside their image, per sampling launch (the others are skipped): one more eager
            # forward, outside the timed pass, for the L1-path figure of the roofline object
            live_fracs = []
            exec_rows_a = []        # per sampling launch: rows of the 128-row chain-A tiles that hold an in-image pair (per image)
            originals = {}

            def counting(name):
                orig = originals[name] = getattr(ops, name)

                def wrapped(*a, **kw):
                    mask = kw.get("pair_mask")
                    if mask is not None:
                        live_fracs.append(mask.float().mean())
                        per_img = mask.view(args.batch * V, -1).sum(1, dtype=torch.int64)
                        exec_rows_a.append(((per_img + 127) // 128 * 128).clamp(max=mask.numel() // (args.batch * V)).sum())
                    return orig(*a, **kw)
                setattr(ops, name, wrapped)
            for name in ("msda_gsamp", "msda_gfused_f32"):
                counting(name)
            try:
                forward()
                torch.cuda.synchronize()
            finally:
                for name, orig in originals.items():
                    setattr(ops, name, orig)
            dec.overlap_pyramid = overlap
            live_frac = float(torch.stack(live_fracs).mean()) if live_fracs else None
            exec_rows_a = [int(x) for x in exec_rows_a] if len(exec_rows_a) == Ly else None
            # the grouped pyramid products of the timed schedule (DQDecoder.launch_pyramid_projections), each launch alone
            if rank == 0 and hasattr(dec, "pyramid_launches") and ctx.feat is not None and ctx.feat.dtype == torch.bfloat16:
                launches = dec.pyramid_launches(ctx)
                if launches:
                    ops.PROFILE = {}
                    for _ in range(args.profile_steps):
                        for grp, slots in launches:
                            jobs = []
                            for layer in grp:
                                jobs += layer.proj_attn.pyramid_jobs(ctx.feat)
                            ops.pyramid_group_ws(ctx.feat, jobs, slots=slots,
                                                 label="pyramid_group_ws_%d%s" % (len(jobs), "_jit" if slots else ""))
                    torch.cuda.synchronize()
                    prof.update(ops.profile_summary())
                    ops.PROFILE = None

    default_headline = (args.config == "cfg2" and args.dtype == "bf16" and args.queries is None and args.valid_fraction is None
                        and args.inside == "grid" and args.inflight == 1 and args.batch == 1 and args.producer == "nchw"
                        and args.emulate_rank is None)
    want_secondary = (default_headline and args.full) if args.secondary < 0 else bool(args.secondary)
    secondary = {}
    if want_secondary and sharded:
        # the weak-scaling number next to the strong-scaling one, in the same job (collective: every rank takes part)
        try:
            secondary["shard_samples"] = measure_replicas(args.config, args.dtype, rank, world, dev, args.steps, args.warmup)
        except Exception as e:
            secondary["shard_samples"] = {"error": "%s: %s" % (type(e).__name__, e)}
            print("# rank %d: replica measurement failed: %s" % (rank, secondary["shard_samples"]["error"]), file=sys.stderr)

    if rank != 0:
        if world > 1:
            dist.destroy_process_group()
        return

    refs = out[1]
    assert torch.isfinite(refs).all(), "non-finite poses"
    ms_mean = elapsed / args.steps * 1e3
    if step_ms and world == 1:
        n = len(step_ms)
        ms_per_step = step_ms[n // 2] if n % 2 else 0.5 * (step_ms[n // 2 - 1] + step_ms[n // 2])
    else:
        ms_per_step = ms_mean          # N > 1: the contract's max-over-ranks wall clock
    value = (world if replicas else 1) * args.inflight * args.batch * args.steps / elapsed   # samples / s of the whole job

    # roofline of the dominant kernel: one sampling-kernel launch covers all V views of one layer
    Lq_loc = (hi - lo) * J
    S = int(sum(h * w for h, w in case.shapes))
    bytes_launch = args.batch * V * algorithmic_bytes_per_view_layer(S, 256, Lq_loc, 8, len(case.shapes), 8, elem)
    roof = None
    # HBM-side bytes of the same kernel from the PMC counters (FETCH_SIZE x2 per the gfx950 correction + WRITE_SIZE).  Either
    # measured by this run (two rocprofv3 child passes of the same command) or the committed figure of tools/prof.sh --
    # quoted only for the kernel sources (hash) and configuration it was measured on; the line says which.
    traffic, traffic_source = None, None
    in_forward = None
    issue_shares = None
    # the dominant kernel: the G-sampling kernel (bf16), its fp32 twin or the generic fused sampling kernel; its algorithmic
    # bytes are SURVEY 8(d)'s sampling figure in all three cases
    kernel_names = {"msda_gsamp": "msda_gsamp_kernel",
                    "msda_gfused_f32": "msda_gfused_f32_hp_kernel", "msda_fused": "msda_fused_kernel"}
    samp_key = next((k for k in kernel_names if k in prof), "msda_fused")
    samp_name = sampler_kernel_name(samp_key, args.batch * V * NQ * J)
    if world == 1 and args.traffic != "off" and args.inflight == 1:
        src_hash = sampler_source_hash()
        want = {"config": args.config, "dtype": args.dtype, "queries": NQ, "valid_fraction": args.valid_fraction,
                "src_sha256": src_hash, "inside": args.inside}
        import glob
        import shutil
        mode = args.traffic
        if mode == "auto":
            mode = "live" if shutil.which("rocprofv3") else "cached"
        if mode == "cached":
            for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_msda.json")), reverse=True):
                with open(path) as f:
                    rec = json.load(f)
                if all(rec.get(k) == v for k, v in want.items()):
                    traffic = int(rec["traffic_bytes_per_launch"])
                    traffic_source = "%s (tools/prof.sh, sources %s)" % (os.path.relpath(path, ROOT), src_hash)
                    break
        if traffic is None and mode == "live":
            tail = ["--config", args.config, "--dtype", args.dtype, "--producer", args.producer, "--cpu-baseline", "0",
                    "--inside", args.inside, "--f32-gemm", args.f32_gemm]
            if args.queries is not None:
                tail += ["--queries", str(args.queries)]
            if args.valid_fraction is not None:
                tail += ["--valid-fraction", str(args.valid_fraction)]
            traffic, detail = measure_traffic_live(tail, samp_name)
            in_forward = measure_sampler_in_forward(tail, samp_name, Ly) if args.batch == 1 else None
            issue_shares = measure_issue_shares(tail, samp_name)
            traffic_source = ("measured in this run: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE child passes, %s" % json.dumps(detail)
                              if traffic is not None else "unavailable: %s" % detail)
        elif traffic is None:
            traffic_source = "no committed PMC profile for these kernel sources (%s) and this configuration" % src_hash
    if samp_key in prof:
        n, ms = prof[samp_key]
        ach = bytes_launch / (ms * 1e-3) / 1e9
        roof = {"bound": "hbm", "kernel": samp_name, "achieved": round(ach, 1), "peak": 8000.0,
                "unit": "GB/s", "frac": round(ach / 8000.0, 4), "traffic": traffic, "traffic_source": traffic_source,
                # share of the (view, query) pairs whose reference point is inside their image, averaged over the layers'
                # launches: the bf16 kernel zero-fills the others without sampling (the consumer multiplies their rows by 0,
                # dq_decoder.py:585-586); `achieved` prices ALL pairs at SURVEY 8(d)'s bytes.  --inside all = nothing skipped
                "in_image_pair_fraction": None if live_frac is None else round(live_frac, 4),
                "pairs_skipped": bool(samp_key in ("msda_gsamp", "msda_gfused_f32")),
                "avg_launch_us": round(ms * 1e3, 2), "launches_timed": n, "algorithmic_bytes_per_launch": bytes_launch,
                # SURVEY 8(d) optional: value read once + output written once (locations / weights never hit HBM here)
                "fused_minimum_bytes_per_launch": args.batch * V * (S * 256 + Lq_loc * 256) * elem}
        if in_forward is not None:
            # the same kernel inside the graph-replayed forward (rocprofv3 --kernel-trace child pass): there its value planes and G
            # were written just before it (Infinity-Cache hits) and it runs shorter than alone; `achieved` / `frac` above keep the
            # kernel-alone duration that profiles/*_kernel_stats.csv reports
            if in_forward[0] is not None:
                roof["in_forward"] = {"avg_launch_us": round(in_forward[0], 2), "launches": in_forward[1],
                                      "achieved": round(bytes_launch / (in_forward[0] * 1e-6) / 1e9, 1),
                                      "frac": round(bytes_launch / (in_forward[0] * 1e-6) / 1e9 / 8000.0, 4),
                                      "source": "rocprofv3 --kernel-trace child pass over 8 graph replays of this configuration"}
                # flat copies: a parser that keeps scalars only must not lose them
                roof["in_forward_us"] = roof["in_forward"]["avg_launch_us"]
                roof["in_forward_frac"] = roof["in_forward"]["frac"]
            else:
                roof["in_forward"] = {"unavailable": in_forward[1]}
        if issue_shares is not None:
            if issue_shares[0] is not None:
                roof.update(issue_shares[0])      # valu_busy, l1_addr_busy (the share that binds: profiles/r06_experiments.txt), ...
            else:
                roof["issue_shares_unavailable"] = issue_shares[1]
        if samp_key == "msda_gsamp":
            # The roof this kernel actually runs against: its gathers are served by the L1s, which deliver
            # 55-57 B/clk/CU = ~35 TB/s to loads of this shape (tools/probes/l1_gather_probe).  Bytes delivered to the lanes per
            # launch: every in-image (pair, head) gathers L*P samples x 4 corners x 64 B of value rows + 4 corners x 9 x 16 B of G.
            live = live_frac if live_frac is not None else 1.0
            n_lv, n_pt, n_head = len(case.shapes), 8, 8
            per_unit = n_lv * n_pt * 4 * 64 + 4 * 9 * 16
            delivered = int(args.batch * V * Lq_loc * n_head * per_unit * live)
            l1_peak = 57.0 * 256 * 2.4           # GB/s: 57 B/clk/CU x 256 CUs x 2.4 GHz
            roof["l1_path"] = {"delivered_bytes_per_launch": delivered, "in_image_pair_fraction": round(live, 4),
                               "achieved": round(delivered / (ms * 1e-3) / 1e9, 1), "peak": round(l1_peak, 1), "unit": "GB/s",
                               "frac": round(delivered / (ms * 1e-3) / 1e9 / l1_peak, 4),
                               "note": "binding roof of the gather kernel: what the L1s deliver to 16-byte-per-lane gathers (one wave "
                                       "instruction per 16 clk, tools/probes/l1_gather_probe); pairs outside their image are skipped"}
    # the MFMA regime: dense flops of the forward against the dense bf16 peak (2.5 PF; the fp32 path's kernels
    # run three fp16 MFMA products per fp32 product: priced at their fp32-equivalent flops against the same peak)
    roof_mfma = None
    if prof:
        fl = dense_flops(S, 256, Lq_loc, 8, len(case.shapes), 8, 1024, V, args.batch, Ly, exec_rows_a)
        per_kernel = {}

        def add(name, key, gflop, launches_per_forward):
            if key in prof and prof[key][1] > 0:
                us = prof[key][1] * 1e3
                per_kernel[name] = {"gflop": round(gflop / 1e9, 2), "us": round(us, 2), "tflops": round(gflop / us / 1e6, 1),
                                    "frac": round(gflop / us / 1e6 / 2500.0, 4), "launches_per_forward": launches_per_forward}
        add("chain_a", "chain_attn_pose", fl["chain_a"], Ly)
        add("chain_b", "chain_update_ffn_class", fl["chain_b"] + fl["query_term"], Ly)
        add("chain_a", "chain_attn_pose_f32h", fl["chain_a"], Ly)                     # fp32: the two-part fp16 kernels
        add("chain_b", "chain_update_ffn_class_f32h", fl["chain_b"] + fl["query_term"], Ly)
        add("pyramid_value_and_G", "pyramid_f32h", fl["value"] + fl["G"], Ly)
        add("value_proj", "value_proj_ws", fl["value"], Ly)
        add("feat_linear", "feat_linear_ws", fl["G"], Ly)
        add("pyramid_group_first_layer", "pyramid_group_ws_2", fl["value"] + fl["G"], 1)
        add("pyramid_group_one_layer_just_in_time", "pyramid_group_ws_2_jit", fl["value"] + fl["G"], Ly)
        for nj in (4, 6, 8):
            add("pyramid_group_%d_layers" % (nj // 2), "pyramid_group_ws_%d" % nj, (fl["value"] + fl["G"]) * (nj // 2), 1)
        roof_mfma = {"bound": "mfma", "peak": 2500.0, "unit": "TFLOP/s", "flops_nominal": fl["nominal"], "flops_executed": fl["executed"],
                     "flops_per_step": fl["executed"], "achieved_tflops": round(fl["executed"] / (ms_per_step * 1e-3) / 1e12, 1),
                     "frac": round(fl["executed"] / (ms_per_step * 1e-3) / 1e12 / 2500.0, 4),
                     "nominal_tflops": round(fl["nominal"] / (ms_per_step * 1e-3) / 1e12, 1), "per_kernel": per_kernel,
                     "note": "whole forward: executed dense flops / ms_per_step; per kernel: each launch timed alone (HIP events).  "
                             "nominal = SURVEY 8(d)'s table (reference decomposition); executed = this build's GEMMs: the offsets / "
                             "logits Linear on the pyramid (G) + the query term instead of on V*Lq*L gathered rows, chain A only on "
                             "tiles with an in-image pair; chain_b includes the next layer's query term"}
    kern = {k: {"launches": n, "avg_us": round(ms * 1e3, 2)} for k, (n, ms) in sorted(prof.items())}
    # per-rank time split (kernel time per forward from the eager profile pass, each kernel alone): "fixed" = work that does
    # not shrink when the queries are sharded (pyramid packing + the query-independent pyramid GEMMs, replicated on every
    # rank), "variable" = everything proportional to this rank's queries
    split = None
    if prof and args.profile_steps > 0:
        n_pyr = args.batch * V * S          # rows of the pyramid GEMMs: query-independent whatever the path (fp32: plain linears)
        grouped = any(k.startswith("pyramid_group_ws_") for k in prof)    # the timed schedule's launches replace the per-product ones
        fixed_keys = ("pack_level", "pack_level_nhwc", "pyramid_all_layers", "pyramid_f32h") + (
            tuple(k for k in prof if k.startswith("pyramid_group_ws_")) if grouped else ("value_proj_ws", "feat_linear_ws")) + (
                      "linear_%dx256x256" % n_pyr, "linear_%dx192x256" % n_pyr)
        skip = ("value_proj_ws", "feat_linear_ws") if grouped else ()
        fx = sum(n * ms for k, (n, ms) in prof.items() if k in fixed_keys) / args.profile_steps
        var = sum(n * ms for k, (n, ms) in prof.items() if k not in fixed_keys and k not in skip) / args.profile_steps
        split = {"fixed_us": round(fx * 1e3, 1), "variable_us": round(var * 1e3, 1),
                 "note": "rank 0, kernels timed one at a time; fixed = replicated query-independent work"}

    touched = None
    if emul:
        # Which part of the pyramid can this rank's samples touch?  Per layer: the reference points it projects (the initial grid
        # block, then its own previous layer's output points) -> 16 x 16-pixel tiles of every level within the offsets' reach
        # (+- 8 cells: the rays of projattn.py:98-108) of an in-image projection, as a share of each level's tiles, weighted by pixels.
        with torch.no_grad():
            outs = forward()
            pts = [ref] + [outs[1][l] for l in range(Ly - 1)]
            shp = [(int(h), int(w)) for h, w in g.spatial_shapes.tolist()]
            per_layer = []
            for X in pts:
                r_, _, ins_ = ops.project(X.reshape(args.batch, -1, 3).float().contiguous(), ctx.cams, ctx.levels, V, args.batch)
                num = den = 0.0
                for (Hl, Wl) in shp:
                    th, tw = -(-Hl // 16), -(-Wl // 16)
                    px = r_[..., 0] * Wl
                    py = r_[..., 1] * Hl
                    hit = torch.zeros((r_.shape[0], th, tw), dtype=torch.bool, device=dev)
                    for dy in (-9, 0, 9):
                        for dx in (-9, 0, 9):
                            tx = ((px + dx) // 16).long().clamp(0, tw - 1)
                            ty = ((py + dy) // 16).long().clamp(0, th - 1)
                            img = torch.arange(r_.shape[0], device=dev)[:, None].expand_as(tx)
                            m = ins_.view(r_.shape[0], -1).bool()
                            hit[img[m], ty[m], tx[m]] = True
                    num += float(hit.float().mean()) * Hl * Wl
                    den += Hl * Wl
                per_layer.append(round(num / den, 4))
            touched = {"per_layer": per_layer, "note": "share of the pyramid's pixels in 16 x 16 tiles within +- 9 cells of an in-image reference "
                       "point of this rank's queries (layer l: the points layer l projects)"}

    if want_secondary and world == 1:
        # the other named workloads, driver-witnessed: same process, same command, after the headline's timed region
        for name, cfg_name, dt_name, inside, batch in SECONDARY:
            try:
                t_sec = time.perf_counter()
                secondary[name] = measure_secondary(cfg_name, dt_name, inside, batch, dev)
                secondary[name]["wall_s"] = round(time.perf_counter() - t_sec, 1)
            except Exception as e:      # a secondary workload must never cost the headline line
                secondary[name] = {"error": "%s: %s" % (type(e).__name__, e)}
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
        if roof is not None and "frac" in secondary.get("cfg2_bf16_inside_all", {}):
            # the sampler's figure with nothing skipped (every pair inside its image), next to the headline's: VERDICT r5 weak 10a
            roof["frac_inside_all"] = secondary["cfg2_bf16_inside_all"]["frac"]
        try:
            t_sec = time.perf_counter()
            secondary["train_step_cfg2_fp32"] = measure_train_step(dev)
            secondary["train_step_cfg2_fp32"]["wall_s"] = round(time.perf_counter() - t_sec, 1)
        except Exception as e:
            secondary["train_step_cfg2_fp32"] = {"error": "%s: %s" % (type(e).__name__, e)}
            torch.cuda.synchronize()
            torch.cuda.empty_cache()

    cpu = None
    if cpu_case is not None:
        from mvgformer_amd.synthetic import to_torch_state
        from oracle import decoder_ref as O
        # threads actually used: the oracle's torch CPU ops stop scaling past ~32 threads (measured on the
        # 2 x 64-core GPU-box host: 16 thr 5.3 s, 32 thr 4.8 s, 64 thr 6.9 s, 256 thr 259 s per layer)
        ncore = min(os.cpu_count() or 1, 32)
        torch.set_num_threads(ncore)
        prm = to_torch_state(cpu_case.weights)
        tgt_c, ref_c = cpu_case.tgt.cpu(), cpu_case.reference_points.cpu()
        done, t_cpu = 0, 0.0
        with torch.no_grad():
            while done < Ly and (done == 0 or t_cpu / done * (done + 1) < 30.0):   # bounded: <= ~30 s of CPU work
                t0 = time.perf_counter()
                tgt_c, ref_c = O.decoder_layer_forward(
                    prm, "layers.%d." % done, tgt_c, cpu_case.query_pos.cpu(), ref_c, cpu_case.src_views,
                    cpu_case.spatial_shapes.cpu(), cpu_case.level_start_index.cpu(), cpu_case.meta, cpu_case.img_size,
                    threshold=thr)[:2]
                t_cpu += time.perf_counter() - t0
                done += 1
        cpu = {"value": round(done / (t_cpu * Ly), 5), "unit": "samples/s", "cores": ncore, "kind": "port",
               "sample": "oracle/decoder_ref.py fp32 (torch CPU ops, %d threads): %d of %d layers of the same workload "
                         "(all %d views, all %d queries) in %.1f s%s"
                         % (ncore, done, Ly, V, NQ, t_cpu, "" if done == Ly else ", scaled x%.2f" % (Ly / done))}

    line = {
        "metric": "decoder samples/sec (5-view, 1024 queries, 4 layers)" if (args.config in ("cfg2", "cfg3") and args.queries is None)
        else "decoder samples/sec (%s)" % args.config,
        "value": round(value, 3), "unit": "samples/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 4), "ms_per_step_mean": round(ms_mean, 4),
        "ms_per_step_note": "ms_per_step = median of the K per-step HIP-event intervals on the launch stream (1 GPU; SURVEY 8(d)); "
                            "ms_per_step_mean = wall clock of the timed region / K, what `value` is computed from",
        "ms_per_step_min_max": None if not step_ms else [round(step_ms[0], 4), round(step_ms[-1], 4)],
        "higher_is_better": True,
        "scaling": "strong" if sharded else ("weak" if replicas else None),
        "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
        "config": {"workload": "%s: %d views, %d queries x %d joints, %d decoder layers, maps %s x 256ch, "
                               "all queries valid" % (args.config, V, NQ, J, Ly, case.shapes)
                   if args.valid_fraction is None else
                   "%s: %d views, %d queries x %d joints, %d layers, ~%.0f%% queries valid"
                   % (args.config, V, NQ, J, Ly, 100 * args.valid_fraction),
                   "parallelism": ("queries sharded x%d + all-gather%s" % (world, " (one graph, speculative any-valid flag)"
                                                                            if (args.speculative and graph is not None) else "")
                                   if sharded else
                                   "one sample per GPU x%d + all-gather of the pose sets" % world if replicas else "single GPU"),
                   "pyramid_handoff": {"nchw": "NCHW fp32 (reference producer format), packed per step",
                                       "nhwc": "channels-last %s, copied per step" % args.dtype,
                                       "inplace": "produced in the packed layout (no per-step pack)"}[args.producer],
                   "initial_poses": {"grid": "'sample_space' grid over the whole space (SURVEY 8(d))",
                                     "all": "grid over 30 % of the space: > 99 % of the (view, query) pairs inside their image"}[args.inside],
                   "samples_in_flight": args.inflight, "samples_per_forward": args.batch,
                   **({"emulated_rank": "%d of %d: persons %d..%d of %d (contiguous block of the grid), no collectives" % (
                       args.emulate_rank, args.of, lo, hi - 1, NQ), "touched_pyramid_share": touched} if emul else {}),
                   **({"fp32_gemm": {"split": "fused kernels (pyramid products, chains A / B): operands scaled per row / tensor by a power of two and "
                                              "split into 2 fp16 parts, 3 fp16 MFMA products, fp32 accumulate; the first layer's query term: 3 "
                                              "bf16 parts, 6 bf16 MFMA products",
                                     "exact": "v_mfma_f32_32x32x2_f32 (fmaf chain)"}[args.f32_gemm]}
                      if args.dtype == "fp32" else {}),
                   "hip_graph": graph is not None, "device": arch, "cus": cus},
        "roofline": roof, "roofline_mfma": roof_mfma, "cpu_baseline": cpu, "rank_time_split": split, "kernels": kern,
        "secondary": secondary or None, "rccl": rccl, "full": args.full,
        **({"dumped_outputs": {"dir": args.dump_outputs, "shapes": dumped}} if dumped is not None else {}),
    }
    print(json.dumps(line))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
