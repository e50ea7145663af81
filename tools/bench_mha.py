"""Time of the query self-attention kernel (ops.self_attention, csrc/mha.hip) at the cfg-2 shape -- B = 1, Lq = 1024 x 15 =
15 360 tokens, 8 heads of 32 -- in both arithmetic variants, next to torch.nn.functional.scaled_dot_product_attention on the SAME
tensors, dtype and card, and of the whole attended block (DQDecoderLayer.attend_queries: in-projection, attention, out-projection,
residual + LayerNorm).

Device time between events around `--inner` back-to-back launches, the two implementations alternating inside one process,
medians over `--reps` such windows after `--warmup` windows.  torch's op is given the (B, Lq, C) tensors as strided (B, M, Lq, D)
views (no copy: what a caller of this library would hand it) and, separately, contiguous (B, M, Lq, D) copies made outside the
timed window; the better of the two is what the kernel is compared with.  FLOP/s: 4 Lq^2 D M B operations over the time.
Prints one JSON line at the end.

    python tools/bench_mha.py [--lq 15360] [--batch 1] [--reps 20] [--inner 5] [--warmup 3] [--only bf16] [--sdpa 0] [--block 0]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda:0"
C, M, D = 256, 8, 32


def _window(fn, inner):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(inner):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / inner


def _alternate(fns, reps, inner, warm):
    """{name: [ms per call]}: the candidates take turns window by window"""
    times = {k: [] for k in fns}
    dead = {}
    for i in range(warm + reps):
        for name, fn in fns.items():
            if name in dead:
                continue
            try:
                ms = _window(fn, inner)
            except RuntimeError as e:           # torch's op has no kernel for this dtype / shape on this build: said, not hidden
                if i > 0 or "HIP error" in str(e) or "illegal" in str(e):
                    raise                       # anything but a refusal at the first call ends the run
                dead[name] = str(e).splitlines()[0][:160]
                continue
            if i >= warm:
                times[name].append(ms)
    return times, dead


def _stat(xs):
    return dict(median_ms=statistics.median(xs), min_ms=min(xs), max_ms=max(xs), windows=len(xs)) if xs else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lq", type=int, default=15360)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["both", "bf16", "fp32"], default="both")
    ap.add_argument("--sdpa", type=int, default=1, help="0: time the kernel alone (a counter run)")
    ap.add_argument("--block", type=int, default=1, help="0: skip the whole attended block")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mha: no GPU -- nothing is measured")
    from mvgformer_amd import ops
    from mvgformer_amd.decoder import DQDecoderLayer
    B, Lq = a.batch, a.lq
    flop = 4.0 * Lq * Lq * D * M * B
    result = dict(tool="bench_mha", device=torch.cuda.get_device_name(0), B=B, Lq=Lq, heads=M, head_dim=D, gflop=flop / 1e9)
    gen = torch.Generator(device=DEV).manual_seed(0)
    for dt, tag in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
        if a.only not in ("both", tag):
            continue
        q, k, v = (torch.randn(B, Lq, C, device=DEV, generator=gen).to(dt) for _ in range(3))
        heads = lambda t: t.view(B, Lq, M, D).transpose(1, 2)                     # (B, M, Lq, D), strided
        qs, ks, vs = heads(q), heads(k), heads(v)
        qc, kc, vc = (t.contiguous() for t in (qs, ks, vs))
        fns = {"mvg_self_attention": lambda: ops.self_attention(q, k, v),
               "torch sdpa (strided views)": lambda: F.scaled_dot_product_attention(qs, ks, vs),
               "torch sdpa (contiguous heads)": lambda: F.scaled_dot_product_attention(qc, kc, vc)}
        if not a.sdpa:
            fns = {"mvg_self_attention": fns["mvg_self_attention"]}
        inner = a.inner if dt == torch.bfloat16 else max(1, a.inner // 2)
        times, dead = _alternate(fns, a.reps, inner, a.warmup)
        out = ops.self_attention(q, k, v)
        agree = None
        if a.sdpa and "torch sdpa (contiguous heads)" not in dead:
            want = F.scaled_dot_product_attention(qc, kc, vc).transpose(1, 2).reshape(B, Lq, C)
            agree = float((out.float() - want.float()).abs().max())
        print("%s  B=%d Lq=%d  (%.1f GFLOP)   max |mvg - torch| %s" % (tag, B, Lq, flop / 1e9, "n/a" if agree is None else "%.3e" % agree))
        entry = dict(max_abs_diff_vs_torch=agree)
        for name in fns:
            st = _stat(times[name])
            if st is None:
                print("    %-32s not measured: %s" % (name, dead.get(name, "no window")))
                entry[name] = dict(error=dead.get(name))
                continue
            st["tflops"] = flop / (st["median_ms"] * 1e-3) / 1e12
            print("    %-32s median %8.3f ms  min %8.3f  max %8.3f  %7.1f TFLOP/s  (%d windows of %d)"
                  % (name, st["median_ms"], st["min_ms"], st["max_ms"], st["tflops"], st["windows"], inner))
            entry[name] = st
        best = [entry[n]["median_ms"] for n in list(fns)[1:] if "median_ms" in entry[n]]
        if best and "median_ms" in entry["mvg_self_attention"]:
            entry["mvg_over_best_torch"] = entry["mvg_self_attention"]["median_ms"] / min(best)
            print("    mvg / best torch: %.3f" % entry["mvg_over_best_torch"])
        result[tag] = entry
        if not a.block:
            continue
        # the whole block at the head of the layer
        layer = DQDecoderLayer([8000.0, 8000.0, 2000.0], [0.0, -500.0, 800.0], [960, 512], 3, n_levels=1, n_points=8,
                               projattn_posembed_mode="ablation_not_use_rayconv", init_self_attention=True).to(DEV).eval()
        layer.set_compute_dtype(dt)
        tgt, pos = (torch.randn(B, Lq, C, device=DEV, generator=gen) for _ in range(2))
        with torch.no_grad():
            layer.attend_queries(tgt, pos)
            blk, _ = _alternate({"block": lambda: layer.attend_queries(tgt, pos)}, a.reps, inner, a.warmup)
        st = _stat(blk["block"])
        print("    %-32s median %8.3f ms  min %8.3f  max %8.3f" % ("attend_queries (whole block)", st["median_ms"], st["min_ms"], st["max_ms"]))
        entry["attend_queries_block"] = st
    print(json.dumps(result))


if __name__ == "__main__":
    main()
