"""Time of the self-attention TRAINING kernels (ops.self_attention_train + ops.self_attention_backward, csrc/mha.hip) at the cfg-2
shape -- B = 1, Lq = 1024 x 15 = 15 360 tokens, 8 heads of 32 -- next to torch.nn.functional.scaled_dot_product_attention forward +
backward on the SAME tensors, dtype and card, with and without attention dropout, and of the whole block
(DQDecoderLayer._attend_queries_autograd forward + backward) under both backends.

Device time between events around `--inner` back-to-back forward + backward pairs, the implementations alternating inside one
process, medians over `--reps` such windows after `--warmup` windows; torch.cuda.max_memory_allocated of each candidate over one
pair on its own (the inputs, which both share, included).  torch's op gets contiguous (B, M, Lq, D) heads made outside the timed
window (its better case, tools/bench_mha.py).  FLOP count: 4 Lq^2 D M B forward and 2.5 x that backward (five products; the native
backward recomputes two of them on top).  Prints one JSON line at the end.

    python tools/bench_mha_train.py [--lq 15360] [--batch 1] [--reps 20] [--inner 3] [--warmup 3] [--only bf16] [--torch 0] [--block 0]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_mha import C, D, DEV, M, _alternate, _stat  # noqa: E402


def _peak(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() / 2 ** 20


def _report(entry, name, times, dead, inner, flop=None):
    st = _stat(times[name])
    if st is None:
        print("    %-44s not measured: %s" % (name, dead.get(name, "no window")))
        entry[name] = dict(error=dead.get(name))
        return
    if flop:
        st["tflops"] = flop / (st["median_ms"] * 1e-3) / 1e12
    print("    %-44s median %8.3f ms  min %8.3f  max %8.3f%s  (%d windows of %d)"
          % (name, st["median_ms"], st["min_ms"], st["max_ms"], "  %7.1f TFLOP/s" % st["tflops"] if flop else "", st["windows"], inner))
    entry[name] = st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lq", type=int, default=15360)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["both", "bf16", "fp32"], default="both")
    ap.add_argument("--torch", type=int, default=1, help="0: time the native kernels alone (a counter run)")
    ap.add_argument("--block", type=int, default=1, help="0: skip the whole block")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mha_train: no GPU -- nothing is measured")
    from mvgformer_amd import ops
    from mvgformer_amd.decoder import DQDecoderLayer
    B, Lq = a.batch, a.lq
    flop = 3.5 * 4.0 * Lq * Lq * D * M * B
    result = dict(tool="bench_mha_train", device=torch.cuda.get_device_name(0), B=B, Lq=Lq, heads=M, head_dim=D, gflop_fwd_bwd=flop / 1e9)
    gen = torch.Generator(device=DEV).manual_seed(0)
    seed = torch.tensor([1234567], dtype=torch.int64, device=DEV)
    for dt, tag in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
        if a.only not in ("both", tag):
            continue
        q, k, v, dout = (torch.randn(B, Lq, C, device=DEV, generator=gen).to(dt) for _ in range(4))
        heads = lambda t: t.view(B, Lq, M, D).transpose(1, 2).contiguous()         # noqa: E731
        qc, kc, vc = (heads(t).requires_grad_(True) for t in (q, k, v))
        gc = heads(dout)
        result[tag] = entry = {}
        inner = a.inner if dt == torch.bfloat16 else max(1, a.inner // 2)
        for p in (0.0, 0.1):
            def native(p=p):
                out, lse = ops.self_attention_train(q, k, v, p, seed)
                return ops.self_attention_backward(q, k, v, out, dout, lse, p, seed)

            def sdpa(p=p):
                out = F.scaled_dot_product_attention(qc, kc, vc, dropout_p=p)
                return torch.autograd.grad(out, (qc, kc, vc), gc)

            fns = {"native fwd+bwd p=%.1f" % p: native, "torch sdpa fwd+bwd p=%.1f" % p: sdpa}
            if not a.torch:
                fns.pop("torch sdpa fwd+bwd p=%.1f" % p)
            times, dead = _alternate(fns, a.reps, inner, a.warmup)
            print("%s  B=%d Lq=%d  p=%.1f  (%.1f GFLOP forward + backward)" % (tag, B, Lq, p, flop / 1e9))
            for name, fn in fns.items():
                _report(entry, name, times, dead, inner, flop)
                if name not in dead:
                    entry[name]["peak_MiB"] = _peak(fn)
                    print("    %-44s peak memory %.1f MiB" % ("", entry[name]["peak_MiB"]))
            names = list(fns)
            if len(names) == 2 and all("median_ms" in entry[n] for n in names):
                entry["native_over_torch p=%.1f" % p] = entry[names[0]]["median_ms"] / entry[names[1]]["median_ms"]
                print("    native / torch: %.3f" % entry["native_over_torch p=%.1f" % p])
            if p == 0.0 and a.torch and names[1] not in dead:
                mine, theirs = native(), sdpa()
                entry["max_abs_diff_vs_torch"] = [float((x.float() - y.transpose(1, 2).reshape(B, Lq, C).float()).abs().max())
                                                  for x, y in zip(mine, theirs)]
                print("    max |native - torch| dq, dk, dv: %s" % " ".join("%.3e" % e for e in entry["max_abs_diff_vs_torch"]))
        if not a.block:
            continue
        # the whole block at the head of the layer, forward + backward, train() mode (dropout 0.1 everywhere), both backends
        layer = DQDecoderLayer([8000.0, 8000.0, 2000.0], [0.0, -500.0, 800.0], [960, 512], 3, n_levels=1, n_points=8,
                               projattn_posembed_mode="ablation_not_use_rayconv", init_self_attention=True).to(DEV).train()
        layer.set_training_dtype(dt)
        tgt, pos, w = (torch.randn(B, Lq, C, device=DEV, generator=gen) for _ in range(3))
        tgt.requires_grad_(True)

        def block(backend):
            def run():
                layer.set_self_attention_training(backend)
                out = layer._attend_queries_autograd(tgt, pos)
                layer.zero_grad(set_to_none=True)
                tgt.grad = None
                (out * w).sum().backward()
            return run
        fns = {"block fwd+bwd, native": block("native"), "block fwd+bwd, torch": block("torch")}
        times, dead = _alternate(fns, a.reps, inner, a.warmup)
        for name, fn in fns.items():
            _report(entry, name, times, dead, inner)
            if name not in dead:
                entry[name]["peak_MiB"] = _peak(fn)
                print("    %-44s peak memory %.1f MiB" % ("", entry[name]["peak_MiB"]))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
