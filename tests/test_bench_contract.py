"""bench.py's output contract (the driver parses this line): one JSON line on stdout with the metric of BASELINE.json; with
--full also the `roofline` of the dominant kernel and the `cpu_baseline` timed beside it, in a plain run only the headline.
Runs the real script on the GPU with few steps; the CPU part checks that the script refuses to run without a GPU instead of
falling back, and what --dump-outputs writes."""
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, timeout=900):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=env, timeout=timeout,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_bench_refuses_to_run_without_a_gpu():
    p = _run(["--steps", "1", "--warmup", "0"], timeout=300)
    assert p.returncode != 0
    assert "no CPU path" in (p.stderr + p.stdout)


@pytest.mark.gpu
def test_bench_line_has_the_contract_fields():
    p = _run(["--steps", "5", "--warmup", "2", "--full", "--cpu-baseline", "0"])
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, "exactly one line on stdout"
    d = json.loads(lines[0])
    with open(os.path.join(ROOT, "BASELINE.json")) as f:
        base = json.load(f)
    assert d["metric"] in base["metric"]                       # the metric BASELINE.json names
    for k in ("value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 5 and d["warmup"] == 2 and d["higher_is_better"] is True
    assert d["unit"] == "samples/s" and d["dtype"] == "bf16" and d["data"] == "synthetic" and d["vs_baseline"] is None
    assert abs(d["value"] - 1e3 / d["ms_per_step_mean"]) < 1e-2 * d["value"]     # value: wall clock of the timed region
    lo, hi = d["ms_per_step_min_max"]
    assert lo <= d["ms_per_step"] <= hi and d["ms_per_step"] <= 1.05 * d["ms_per_step_mean"]    # the median of the per-step intervals
    assert "workload" in d["config"] and "model" not in d["config"] and d["config"]["hip_graph"] is True
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and r["kernel"] == "msda_gsamp_pipe_kernel"    # (the double-buffered build: 76 800 pairs per launch)
    # the same kernel inside the replayed forward (kernel-trace child pass): 4 launches per forward x 8 replays, priced by the same bytes
    f = r["in_forward"]
    assert "unavailable" not in f, f
    assert f["launches"] == 32 and 0.5 * r["avg_launch_us"] < f["avg_launch_us"] < 1.5 * r["avg_launch_us"]
    assert abs(f["frac"] - r["algorithmic_bytes_per_launch"] / (f["avg_launch_us"] * 1e-6) / 8e12) < 1e-3
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    # flat scalars of the same facts (a parser that drops nested objects keeps them) + what the launch keeps busy (PMC child pass)
    assert r["in_forward_us"] == f["avg_launch_us"] and r["in_forward_frac"] == f["frac"]
    assert "issue_shares_unavailable" not in r, r.get("issue_shares_unavailable")
    assert 0.05 < r["valu_busy"] < 1.0 and 0.05 < r["l1_addr_busy"] < 1.2 and 50 < r["vmem_rd_per_wave"] < 130
    assert r["valu_insts_per_wave"] < 1200                                       # VERDICT r5 item 1's instruction bar (1 404 in round 5)
    # 5 views x 46.20 MB (bf16) per launch
    assert r["algorithmic_bytes_per_launch"] == 231014400
    assert abs(r["achieved"] - r["algorithmic_bytes_per_launch"] / r["avg_launch_us"] / 1e3) < 1.0
    assert 0.02 < r["frac"] < 1.0
    # the MFMA regime of SURVEY 8(d)(ii), next to the HBM one
    m = d["roofline_mfma"]
    assert m["bound"] == "mfma" and m["peak"] == 2500.0 and m["unit"] == "TFLOP/s"
    assert m["flops_nominal"] == 390038814720                     # 97.5 GFLOP per layer x 4
    assert 0.5 * m["flops_nominal"] < m["flops_executed"] <= m["flops_per_step"] <= 1.2 * m["flops_nominal"]
    assert abs(m["frac"] - m["achieved_tflops"] / m["peak"]) < 1e-3 and 0.0 < m["frac"] <= 1.0
    assert abs(m["achieved_tflops"] - m["flops_executed"] / d["ms_per_step"] / 1e9) < 0.5
    assert {"chain_a", "chain_b", "value_proj", "feat_linear", "pyramid_group_one_layer_just_in_time"} <= set(m["per_kernel"])
    for name, k in m["per_kernel"].items():
        assert 0.0 < k["frac"] <= 1.0 and abs(k["tflops"] - k["gflop"] / k["us"] * 1e3) < 0.02 * k["tflops"] + 0.5, (name, k)
    assert d["scaling"] is None and d["rccl"] is None           # one GPU: neither weak nor strong, no collectives
    # the other named workloads ride in the same line (driver-witnessed): fp32 at cfg-2 / cfg-4, nothing-skipped bf16, cfg-5, B > 1
    sec = d["secondary"]
    assert set(sec) == {"cfg2_fp32", "cfg4_fp32", "cfg2_bf16_inside_all", "cfg5_bf16", "cfg2_bf16_batch2", "cfg2_bf16_batch4",
                        "cfg2_bf16_valid10", "cfg2_bf16_producer_inplace", "train_step_cfg2_fp32"}
    assert r["frac_inside_all"] == sec["cfg2_bf16_inside_all"]["frac"]
    train = sec.pop("train_step_cfg2_fp32")
    assert "error" not in train, train
    done, total = train["parameters_with_finite_gradients"].split(" / ")
    assert train["steps"] >= 5 and train["fp32_form"] == "2xfp16x3" and 0 < int(done) <= int(total) and train["ms_per_step"] > 0
    assert 0.02 < sec["cfg2_bf16_valid10"]["valid_query_share_last_layer"] < 0.5
    for name, rec in sec.items():
        assert "error" not in rec, (name, rec)
        assert ("fp32_form" in rec) == name.endswith("fp32") and rec.get("fp32_form", "2xfp16x3") == "2xfp16x3"
        for k in ("ms_per_step", "ms_per_sample", "value", "dtype", "workload", "sampler_kernel", "sampler_us", "frac", "steps"):
            assert k in rec, (name, k)
        assert rec["steps"] >= 20 and rec["hip_graph"] is True and 0.02 < rec["frac"] < 1.0
        assert abs(rec["ms_per_sample"] * int(rec["workload"].split("batch ")[1].split(",")[0]) - rec["ms_per_step_median"]) < 1e-3
        assert rec["dtype"] == ("fp32" if name.endswith("fp32") else "bf16")
    # no per-step pack: not slower than the headline beyond what two segments of one process differ by (+-3 %: the pack is off the
    # critical path, profiles/r06_experiments.txt)
    assert sec["cfg2_bf16_producer_inplace"]["ms_per_step_median"] < 1.06 * d["ms_per_step"]
    assert sec["cfg5_bf16"]["ms_per_step"] > sec["cfg2_fp32"]["ms_per_step"] > d["ms_per_step"]
    for name, rec in sec.items():
        lo, hi = rec["ms_per_step_min_max"]
        assert lo <= rec["ms_per_step"] <= hi and rec["ms_per_step"] == rec["ms_per_step_median"], name


@pytest.mark.gpu
def test_plain_bench_run_times_the_headline_only_and_dumps_its_outputs(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W`: the headline fields, K timed steps, nothing of what --full adds; --dump-outputs writes
    the last timed step's outputs (float32, at most 64 MB) and the line names what it wrote."""
    dump = tmp_path / "out"
    p = _run(["--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", str(dump)])
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, "exactly one line on stdout"
    d = json.loads(lines[0])
    with open(os.path.join(ROOT, "BASELINE.json")) as f:
        assert d["metric"] in json.load(f)["metric"]
    assert d["steps"] == 7 and d["warmup"] == 2 and d["unit"] == "samples/s" and d["dtype"] == "bf16" and d["higher_is_better"] is True
    lo, hi = d["ms_per_step_min_max"]
    assert 0 < lo <= d["ms_per_step"] <= hi and abs(d["value"] - 1e3 / d["ms_per_step_mean"]) < 1e-2 * d["value"]
    assert d["full"] is False and d["config"]["hip_graph"] is True
    assert d["roofline"] is None and d["roofline_mfma"] is None and d["cpu_baseline"] is None and d["secondary"] is None
    assert d["kernels"] == {} and d["rank_time_split"] is None
    import numpy as np
    shapes = d["dumped_outputs"]["shapes"]
    assert set(shapes) == {"hs", "refs", "refs2d", "projs2d", "class_prob"}
    total = 0
    for name, shape in shapes.items():
        a = np.load(str(dump / (name + ".npy")))
        assert a.dtype == np.float32 and list(a.shape) == shape and np.isfinite(a).all(), name
        total += a.nbytes
    assert total <= 64 << 20
    assert shapes["refs"][:2] == [4, 1] and shapes["refs"][3] == 3 and shapes["class_prob"][-1] == 2


def test_dump_outputs_is_float32_bounded_and_the_same_sample_every_time(tmp_path):
    """bench.dump_outputs on the headline's output shapes (cfg-2: 4 layers, 15 360 query-joints, 5 views): over 64 MB in all, so
    every array keeps the same seeded sample of its query axis; two dumps of the same outputs are identical."""
    import numpy as np
    import bench
    g = torch.Generator().manual_seed(0)
    L, Lq, V, NQ = 4, 15360, 5, 1024
    out = (torch.randn(L, 1, Lq, 256, generator=g), torch.randn(L, 1, Lq, 3, generator=g), torch.randn(L, 1, V, Lq, 2, generator=g),
           torch.randn(L, 1, V, Lq, 2, generator=g), [torch.rand(1, NQ, 2, generator=g).to(torch.bfloat16) for _ in range(L)])
    a = bench.dump_outputs(out, str(tmp_path / "a"))
    b = bench.dump_outputs(out, str(tmp_path / "b"))
    assert a == b and set(a) == {"hs", "refs", "refs2d", "projs2d", "class_prob"}
    assert a["hs"][2] == a["refs"][2] == a["refs2d"][3] < Lq
    total = 0
    for name in a:
        x, y = np.load(str(tmp_path / "a" / (name + ".npy"))), np.load(str(tmp_path / "b" / (name + ".npy")))
        assert x.dtype == np.float32 and (x == y).all()
        total += x.nbytes
    assert total <= 64 << 20
    # the sample holds rows of the originals: hs row k of the dump is one of the 15 360 rows of the last layer
    hs = np.load(str(tmp_path / "a" / "hs.npy"))
    assert (out[0][-1, 0].numpy() == hs[-1, 0, 0]).all(axis=1).any()


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_plain_multi_gpu_command_launches_its_own_ranks():
    """`python bench.py --gpus 2` (no torch.distributed.run in front, the shape of the driver's 1-GPU command) starts two
    ranks itself and both reach init_process_group (gloo override: no GPU / RCCL in this container); then every rank
    stops because there is no GPU -- not because the launch was refused."""
    env = dict(os.environ, PYTHONPATH=ROOT, MVG_DIST_BACKEND="gloo")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       cwd=ROOT, env=env, timeout=600, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    out = p.stderr + p.stdout
    assert p.returncode != 0
    assert "rank 0/2: process group up (gloo)" in out and "rank 1/2: process group up (gloo)" in out, out[-3000:]
    assert "no CPU path" in out
    assert "launch with torch.distributed.run" not in out


@pytest.mark.gpu
@pytest.mark.parametrize("speculative", [1, 0])
def test_two_rank_query_sharded_bench_runs_end_to_end_on_one_gpu(speculative):
    """`python bench.py --gpus 2` end to end on the one-GPU box: the script starts its own two ranks (torch.distributed.run,
    127.0.0.1), both on cuda:0 with gloo carrying the collectives (RCCL needs one device per rank), query shards of 512,
    the forward as one HIP graph with the speculative any-valid flag (or graph segments + per-layer all-reduce), the one
    all-gather of the pose set per step, barrier + max-over-ranks timing, ONE JSON line from rank 0."""
    env = dict(os.environ, PYTHONPATH=ROOT, MVG_DIST_BACKEND="gloo")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "2",
                        "--speculative", str(speculative), "--full", "--traffic", "off", "--profile-steps", "1"],
                       cwd=ROOT, env=env, timeout=900, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["steps"] == 4
    assert "queries sharded x2" in d["config"]["parallelism"] and d["config"]["hip_graph"] is True
    assert ("speculative" in d["config"]["parallelism"]) == bool(speculative)
    assert abs(d["value"] - 1e3 / d["ms_per_step_mean"]) < 1e-2 * d["value"]       # one sample per step, whole job
    assert "process group up (gloo)" in p.stderr
    # first-contact insurance: the collectives ran once before anything was timed, and the line says what they saw
    assert d["rccl"]["ok"] is True and d["rccl"]["ranks"] == 2 and d["rccl"]["ranks_seen"] == [0, 1] and d["rccl"]["backend"] == "gloo"
    # the weak-scaling number of the same job: one sample per rank and step
    rep = d["secondary"]["shard_samples"]
    assert rep["scaling"] == "weak" and rep["n_gpus"] == 2 and abs(rep["value"] - 2e3 / rep["ms_per_step"]) < 1e-2 * rep["value"]


@pytest.mark.gpu
def test_eight_rank_query_sharded_bench_on_one_gpu():
    """the shape of the driver's 8-GPU command (8 ranks, 128 queries each, one graph per rank + the all-gather) on the one-GPU box:
    all ranks on cuda:0, gloo carrying the collectives -- everything of the N = 8 run except RCCL itself and the xGMI links."""
    env = dict(os.environ, PYTHONPATH=ROOT, MVG_DIST_BACKEND="gloo", OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "3", "--warmup", "1",
                        "--full", "--traffic", "off", "--profile-steps", "1", "--secondary", "0"],
                       cwd=ROOT, env=env, timeout=1500, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 8 and d["scaling"] == "strong" and "queries sharded x8" in d["config"]["parallelism"]
    assert d["rccl"]["ok"] is True and d["rccl"]["ranks_seen"] == list(range(8))
    assert d["roofline"]["algorithmic_bytes_per_launch"] < 231014400       # a rank's shard: 128 of the 1024 queries
