"""CPU-only checks of the optimizer step's host side: the two parameter groups of factory.build_optimizer_from_cfg for every shipped
YAML (run/train_3d.py:116-146), the TRAIN block of load_yaml_config, and what optim.FusedAdam refuses.  No kernel is launched."""
import json
import os
from types import SimpleNamespace

import pytest
import torch

from mvgformer_amd.factory import build_decoder_from_cfg, build_optimizer_from_cfg, load_yaml_config
from mvgformer_amd.optim import CHUNK, FusedAdam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "mvgformer_amd", "data", "yaml_extract.json")) as _f:
    EXTRACT = json.load(_f)


def _cfg(val, train=None):
    cfg = SimpleNamespace(DECODER=SimpleNamespace(**val["DECODER"]), NETWORK=SimpleNamespace(IMAGE_SIZE=val["IMAGE_SIZE"]),
                          MULTI_PERSON=SimpleNamespace(SPACE_SIZE=val["SPACE_SIZE"], SPACE_CENTER=val["SPACE_CENTER"]),
                          DATASET=SimpleNamespace(CAMERA_NUM=val["CAMERA_NUM"]))
    if train is not None:
        cfg.TRAIN = SimpleNamespace(**train)
    return cfg


@pytest.mark.parametrize("rel", sorted(EXTRACT))
def test_parameter_groups_of_every_shipped_yaml(rel):
    from mvgformer_amd.caller import DecoderHead
    assert len(EXTRACT) == 12
    val = EXTRACT[rel]
    cfg = _cfg(val, dict(LR=0.0004, clip_max_norm=0.1))
    d = cfg.DECODER
    head = DecoderHead(build_decoder_from_cfg(cfg), 8, d.num_keypoints, d.d_model, val["SPACE_SIZE"], val["SPACE_CENTER"])
    opt = build_optimizer_from_cfg(head, cfg)
    named = dict(head.named_parameters())
    slow = {n for n in named if "sampling_offsets" in n or "reference_points" in n}
    assert len(slow) == 2 * d.num_decoder_layers                      # sampling_offsets.weight / .bias of every layer
    g0, g1 = opt.param_groups
    assert {id(p) for p in g1["params"]} == {id(named[n]) for n in slow}
    assert {id(p) for p in g0["params"]} == {id(named[n]) for n in named if n not in slow}
    assert len(g0["params"]) + len(g1["params"]) == len(named)
    assert g0["lr"] == 0.0004 and g1["lr"] == 0.0004 * d.lr_linear_proj_mult == 0.0004 * 0.1
    want_wd, want_dec = (1e-4, True) if d.optimizer == "adamw" else (0.0, False)
    assert d.optimizer in ("adam", "adamw")
    for g in opt.param_groups:
        assert g["weight_decay"] == want_wd and g["decoupled_weight_decay"] is want_dec
    assert opt.clip_max_norm == 0.1 and opt.zero_grad_after_step is True
    # the arguments override the cfg; without a TRAIN block the defaults of lib/core/config.py hold
    other = build_optimizer_from_cfg(head, _cfg(val), optim_type="adamw", weight_decay=0.01, lr=0.5)
    assert [g["lr"] for g in other.param_groups] == [0.5, 0.5 * 0.1] and other.param_groups[0]["weight_decay"] == 0.01
    assert other.param_groups[1]["decoupled_weight_decay"] is True and other.clip_max_norm == 0.1
    assert build_optimizer_from_cfg(head, _cfg(val)).param_groups[0]["lr"] == 0.001
    with pytest.raises(ValueError, match="adam"):
        build_optimizer_from_cfg(head, cfg, optim_type="sgd")


_YAML = """
DATASET: {CAMERA_NUM: 5}
NETWORK: {IMAGE_SIZE: [960, 512]}
MULTI_PERSON: {SPACE_SIZE: [8000.0, 8000.0, 2000.0], SPACE_CENTER: [0.0, -500.0, 800.0]}
DECODER: {d_model: 256, nhead: 8, num_decoder_layers: 4, num_instance: 1024, optimizer: adam, lr_linear_proj_mult: 0.1}
%s
"""


def test_load_yaml_config_reads_the_train_block(tmp_path):
    y = tmp_path / "cfg.yaml"
    y.write_text(_YAML % "TRAIN: {BATCH_SIZE: 1, SHUFFLE: true, BEGIN_EPOCH: 0, END_EPOCH: 100, RESUME: false, OPTIMIZER: adam, LR: 0.0004}")
    cfg = load_yaml_config(str(y))
    assert cfg.TRAIN.LR == 0.0004 and cfg.TRAIN.clip_max_norm == 0.1          # clip_max_norm: no shipped YAML sets it
    assert cfg.DECODER.optimizer == "adam" and cfg.DATASET.CAMERA_NUM == 5
    y.write_text(_YAML % "TRAIN: {LR: 0.002, clip_max_norm: 0.5}")
    cfg = load_yaml_config(str(y))
    assert cfg.TRAIN.LR == 0.002 and cfg.TRAIN.clip_max_norm == 0.5
    y.write_text(_YAML % "")
    cfg = load_yaml_config(str(y))
    assert cfg.TRAIN.LR == 0.001 and cfg.TRAIN.clip_max_norm == 0.1           # lib/core/config.py:152,169


def test_cpu_parameters_raise_on_step():
    p = torch.nn.Parameter(torch.zeros(5))
    p.grad = torch.ones(5)
    opt = FusedAdam([p], lr=1e-3)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        opt.step()
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        opt.prepare()
    assert torch.equal(p.detach(), torch.zeros(5))


def test_unsupported_options_and_parameters_raise():
    p = torch.nn.Parameter(torch.zeros(4, 6))
    with pytest.raises(NotImplementedError, match="amsgrad"):
        FusedAdam([p], lr=1e-3, amsgrad=True)
    with pytest.raises(NotImplementedError, match="maximize"):
        FusedAdam([p], lr=1e-3, maximize=True)
    with pytest.raises(TypeError, match="float32"):
        FusedAdam([torch.nn.Parameter(torch.zeros(4, dtype=torch.bfloat16))], lr=1e-3)
    with pytest.raises(ValueError, match="contiguous"):
        FusedAdam([torch.zeros(4, 6).t().requires_grad_(True)], lr=1e-3)
    opt = FusedAdam([p], lr=1e-3)
    with pytest.raises(TypeError, match="float32"):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(2, dtype=torch.float64))]})
    with pytest.raises(NotImplementedError, match="closure"):
        opt.step(closure=lambda: 0.0)
    with pytest.raises(ValueError, match="learning rate"):
        FusedAdam([p], lr=-1.0)
    sd = torch.optim.Adam([p], lr=1e-3, amsgrad=True).state_dict()
    with pytest.raises(NotImplementedError, match="amsgrad"):
        FusedAdam([p], lr=1e-3).load_state_dict(sd)


def test_state_dict_layout_is_torch_adams():
    """keys of the state dict, of a parameter's state and of a group, and a load in both directions on host tensors (load_state_dict
    launches nothing)"""
    def make():
        a, b = torch.nn.Parameter(torch.arange(6.).reshape(2, 3)), torch.nn.Parameter(torch.ones(4))
        return [{"params": [a]}, {"params": [b], "lr": 0.5}]
    tp = make()
    ref = torch.optim.Adam(tp, lr=1e-2, foreach=False)
    for g in tp:
        g["params"][0].grad = torch.ones_like(g["params"][0])
    ref.step()
    ref.step()
    want = ref.state_dict()
    mine = FusedAdam(make(), lr=1e-2)
    mine.load_state_dict(want)
    got = mine.state_dict()
    assert list(got) == list(want) and list(got["state"]) == list(want["state"])
    for k in want["state"]:
        assert list(got["state"][k]) == list(want["state"][k]) == ["step", "exp_avg", "exp_avg_sq"]
        assert float(got["state"][k]["step"]) == 2.0 and got["state"][k]["step"].dtype == want["state"][k]["step"].dtype
        for n in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(got["state"][k][n], want["state"][k][n])
            assert got["state"][k][n].data_ptr() != want["state"][k][n].data_ptr()      # own memory, not the saved tensors
    assert mine.step_count() == 2
    for g, w in zip(got["param_groups"], want["param_groups"]):
        assert set(g) == set(w) and g["params"] == w["params"] and g["lr"] == w["lr"]
    back = torch.optim.Adam(make(), lr=1e-2, foreach=False)
    back.load_state_dict(got)
    assert float(back.state[back.param_groups[1]["params"][0]]["step"]) == 2.0
    # per-parameter steps that differ cannot be kept in one count
    bad = ref.state_dict()
    bad["state"][1] = dict(bad["state"][1], step=torch.tensor(5.0))
    with pytest.raises(ValueError, match="one step count"):
        FusedAdam(make(), lr=1e-2).load_state_dict(bad)
    assert CHUNK == 4096
