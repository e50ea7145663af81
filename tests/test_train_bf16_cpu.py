"""CPU checks of the bf16 training switch: set_training_dtype's contract, the state dict, and the two new C symbols."""
import copy
import os
import re

import pytest
import torch

from mvgformer_amd import _lib
from mvgformer_amd.factory import build_decoder_for_case
from mvgformer_amd.synthetic import build_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _decoder():
    return build_decoder_for_case(build_case("cfg1", seed=0, layers=2), "cpu", torch.float32)


def test_set_training_dtype_accepts_fp32_and_bf16_only_and_reaches_every_layer():
    dec = _decoder()
    assert all(l.training_dtype == torch.float32 and l.proj_attn.training_dtype == torch.float32 for l in dec.layers)
    assert dec.set_training_dtype(torch.bfloat16) is dec
    assert all(l.training_dtype == torch.bfloat16 and l.proj_attn.training_dtype == torch.bfloat16 for l in dec.layers)
    assert all(l.compute_dtype == torch.float32 for l in dec.layers)          # the inference setting is a separate one
    layer = dec.layers[0]
    assert layer.set_training_dtype(torch.float32) is layer
    assert layer.training_dtype == torch.float32 and dec.layers[1].training_dtype == torch.bfloat16
    for bad in (torch.float16, torch.float64, "bf16", None):
        with pytest.raises(ValueError):
            dec.set_training_dtype(bad)
        with pytest.raises(ValueError):
            layer.set_training_dtype(bad)


def test_training_dtype_adds_no_state():
    dec = _decoder()
    before = {k: v.clone() for k, v in dec.state_dict().items()}
    dec.set_training_dtype(torch.bfloat16)
    after = dec.state_dict()
    assert list(before) == list(after) and all(torch.equal(before[k], after[k]) for k in before)
    assert sum(1 for k in after if k.startswith("layers.0.")) == 32
    cp = copy.deepcopy(dec)
    assert all(l.training_dtype == torch.bfloat16 for l in cp.layers)


def test_new_symbols_are_in_the_header_and_the_signatures():
    header = open(os.path.join(ROOT, "include", "mvg_decoder.h")).read()
    for name in ("mvg_msda_backward_det_bf16", "mvg_linear_wgrad_bias_bf16"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES["mvg_msda_backward_det_bf16"] == _lib.SIGNATURES["mvg_msda_backward_det_f32"]
    assert _lib.SIGNATURES["mvg_linear_wgrad_bias_bf16"] == _lib.SIGNATURES["mvg_linear_wgrad_bias_f32"]
