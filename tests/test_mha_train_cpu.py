"""CPU side of the self-attention training path: tests/mha_train_ref.py pinned to torch's own operator and to fp64 autograd, the
backend switch, and the refusals of CPU tensors.  No kernel is launched."""
import pytest
import torch
import torch.nn.functional as F

from tests import mha_train_ref as T
from tests import test_mha_fp64 as base

C, M = base.C, base.M


def _inputs(Lq, B=2):
    q, k, v = base._case(Lq, B, "float32")[:3]
    dout = torch.randn(B, Lq, C, generator=torch.Generator().manual_seed(77 + Lq))
    return q, k, v, dout


def _Z(B, Lq, p, seed=3):
    keep = torch.rand(B, M, Lq, Lq, generator=torch.Generator().manual_seed(seed)) >= p
    return keep.double() / (1.0 - p)


@pytest.mark.parametrize("Lq", [1, 15, 65])
def test_statement_without_dropout_is_torchs_multi_head_attention_in_fp64(Lq):
    q, k, v, dout = (t.double() for t in _inputs(Lq))
    want = T.statement(q, k, v, dout)
    eye3, eye, z3, z = torch.eye(C).repeat(3, 1).double(), torch.eye(C).double(), torch.zeros(3 * C).double(), torch.zeros(C).double()
    qt, kt, vt = (t.transpose(0, 1).contiguous().requires_grad_(True) for t in (q, k, v))
    y = F.multi_head_attention_forward(qt, kt, vt, C, M, eye3, z3, None, None, False, 0.0, eye, z, training=False,
                                       need_weights=False)[0].transpose(0, 1)
    g = torch.autograd.grad(y, (qt, kt, vt), dout)
    assert float((y.detach() - want["out"]).abs().max()) <= 1e-12
    for name, got in zip(("dq", "dk", "dv"), g):
        assert float((got.transpose(0, 1) - want[name]).abs().max()) <= 1e-12, name


@pytest.mark.parametrize("Lq", [1, 15, 33, 65, 129])
def test_flash_formulas_equal_fp64_autograd_under_a_random_mask(Lq):
    q, k, v, dout = _inputs(Lq)
    Z = _Z(2, Lq, 0.1)
    want = T.statement(q, k, v, dout, Z)
    got = T.flash_backward(q, k, v, dout, Z, torch.float64)
    for name in T.NAMES + ("lse",):
        err = float((got[name] - want[name]).abs().max())
        print("Lq=%d %s: max|err| %.3e (largest entry %.3g)" % (Lq, name, err, float(want[name].abs().max())))
        assert err <= 4e-13, name


def test_bf16_model_is_close_and_not_equal():
    q, k, v, dout = (t.bfloat16() for t in _inputs(33))
    Z = _Z(2, 33, 0.1)
    want, got = T.statement(q, k, v, dout, Z), T.flash_backward_bf16_model(q, k, v, dout, Z)
    for name in T.NAMES:
        err, top = float((got[name] - want[name]).abs().max()), float(want[name].abs().max())
        assert 0.0 < err <= 0.2 * top, (name, err, top)


def _layer():
    from tests.test_selfattn_cpu import _layer as make
    return make(init_self_attention=True)


def test_switch_validates_and_defaults_to_torch():
    from mvgformer_amd import decoder as D
    layer = _layer()
    assert D.SELF_ATTN_TRAIN == "torch" and layer.self_attention_training == "torch"
    assert layer.set_self_attention_training("native") is layer and layer.self_attention_training == "native"
    for bad in ("hip", None, "Native", 1):
        with pytest.raises(ValueError):
            layer.set_self_attention_training(bad)
    assert layer.self_attention_training == "native"
    dec = torch.nn.Module.__new__(D.DQDecoder)
    torch.nn.Module.__init__(dec)
    dec.layers = torch.nn.ModuleList([layer, _layer()])
    with pytest.raises(ValueError):
        dec.set_self_attention_training("flash")
    assert dec.set_self_attention_training("native") is dec
    assert [l.self_attention_training for l in dec.layers] == ["native", "native"]
    dec.set_self_attention_training("torch")
    assert [l.self_attention_training for l in dec.layers] == ["torch", "torch"]


def test_cpu_tensors_are_refused():
    from mvgformer_amd import functions, ops
    q = torch.zeros(1, 8, C)
    lse = torch.zeros(1, M, 8)
    seed = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.self_attention_train(q, q, q)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.self_attention_backward(q, q, q, q, q, lse)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.self_attention_dropout_mask(1, 8, 0.1, seed)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        functions.self_attention(q, q, q, dropout_p=0.1, training=True)
    layer = _layer().set_self_attention_training("native")
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        layer._attend_queries_autograd(q, q)


def test_quantised_probability():
    from mvgformer_amd import ops
    assert ops.dropout_p_quantised(0.0) == 0.0 and ops.dropout_p_quantised(0.1) == 26 / 256
    assert ops.dropout_p_quantised(0.5) == 0.5 and ops.dropout_p_quantised(0.9999) == 255 / 256
