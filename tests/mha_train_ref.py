"""References of the self-attention training kernels (csrc/mha.hip, mvg_self_attention_train / _backward), batch-first (B, Lq, C),
heads as in tests/mha_ref.py.  Z is the dropout factor keep / (1 - p_q), (B, M, Lq, Lq), or None for no dropout.

  statement(q, k, v, dout, Z)       the fp64 statement: out = (Z o softmax(q k^T / sqrt(D))) v, lse, and dq, dk, dv by fp64
                                    AUTOGRAD of <out, dout> -- no formula of the kernels enters it
  flash_backward(..., dtype)        the kernels' formulas evaluated by torch on the CPU in `dtype`:
                                    P = exp(S - lse), delta = rowsum(dout o out), dS = P o (Z o dP - delta) / sqrt(D)
  flash_backward_bf16_model(...)    the same in fp64 with the bf16 kernels' rounding points: q, k, v, dout, out bf16; Z o P and
                                    dS rounded to bf16 as product operands; dq, dk, dv rounded on store; the rest unrounded
Each returns a dict of (B, Lq, C) tensors out, dq, dk, dv and lse (B, M, Lq)."""
import math

import torch

from tests import mha_ref as R

NAMES = ("out", "dq", "dk", "dv")


def _unheads(x):
    B, M, Lq, D = x.shape
    return x.permute(0, 2, 1, 3).reshape(B, Lq, M * D)


def statement(q, k, v, dout, Z=None, n_heads=R.N_HEADS):
    q, k, v = (t.double().detach().clone().requires_grad_(True) for t in (q, k, v))
    s = R.scores(q, k, n_heads)
    p = torch.softmax(s, -1)
    out = _unheads((p if Z is None else p * Z.double()) @ R._heads(v, n_heads))
    dq, dk, dv = torch.autograd.grad(out, (q, k, v), dout.double())
    return dict(out=out.detach(), lse=torch.logsumexp(s.detach(), -1), dq=dq, dk=dk, dv=dv)


def flash_backward(q, k, v, dout, Z=None, dtype=torch.float32, n_heads=R.N_HEADS, bf16_model=False, stored_out=None):
    """stored_out: the `out` the backward reads delta from, when it is not this function's own -- the backward kernel is a
    function of (q, k, v, out, dout, lse), and which way a stored bf16 `out` was rounded decides delta"""
    rnd = R.bf if bf16_model else (lambda x: x)
    qh, kh, vh, gh = (R._heads(rnd(t.to(dtype)).to(dtype), n_heads) for t in (q, k, v, dout))
    rs = 1.0 / math.sqrt(qh.shape[-1])
    s = (qh @ kh.transpose(-1, -2)) * rs
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    zp = p if Z is None else p * Z.to(dtype)
    out = rnd(rnd(zp) @ vh)
    delta = (gh * (out if stored_out is None else R._heads(stored_out.to(dtype), n_heads))).sum(-1, keepdim=True)
    dv = rnd(zp).transpose(-1, -2) @ gh
    dp = gh @ vh.transpose(-1, -2)
    ds = rnd(p * ((dp if Z is None else dp * Z.to(dtype)) - delta) * rs)
    dq, dk = ds @ kh, ds.transpose(-1, -2) @ qh
    return dict(out=_unheads(out), lse=lse, dq=rnd(_unheads(dq)), dk=rnd(_unheads(dk)), dv=rnd(_unheads(dv)))


def flash_backward_bf16_model(q, k, v, dout, Z=None, n_heads=R.N_HEADS, stored_out=None):
    return flash_backward(q, k, v, dout, Z, torch.float64, n_heads, bf16_model=True, stored_out=stored_out)


def attention_fn(Z=None, bf16_model=False):
    """a differentiable `attend` for mha_ref.block: the statement, or the bf16 model -- forward AND backward through its rounding
    points (a torch.autograd.Function around flash_backward_bf16_model), with q, k, v rounded to bf16 on the way in"""
    if not bf16_model:
        def attend(q, k, v, n_heads=R.N_HEADS):
            p = torch.softmax(R.scores(q, k, n_heads), -1)
            return _unheads((p if Z is None else p * Z.double()) @ R._heads(v.double(), n_heads))
        return attend

    class Model(torch.autograd.Function):
        @staticmethod
        def forward(ctx, q, k, v):
            ctx.save_for_backward(q, k, v)
            return flash_backward_bf16_model(q, k, v, torch.zeros_like(q), Z)["out"]

        @staticmethod
        def backward(ctx, g):
            r = flash_backward_bf16_model(*ctx.saved_tensors, g, Z)
            return r["dq"], r["dk"], r["dv"]

    return lambda q, k, v, n_heads=R.N_HEADS: Model.apply(q, k, v)
