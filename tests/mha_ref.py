"""fp64 statement of the decoder layer's query self-attention block (init_self_attention, dq_decoder.py:281-283,532-539):
    q = k = tgt + query_pos;  tgt' = norm2(tgt + out_proj(attention(Wq q, Wk k, Wv tgt)))
batch-first, (B, Lq, C) throughout -- the reference transposes to (Lq, B, C) around nn.MultiheadAttention and back.  Pinned to
torch.nn.functional.multi_head_attention_forward in fp64 by tests/test_mha_ref_cpu.py.

`attention_bf16_model` is the same attention with the bf16 kernel's rounding points (csrc/mha.hip) applied in fp64: Q, K, V
rounded to bf16; P = exp(score - TRUE row maximum) rounded to bf16 as the operand of P V while the row sum adds the unrounded P;
O rounded to bf16 after the division.  (The kernel rounds P relative to its running maximum: another scale, the same relative
rounding -- which is why the test grants the kernel twice this model's error.)"""
import math

import torch

N_HEADS, D_HEAD = 8, 32


def bf(x):
    """round to bf16, back in fp64"""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def _heads(x, n_heads):
    B, Lq, C = x.shape
    return x.view(B, Lq, n_heads, C // n_heads).permute(0, 2, 1, 3)          # (B, M, Lq, D)


def scores(q, k, n_heads=N_HEADS):
    """(B, M, Lq, Lq) fp64: q . k / sqrt(D)"""
    qh, kh = _heads(q.double(), n_heads), _heads(k.double(), n_heads)
    return qh @ kh.transpose(-1, -2) / math.sqrt(qh.shape[-1])


def attention(q, k, v, n_heads=N_HEADS):
    """O (B, Lq, C) fp64 = softmax_j(q_i . k_j / sqrt(D)) v_j per head; heads in columns D h .. D h + D - 1"""
    B, Lq, C = q.shape
    s = scores(q, k, n_heads)
    p = torch.exp(s - s.amax(-1, keepdim=True))
    o = (p @ _heads(v.double(), n_heads)) / p.sum(-1, keepdim=True)
    return o.permute(0, 2, 1, 3).reshape(B, Lq, C)


def attention_bf16_model(q, k, v, n_heads=N_HEADS):
    """the bf16 variant's rounding points in fp64 (see the module docstring)"""
    B, Lq, C = q.shape
    s = scores(bf(q), bf(k), n_heads)
    p = torch.exp(s - s.amax(-1, keepdim=True))
    o = (bf(p) @ _heads(bf(v), n_heads)) / p.sum(-1, keepdim=True)
    return bf(o.permute(0, 2, 1, 3).reshape(B, Lq, C))


def layer_norm(x, g, b, eps=1e-5):
    x = x.double()
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g.double() + b.double()


def block(tgt, query_pos, in_proj_weight, in_proj_bias, out_proj_weight, out_proj_bias, norm_weight, norm_bias, n_heads=N_HEADS,
          attend=attention):
    """tgt' (B, Lq, C) fp64 of the block at the head of the layer; `attend`: attention or attention_bf16_model"""
    tgt = tgt.double()
    x = tgt if query_pos is None else tgt + query_pos.double()
    C = tgt.shape[-1]
    W, bias = in_proj_weight.double(), in_proj_bias.double()
    q = x @ W[:C].T + bias[:C]
    k = x @ W[C:2 * C].T + bias[C:2 * C]
    v = tgt @ W[2 * C:].T + bias[2 * C:]
    a = attend(q, k, v, n_heads) @ out_proj_weight.double().T + out_proj_bias.double()
    return layer_norm(tgt + a, norm_weight, norm_bias)
