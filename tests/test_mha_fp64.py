"""mvg_self_attention (csrc/mha.hip) against the fp64 statement of tests/mha_ref.py, both arithmetic variants, at the sequence
lengths where its code switches paths (one tile / a ragged tile / several tiles / several workgroups) and on rows built to
break an online softmax.  The bounds are measured on the spot from the same inputs, not fixed numbers:
  fp32: max |err| <= 4 x the max |err| of torch's own fp32 multi_head_attention_forward on the CPU (identity projections, so
        that its error is the attention's alone; need_weights=True, as the reference calls it) -- the margin covers the other
        summation order;
  bf16: max |err| <= 2 x the max |err| of mha_ref.attention_bf16_model (the kernel's rounding points in fp64) -- the margin is
        there because the running maximum rounds P at another scale than the model's true maximum does.
Every element of every output is compared.  Every output lies between two guard regions that must come back untouched.
Each assertion prints both figures and their ratio."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import mha_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 1024
SENT = -7.25e5
BADARG = 10001
LQS = (1, 15, 31, 32, 33, 63, 64, 65, 127, 129, 975)
C, M, D = 256, 8, 32


def _lib():
    from mvgformer_amd import _lib as L
    return L


def _adversarial(q, k):
    """rewrites rows of q / keys of k (one batch element, (Lq, C) fp32, in place), head by head.  Returns {name: query row}."""
    Lq = q.shape[0]
    rows = {}
    if Lq < 6:
        return rows
    # one key whose score exceeds the rest of its row by 60: first, last, on both sides of a tile boundary (32-key blocks
    # inside a 64-key tile, and the 64-key tile itself)
    edge = 64 if Lq > 65 else 32 if Lq > 33 else Lq // 2
    want = {"big_first": (0, 0), "big_last": (1, Lq - 1), "big_tile_start": (2, edge), "big_tile_end": (3, edge - 1)}
    for h in range(M):                                   # rows 0..3 mutually orthogonal: one row's big key is a zero score for the others
        sl = slice(D * h, D * h + D)
        for i in range(1, 4):
            for j in range(i):
                q[i, sl] -= q[j, sl] * (float(q[i, sl] @ q[j, sl]) / float(q[j, sl] @ q[j, sl]))
    used = set()
    for name, (row, key) in want.items():
        if key in used or key < 0:
            continue
        used.add(key)
        rows[name] = row
        for h in range(M):
            sl = slice(D * h, D * h + D)
            s = (k[:, sl] @ q[row, sl]) / D ** 0.5
            s[key] = float("-inf")
            k[key, sl] = q[row, sl] * ((float(s.max()) + 60.0) * D ** 0.5 / float(q[row, sl] @ q[row, sl]))
    q[4] = 0.0                                           # all scores of the row equal
    rows["all_equal"] = 4
    for h in range(M):                                   # scores of the row spread over [-80, 80]
        sl = slice(D * h, D * h + D)
        s = (k[:, sl] @ q[5, sl]) / D ** 0.5
        q[5, sl] *= 80.0 / float(s.abs().max())
    rows["pm80"] = 5
    return rows


@functools.lru_cache(maxsize=None)
def _case(Lq, B, dt_name, variant=0):
    """inputs (CPU, in the kernel's dtype), the exact fp64 result from THOSE inputs, and the yardstick's max |err|.
    variant != 0: batch element 1 gets other content, element 0 stays."""
    dt = getattr(torch, dt_name)
    qs, ks, vs, rows = [], [], [], {}
    for b in range(B):
        gen = torch.Generator().manual_seed(1000 * Lq + 10 * b + (variant if b == 1 else 0))
        q, k, v = (torch.randn(Lq, C, generator=gen) for _ in range(3))
        q *= 1.5
        rows = _adversarial(q, k)
        qs.append(q), ks.append(k), vs.append(v)
    q, k, v = (torch.stack(t).to(dt) for t in (qs, ks, vs))
    exact = R.attention(q, k, v)
    if dt == torch.float32:
        eye3, eye, z3, z = torch.eye(C).repeat(3, 1), torch.eye(C), torch.zeros(3 * C), torch.zeros(C)
        qt, kt, vt = (t.transpose(0, 1).contiguous() for t in (q, k, v))         # (Lq, B, C), the reference's layout
        y = F.multi_head_attention_forward(qt, kt, vt, C, M, eye3, z3, None, None, False, 0.0, eye, z, training=False,
                                           need_weights=True)[0].transpose(0, 1)
        yard = float((y.double() - exact).abs().max())
    else:
        yard = float((R.attention_bf16_model(q, k, v) - exact).abs().max())
    return q, k, v, exact, yard, rows


def _launch(q, k, v, C_=C, M_=M):
    """raw C-ABI launch into a guarded buffer; returns (code, output clone)"""
    L = _lib()
    B, Lq = q.shape[0], q.shape[1]
    n = B * Lq * C
    buf = torch.full((GUARD + n + GUARD,), SENT, dtype=q.dtype, device=DEV)
    out = buf[GUARD:GUARD + n]
    rc = L.load().mvg_self_attention(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(out), q.stride(1), k.stride(1), v.stride(1), B, Lq, C_, M_,
                                     L.dtype_code(q.dtype), L.stream_ptr())
    torch.cuda.synchronize()
    sent = torch.tensor(SENT, dtype=q.dtype).item()
    assert bool((buf[:GUARD] == sent).all()) and bool((buf[GUARD + n:] == sent).all()), "guard region overwritten"
    if rc != 0:
        assert bool((out == sent).all()), "a refused call wrote its output"
    return rc, out.view(B, Lq, C).clone()


@pytest.mark.parametrize("dt_name", ["float32", "bfloat16"])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("Lq", LQS)
def test_self_attention_vs_fp64(Lq, B, dt_name):
    q, k, v, exact, yard, rows = _case(Lq, B, dt_name)
    margin = 4.0 if dt_name == "float32" else 2.0
    dq, dk, dv = q.to(DEV), k.to(DEV), v.to(DEV)
    rc, out = _launch(dq, dk, dv)
    assert rc == 0
    assert bool(torch.isfinite(out).all())
    err_all = (out.cpu().double() - exact).abs()
    err = float(err_all.max())
    adv = max([float(err_all[:, r].max()) for r in rows.values()], default=0.0)
    print("self_attention %s Lq=%d B=%d: max|err| %.3e (adversarial rows %.3e)  yardstick %.3e  ratio %.2f (allowed %.0f)"
          % (dt_name, Lq, B, err, adv, yard, err / yard if yard > 0 else 0.0, margin))
    assert err <= margin * yard
    # two launches give identical bits
    rc2, out2 = _launch(dq, dk, dv)
    assert rc2 == 0 and torch.equal(out.view(torch.int16 if out.dtype == torch.bfloat16 else torch.int32),
                                    out2.view(torch.int16 if out.dtype == torch.bfloat16 else torch.int32))
    if B == 2:
        # nothing crosses the batch: other content in element 1 leaves element 0's rows bit for bit
        q2, k2, v2 = _case(Lq, B, dt_name, 7)[:3]
        assert torch.equal(q2[0], q[0]) and not torch.equal(v2[1], v[1])
        rc3, out3 = _launch(q2.to(DEV), k2.to(DEV), v2.to(DEV))
        assert rc3 == 0 and torch.equal(out3[0].float(), out[0].float()) and not torch.equal(out3[1].float(), out[1].float())


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_self_attention_on_column_blocks_of_a_wider_tensor(dt):
    """q, k as the two halves of one (B, Lq, 512) projection output, v on its own: same bits as from contiguous copies"""
    gen = torch.Generator().manual_seed(5)
    qk = torch.randn(2, 77, 2 * C, generator=gen).to(dt).to(DEV)
    v = torch.randn(2, 77, C, generator=gen).to(dt).to(DEV)
    rc, a = _launch(qk[..., :C], qk[..., C:], v)
    rc2, b = _launch(qk[..., :C].contiguous(), qk[..., C:].contiguous(), v)
    assert rc == 0 and rc2 == 0 and torch.equal(a.float(), b.float())


def test_self_attention_refuses_other_geometries():
    q = torch.zeros(1, 8, C, device=DEV)
    assert _launch(q, q, q, C_=128)[0] == BADARG
    assert _launch(q, q, q, M_=4)[0] == BADARG
    L = _lib()
    out = torch.zeros_like(q)
    args = lambda Lq, dtype: (L.ptr(q), L.ptr(q), L.ptr(q), L.ptr(out), C, C, C, 1, Lq, C, M, dtype, L.stream_ptr())
    assert L.load().mvg_self_attention(*args(0, 0)) == BADARG
    assert L.load().mvg_self_attention(*args(8, 2)) == BADARG


def test_ops_wrapper_checks():
    from mvgformer_amd import ops
    q = torch.zeros(1, 8, C)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.self_attention(q, q, q)
    g = q.to(DEV)
    with pytest.raises(RuntimeError, match="float32 or all bfloat16"):
        ops.self_attention(g, g.bfloat16(), g)
    with pytest.raises(RuntimeError, match="row-major"):
        ops.self_attention(g.expand(2, 8, C), g.expand(2, 8, C), g.expand(2, 8, C))
    with pytest.raises(RuntimeError, match="d_model 256"):
        ops.self_attention(g[..., :128], g[..., :128], g[..., :128])
    x = torch.randn(2, 40, C, device=DEV)
    assert torch.equal(ops.self_attention(x, x, x), _launch(x, x, x)[1])
