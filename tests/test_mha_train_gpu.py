"""The self-attention training kernels (csrc/mha.hip: mvg_self_attention_train, mvg_self_attention_backward,
mvg_self_attention_dropout_mask) against the fp64 statement of tests/mha_train_ref.py: raw C-ABI launches into guarded buffers,
the inputs of tests/test_mha_fp64.py (adversarial rows included) plus a seeded dout, every element of every output compared.
The bounds are measured on the spot from the same inputs:
  lse   max |err| <= 4 x the max |err| of torch.logsumexp in fp32 on the CPU from fp32 scores;
  fp32  per tensor, max |err| <= 4 x max(A, B): A the error of torch's own fp32 autograd on the CPU (through
        multi_head_attention_forward without dropout; through softmax o Z with a given mask, which that operator cannot take),
        B the error of mha_train_ref.flash_backward in fp32 on the CPU -- recomputing P from an fp32 lse costs a correct
        implementation up to 10 x A on these rows, and at Lq = 1 A is exactly 0 for dq and dk.  The margin is the forward's
        (tests/test_mha_fp64.py): another summation order;
  bf16  per tensor, max |err| <= 2 x the error of mha_train_ref.flash_backward_bf16_model (the margin is the forward's: the
        model rounds at another scale).  The model's backward reads delta from the `out` the backward under test was given
        (stored_out), as the kernel does: the backward is a function of (q, k, v, out, dout, lse), and on these rows which way
        ONE element of a stored bf16 `out` was rounded moves the model's own dk error by 3.4 x (Lq = 33: 2.3e-2 from the
        model's own out, 7.8e-2 from bf16(exact out)) -- both of them outputs the forward's own test accepts.  `out` itself is
        held to the model's own forward.
Each comparison prints error, yardstick and ratio."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import mha_ref as R
from tests import mha_train_ref as T
from tests import test_mha_fp64 as base

pytestmark = pytest.mark.gpu
DEV, GUARD, SENT, BADARG = base.DEV, base.GUARD, base.SENT, base.BADARG
C, M, D = base.C, base.M, base.D
P_DROP, P_Q = 0.1, 26 / 256
SEED = 0x5EED0123456789


def _L():
    from mvgformer_amd import _lib as L
    return L


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _seed(value=SEED):
    return torch.tensor([value], dtype=torch.int64, device=DEV)


def _mask(B, Lq, seed, p=P_DROP):
    from mvgformer_amd import ops
    return ops.self_attention_dropout_mask(B, Lq, p, seed)


@functools.lru_cache(maxsize=None)
def _inputs(Lq, B, dt_name, variant=0):
    q, k, v = base._case(Lq, B, dt_name, variant)[:3]
    dout = torch.randn(B, Lq, C, generator=torch.Generator().manual_seed(4242 + Lq)).to(q.dtype)
    return q, k, v, dout


def _refs(q, k, v, dout, Z, stored_out, exact=None):
    """exact fp64 results and the yardstick per tensor (module docstring); stored_out: the `out` the backward under test read"""
    exact = exact or T.statement(q, k, v, dout, Z)
    err = lambda got, name: float((got.detach().double() - exact[name]).abs().max())     # noqa: E731
    yard = {}
    s32 = (R._heads(q.float(), M) @ R._heads(k.float(), M).transpose(-1, -2)) / D ** 0.5
    yard["lse"] = err(torch.logsumexp(s32, -1), "lse")
    if q.dtype == torch.float32:
        leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
        if Z is None:
            eye3, eye, z3, z = torch.eye(C).repeat(3, 1), torch.eye(C), torch.zeros(3 * C), torch.zeros(C)
            y = F.multi_head_attention_forward(*(t.transpose(0, 1) for t in leaves), C, M, eye3, z3, None, None, False, 0.0, eye, z,
                                               training=False, need_weights=True)[0].transpose(0, 1)
        else:
            p = torch.softmax((R._heads(leaves[0], M) @ R._heads(leaves[1], M).transpose(-1, -2)) / D ** 0.5, -1) * Z.float()
            y = T._unheads(p @ R._heads(leaves[2], M))
        a = dict(zip(T.NAMES, (y.detach(),) + torch.autograd.grad(y, leaves, dout)))
        b = T.flash_backward(q, k, v, dout, Z, torch.float32)
        for name in T.NAMES:
            yard[name] = max(err(a[name], name), err(b[name], name))
    else:
        model = T.flash_backward_bf16_model(q, k, v, dout, Z, stored_out=stored_out.cpu())
        for name in T.NAMES:
            yard[name] = err(model[name], name)
    return exact, yard


@functools.lru_cache(maxsize=None)
def _exact(Lq, B, dt_name):
    return T.statement(*_inputs(Lq, B, dt_name), None)


def _guarded(shape, dtype):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((GUARD + n + GUARD,), SENT, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _check_guards(bufs, rc):
    for buf in bufs:
        sent = torch.tensor(SENT, dtype=buf.dtype).item()
        n = buf.numel() - 2 * GUARD
        assert bool((buf[:GUARD] == sent).all()) and bool((buf[GUARD + n:] == sent).all()), "guard region overwritten"
        if rc != 0:
            assert bool((buf == sent).all()), "a refused call wrote its output"


def _train(q, k, v, p=0.0, seed=None, C_=C, M_=M, lse_null=False):
    """raw launch of mvg_self_attention_train -> (code, out, lse)"""
    L = _L()
    B, Lq = q.shape[:2]
    obuf, out = _guarded((B, Lq, C), q.dtype)
    lbuf, lse = _guarded((B, M, Lq), torch.float32)
    rc = L.load().mvg_self_attention_train(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(out), None if lse_null else L.ptr(lse), q.stride(1),
                                           k.stride(1), v.stride(1), B, Lq, C_, M_, L.dtype_code(q.dtype), p, L.ptr(seed), L.stream_ptr())
    torch.cuda.synchronize()
    _check_guards((obuf, lbuf), rc)
    return rc, out.clone(), lse.clone()


def _backward(q, k, v, out, dout, lse, p=0.0, seed=None, wide=False, ws_short=0, null=None, C_=C, M_=M):
    """raw launch of mvg_self_attention_backward -> (code, dq, dk, dv); wide: dq, dk as the column blocks of one (B, Lq, 512)"""
    L = _L()
    B, Lq = q.shape[:2]
    if wide:
        qkbuf, dqk = _guarded((B, Lq, 2 * C), q.dtype)
        dq, dk = dqk[..., :C], dqk[..., C:]
        bufs = [qkbuf]
    else:
        (qbuf, dq), (kbuf, dk) = _guarded((B, Lq, C), q.dtype), _guarded((B, Lq, C), q.dtype)
        bufs = [qbuf, kbuf]
    vbuf, dv = _guarded((B, Lq, C), q.dtype)
    nbytes = int(L.load().mvg_self_attention_backward_workspace(B, Lq))
    assert nbytes == B * M * Lq * 4
    wbuf, ws = _guarded((nbytes // 4,), torch.float32)
    ptr = lambda name, t: None if name == null else L.ptr(t)      # noqa: E731
    rc = L.load().mvg_self_attention_backward(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(out), L.ptr(dout), ptr("lse", lse), ptr("dq", dq),
                                              ptr("dk", dk), ptr("dv", dv), q.stride(1), k.stride(1), v.stride(1), dq.stride(1),
                                              dk.stride(1), dv.stride(1), B, Lq, C_, M_, L.dtype_code(q.dtype), p, L.ptr(seed),
                                              ptr("ws", ws), nbytes - ws_short, L.stream_ptr())
    torch.cuda.synchronize()
    _check_guards(bufs + [vbuf], rc)
    _check_guards([wbuf], 0)
    if rc != 0:
        assert bool((wbuf == SENT).all()), "a refused call wrote its workspace"
    return rc, dq.clone(), dk.clone(), dv.clone()


def _compare(tag, got, exact, yard, margin):
    bad = []
    for name, t in got.items():
        assert bool(torch.isfinite(t).all()), name
        err = float((t.detach().cpu().double() - exact[name]).abs().max())
        ratio = err / yard[name] if yard[name] > 0 else (0.0 if err == 0 else float("inf"))
        print("%s %-3s: max|err| %.3e  yardstick %.3e  ratio %.2f (allowed %.0f)  largest entry %.3g"
              % (tag, name, err, yard[name], ratio, margin[name], float(exact[name].abs().max())))
        if not err <= margin[name] * yard[name]:
            bad.append(name)
    assert not bad, bad


def _margins(dt_name):
    m = dict.fromkeys(T.NAMES, 4.0 if dt_name == "float32" else 2.0)
    m["lse"] = 4.0
    return m


@pytest.mark.parametrize("dt_name", ["float32", "bfloat16"])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("Lq", base.LQS)
def test_forward_and_backward_vs_fp64(Lq, B, dt_name):
    q, k, v, dout = _inputs(Lq, B, dt_name)
    dev = [t.to(DEV) for t in (q, k, v, dout)]
    rc, out, lse = _train(*dev[:3])
    assert rc == 0
    rc0, out0 = base._launch(*dev[:3])
    assert rc0 == 0 and torch.equal(_bits(out), _bits(out0)), "out differs from mvg_self_attention's"
    rc, dq, dk, dv = _backward(*dev[:3], out, dev[3], lse)
    assert rc == 0
    exact, yard = _refs(q, k, v, dout, None, out, _exact(Lq, B, dt_name))
    _compare("%s Lq=%d B=%d" % (dt_name, Lq, B), dict(lse=lse, dq=dq, dk=dk, dv=dv), exact, yard, _margins(dt_name))
    # two launches give identical bits
    rc, out2, lse2 = _train(*dev[:3])
    again = _backward(*dev[:3], out2, dev[3], lse2)
    assert rc == 0 and again[0] == 0 and torch.equal(lse, lse2)
    for a, b in zip((dq, dk, dv), again[1:]):
        assert torch.equal(_bits(a), _bits(b))
    if B == 2:
        # nothing crosses the batch: other content in element 1 leaves element 0 bit for bit
        other = [t.to(DEV) for t in _inputs(Lq, B, dt_name, 7)]
        assert torch.equal(other[0][0], dev[0][0]) and not torch.equal(other[2][1], dev[2][1])
        rc, out3, lse3 = _train(*other[:3])
        res = _backward(*other[:3], out3, other[3], lse3)
        assert rc == 0 and res[0] == 0 and torch.equal(lse3[0], lse[0]) and not torch.equal(lse3[1], lse[1])
        for a, b in zip((dq, dk, dv), res[1:]):
            assert torch.equal(_bits(a[0]), _bits(b[0]))
        # ... and is seen in element 1 (at Lq = 1, dq = dk = 0 and dv = dout whatever the content: out and lse show it)
        assert not torch.equal(_bits(out3[1]), _bits(out[1]))
        assert Lq == 1 or not any(torch.equal(_bits(a[1]), _bits(b[1])) for a, b in zip((dq, dk, dv), res[1:]))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_column_blocks_of_wider_tensors(dt):
    """q, k as the halves of one (B, Lq, 512) projection output, and dq, dk written into the halves of one (B, Lq, 512) gradient:
    the bits of contiguous copies"""
    gen = torch.Generator().manual_seed(5)
    qk = torch.randn(2, 77, 2 * C, generator=gen).to(dt).to(DEV)
    v, dout = (torch.randn(2, 77, C, generator=gen).to(dt).to(DEV) for _ in range(2))
    qc, kc = qk[..., :C].contiguous(), qk[..., C:].contiguous()
    rc, out, lse = _train(qk[..., :C], qk[..., C:], v)
    rc2, out2, lse2 = _train(qc, kc, v)
    assert rc == 0 and rc2 == 0 and torch.equal(_bits(out), _bits(out2)) and torch.equal(lse, lse2)
    ref = _backward(qc, kc, v, out, dout, lse)
    for res in (_backward(qk[..., :C], qk[..., C:], v, out, dout, lse), _backward(qc, kc, v, out, dout, lse, wide=True),
                _backward(qk[..., :C], qk[..., C:], v, out, dout, lse, wide=True)):
        assert res[0] == 0 and ref[0] == 0
        for a, b in zip(ref[1:], res[1:]):
            assert torch.equal(_bits(a), _bits(b))


def test_refused_calls_write_nothing():
    q = torch.randn(1, 8, C, device=DEV)
    seed = _seed()
    rc, out, lse = _train(q, q, q)
    assert rc == 0
    assert _train(q, q, q, C_=128)[0] == BADARG and _train(q, q, q, M_=4)[0] == BADARG
    assert _train(q, q, q, lse_null=True)[0] == BADARG
    for p in (-0.1, 1.0, 1.5, float("nan")):
        assert _train(q, q, q, p, seed)[0] == BADARG
        assert _backward(q, q, q, out, q, lse, p, seed)[0] == BADARG
    assert _train(q, q, q, 0.1, None)[0] == BADARG
    assert _backward(q, q, q, out, q, lse, 0.1, None)[0] == BADARG
    assert _backward(q, q, q, out, q, lse, C_=128)[0] == BADARG and _backward(q, q, q, out, q, lse, M_=4)[0] == BADARG
    for null in ("lse", "dq", "dk", "dv", "ws"):
        assert _backward(q, q, q, out, q, lse, null=null)[0] == BADARG
    assert _backward(q, q, q, out, q, lse, ws_short=4)[0] == BADARG
    assert _backward(q, q, q, out, q, lse)[0] == 0
    L = _L()
    assert L.load().mvg_self_attention_backward_workspace(0, 8) == 0 and L.load().mvg_self_attention_backward_workspace(1, 0) == 0
    mask = torch.zeros(1, M, 8, 8, dtype=torch.uint8, device=DEV)
    args = lambda Lq, p, s: (L.ptr(mask), 1, Lq, p, L.ptr(s), L.stream_ptr())     # noqa: E731
    assert L.load().mvg_self_attention_dropout_mask(*args(1025, 0.1, seed)) == BADARG
    assert L.load().mvg_self_attention_dropout_mask(*args(8, 0.1, None)) == BADARG
    assert L.load().mvg_self_attention_dropout_mask(*args(8, 1.0, seed)) == BADARG
    torch.cuda.synchronize()
    assert not bool(mask.any())
    assert L.load().mvg_self_attention_dropout_mask(*args(8, 0.0, None)) == 0
    torch.cuda.synchronize()
    assert bool((mask == 1).all())


def test_ops_wrapper_checks():
    from mvgformer_amd import ops
    g = torch.zeros(1, 8, C, device=DEV)
    lse = torch.zeros(1, M, 8, device=DEV)
    like = lambda t: torch.zeros(t.shape, dtype=t.dtype, device=DEV)      # noqa: E731
    for call in (lambda *a: ops.self_attention_train(*a), lambda *a: ops.self_attention_backward(*a, like(a[0]), like(a[0]), lse)):
        with pytest.raises(RuntimeError, match="float32 or all bfloat16"):
            call(g, g.bfloat16(), g)
        with pytest.raises(RuntimeError, match="row-major"):
            call(g.expand(2, 8, C), g.expand(2, 8, C), g.expand(2, 8, C))
        with pytest.raises(RuntimeError, match="d_model 256"):
            call(g[..., :128], g[..., :128], g[..., :128])
    with pytest.raises(RuntimeError, match="needs seed"):
        ops.self_attention_train(g, g, g, 0.1)
    with pytest.raises(RuntimeError, match="p_drop"):
        ops.self_attention_train(g, g, g, 1.0, _seed())
    x, dout = torch.randn(2, 40, C, device=DEV), torch.randn(2, 40, C, device=DEV)
    out, lse = ops.self_attention_train(x, x, x)
    rc, out_raw, lse_raw = _train(x, x, x)
    assert torch.equal(out, out_raw) and torch.equal(lse, lse_raw) and torch.equal(out, ops.self_attention(x, x, x))
    for a, b in zip(ops.self_attention_backward(x, x, x, out, dout, lse), _backward(x, x, x, out, dout, lse)[1:]):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------ dropout
def _within(tag, got, want, n, sigmas=5.0):
    sigma = (want * (1.0 - want) / n) ** 0.5
    print("%s: %.6f  expected %.6f  (%.2f sigma, allowed %.0f)" % (tag, got, want, abs(got - want) / sigma, sigmas))
    assert abs(got - want) <= sigmas * sigma, tag


def test_mask_statistics():
    B, Lq = 2, 129
    keep = _mask(B, Lq, _seed()).cpu().bool()
    assert keep.shape == (B, M, Lq, Lq)
    k = 1.0 - P_Q
    _within("kept", keep.float().mean().item(), k, keep.numel())
    for b in range(B):
        for h in range(M):
            _within("kept (%d, %d)" % (b, h), keep[b, h].float().mean().item(), k, Lq * Lq)
    both = keep[..., :, 1:] & keep[..., :, :-1]
    _within("both kept, neighbouring keys", both.float().mean().item(), k * k, both.numel())
    both = keep[..., 1:, :] & keep[..., :-1, :]
    _within("both kept, neighbouring queries", both.float().mean().item(), k * k, both.numel())
    other = _mask(B, Lq, _seed(SEED + 1)).cpu().bool()
    _within("agreement with another seed", (keep == other).float().mean().item(), k * k + P_Q * P_Q, keep.numel())
    # the mask of element 0 does not change with B; p = 0 keeps everything
    assert torch.equal(_mask(1, Lq, _seed()).cpu().bool()[0], keep[0])
    assert bool(_mask(1, 33, _seed(), 0.0).all())


@pytest.mark.parametrize("dt_name", ["float32", "bfloat16"])
@pytest.mark.parametrize("Lq", [65, 129, 975])
def test_dropout_forward_and_backward_vs_fp64_with_the_exported_mask(Lq, dt_name):
    B = 2
    q, k, v, dout = _inputs(Lq, B, dt_name)
    seed = _seed()
    Z = _mask(B, Lq, seed).cpu().double() / (1.0 - P_Q)
    dev = [t.to(DEV) for t in (q, k, v, dout)]
    rc, out, lse = _train(*dev[:3], P_DROP, seed)
    assert rc == 0
    rc, dq, dk, dv = _backward(*dev[:3], out, dev[3], lse, P_DROP, seed)
    assert rc == 0
    exact, yard = _refs(q, k, v, dout, Z, out)
    _compare("dropout %s Lq=%d" % (dt_name, Lq), dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv), exact, yard, _margins(dt_name))
    # the same seed gives the same bits, another seed does not
    rc, out2, lse2 = _train(*dev[:3], P_DROP, _seed())
    res = _backward(*dev[:3], out2, dev[3], lse2, P_DROP, _seed())
    assert rc == 0 and res[0] == 0 and torch.equal(_bits(out), _bits(out2)) and torch.equal(lse, lse2)
    for a, b in zip((dq, dk, dv), res[1:]):
        assert torch.equal(_bits(a), _bits(b))
    rc, out3, lse3 = _train(*dev[:3], P_DROP, _seed(SEED + 1))
    res = _backward(*dev[:3], out3, dev[3], lse3, P_DROP, _seed(SEED + 1))
    assert rc == 0 and res[0] == 0 and torch.equal(lse, lse3) and not torch.equal(_bits(out), _bits(out3))
    for a, b in zip((dq, dk, dv), res[1:]):
        assert not torch.equal(_bits(a), _bits(b))
    # p = 0 with any seed gives the no-dropout bits
    rc, out4, lse4 = _train(*dev[:3], 0.0, seed)
    rc0, out0, lse0 = _train(*dev[:3])
    assert rc == 0 and rc0 == 0 and torch.equal(_bits(out4), _bits(out0)) and torch.equal(lse4, lse0)
    for a, b in zip(_backward(*dev[:3], out0, dev[3], lse0, 0.0, seed)[1:], _backward(*dev[:3], out0, dev[3], lse0)[1:]):
        assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("dt_name", ["float32", "bfloat16"])
def test_functions_self_attention_under_a_captured_graph(dt_name):
    """forward + backward at p = 0.1 captured once: every replay draws a new seed on the device, and the last replay is the fp64
    statement with the mask exported from the seed tensor the graph holds"""
    from mvgformer_amd import functions as Fn
    B, Lq = 2, 129
    q, k, v, dout = _inputs(Lq, B, dt_name)
    dq_, dk_, dv_, dout_ = (t.to(DEV) for t in (q, k, v, dout))
    leaves = [t.requires_grad_(True) for t in (dq_, dk_, dv_)]

    def step():
        seed = Fn.attention_seed(DEV)
        out = Fn.self_attention(*leaves, dropout_p=P_DROP, training=True, seed=seed)
        return (seed, out) + torch.autograd.grad(out, leaves, dout_)

    torch.manual_seed(11)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = step()
    torch.cuda.current_stream().wait_stream(side)
    assert eager[1].dtype == q.dtype and all(g.dtype == q.dtype for g in eager[2:])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = step()
    runs = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        runs.append([t.clone() for t in held])
    assert not torch.equal(runs[0][0], runs[1][0]), "the graph replays one seed"
    for a, b in zip(runs[0][1:], runs[1][1:]):
        assert not torch.equal(_bits(a), _bits(b))
    Z = _mask(B, Lq, runs[1][0]).cpu().double() / (1.0 - P_Q)
    exact, yard = _refs(q, k, v, dout, Z, runs[1][1])
    _compare("graph %s" % dt_name, dict(zip(T.NAMES, runs[1][1:])), exact, yard, _margins(dt_name))
    # without a capture torch.manual_seed repeats the run
    torch.manual_seed(11)
    again = step()
    torch.cuda.synchronize()
    assert torch.equal(again[0], eager[0]) and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(again[1:], eager[1:]))
