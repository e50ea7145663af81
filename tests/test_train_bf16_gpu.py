"""bf16 mixed-precision training path (DQDecoderLayer.set_training_dtype(torch.bfloat16)): the two new kernels
(mvg_msda_backward_det_bf16, mvg_linear_wgrad_bias_bf16), LinearBF16, and the layer / decoder gradients."""
import pytest
import torch

from mvgformer_amd import ops
from mvgformer_amd.factory import build_decoder_for_case, case_to_device
from mvgformer_amd.synthetic import build_case, to_torch_state
from tests.golden.cases import GRAD_CASES, LAYER_CASES, layer_loss

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16


def _case(cname, **kw):
    spec = LAYER_CASES[cname]
    return build_case(spec["config"], B=spec.get("B", 1), seed=spec["seed"], NQ=spec.get("NQ"),
                      layers=spec.get("layers"), valid_fraction=spec.get("valid_fraction"), **kw)


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu() if t.dtype == torch.float32 else t.detach().cpu()


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ 1. sampling backward
def _msda_inputs(N, shapes, Lq, M=8, D=32, P=8, seed=0, empty_image=None, nonfinite=False):
    g = torch.Generator().manual_seed(seed)
    shapes_t = torch.tensor(shapes, dtype=torch.int64)
    starts = torch.cat([torch.zeros(1, dtype=torch.int64), (shapes_t[:, 0] * shapes_t[:, 1]).cumsum(0)[:-1]])
    S = int((shapes_t[:, 0] * shapes_t[:, 1]).sum())
    L = len(shapes)
    value = torch.randn((N, S, M, D), generator=g).to(BF)
    loc = torch.rand((N, Lq, M, L, P, 2), generator=g) * 1.2 - 0.1
    if empty_image is not None:
        loc[empty_image] = -3.0                                   # every sample of this image falls outside its maps
    attn = torch.rand((N, Lq, M, L, P), generator=g)
    attn = attn / attn.sum((-1, -2), keepdim=True)
    gout = torch.randn((N, Lq, M * D), generator=g)
    if nonfinite:
        gout[0, 1, 3] = float("nan")
        gout[N - 1, Lq // 2, 40] = float("inf")
        gout[N - 1, Lq - 1, 7] = -float("inf")
    return [t.to(DEV) for t in (value, shapes_t, starts, loc, attn, gout)]


@pytest.mark.parametrize("kind", ["random", "nonfinite_empty", "cfg2"])
def test_msda_backward_bf16_value_equals_fp32_on_the_upcast_value_bitwise(kind):
    """msda_backward with a bf16 value equals the fp32 call on value.float() in all three outputs, bit for bit (only the patch
    load differs: the bf16 value is widened exactly); NaN / Inf in grad_output stay out of grad_value as in the fp32 form; an
    image without samples gets a zero grad_value; two calls give the same bytes."""
    if kind == "random":
        args = _msda_inputs(3, [[24, 40], [12, 20]], 96, seed=1)
    elif kind == "nonfinite_empty":
        args = _msda_inputs(4, [[17, 29]], 64, seed=2, empty_image=1, nonfinite=True)
    else:
        case = build_case("cfg2", seed=0)
        args = _msda_inputs(case.V * case.tgt.shape[0], case.spatial_shapes.tolist(), case.tgt.shape[1], seed=3)
    value, shapes_t, starts, loc, attn, gout = args
    got = ops.msda_backward(value, shapes_t, starts, loc, attn, gout)
    want = ops.msda_backward(value.float(), shapes_t, starts, loc, attn, gout)
    again = ops.msda_backward(value, shapes_t, starts, loc, attn, gout)
    torch.cuda.synchronize()
    for a, b, c, name in zip(got, want, again, ("grad_value", "grad_loc", "grad_attn")):
        assert a.dtype == torch.float32 and a.shape == b.shape, name
        assert _same_bits(a, b), (kind, name, float((a - b).abs().nan_to_num(0).max()))
        assert _same_bits(a, c), (kind, name)
    assert torch.isfinite(got[0]).all()
    if kind == "nonfinite_empty":
        assert float(got[0][1].abs().max()) == 0.0


def test_msda_backward_bf16_value_falls_back_where_the_deterministic_form_does_not_apply():
    """D != 32: no deterministic workspace -- the fp32 atomic kernel runs on value.float() (before this path, a bf16 value raised)"""
    value, shapes_t, starts, loc, attn, _ = _msda_inputs(2, [[10, 12]], 20, M=4, D=16, seed=4)
    gout = torch.randn((2, 20, 4 * 16), device=DEV)
    got = ops.msda_backward(value, shapes_t, starts, loc, attn, gout)
    want = ops.msda_backward(value.float(), shapes_t, starts, loc, attn, gout)
    for a, b in zip(got, want):
        assert a.dtype == torch.float32
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------------------------ 2. bf16 wgrad
def _wgrad_bar(dy, x, rows, splits):
    """|fl(sum) - sum| <= (terms per slice + slices + 4) * 2^-24 * sum |dy| |x| (fp32 accumulation: one rounding per addition
    along the longest chain, as tests/chain_ref.py bounds its sums)"""
    a = (dy.double().abs().t() @ x.double().abs()).cpu()
    rps = -(-rows // max(splits, 1))
    return (rps + splits + 4) * 2.0 ** -24 * a + 1e-30


@pytest.mark.parametrize("N,K", [(32, 64), (64, 256), (256, 256), (1024, 256), (256, 1024), (1024, 64)])
@pytest.mark.parametrize("rows", [0, 31, 256, 1000, 9000])
def test_linear_wgrad_bias_bf16_against_fp64(N, K, rows):
    """dW = dy^T x and db = sum dy from bf16 operands (fp32 accumulation) against fp64 on the same bf16 values; rows below, at
    and above a slice (256 rows per slice at these sizes) and zero rows; bit-identical on a repeat call."""
    g = torch.Generator(device=DEV).manual_seed(N * 7 + K + rows)
    dy = torch.randn((rows, N), device=DEV, generator=g).to(BF)
    x = torch.randn((rows, K), device=DEV, generator=g).to(BF)
    dw, db = ops.linear_wgrad_bias(dy, x)
    dw2, db2 = ops.linear_wgrad_bias(dy, x)
    torch.cuda.synchronize()
    assert dw.dtype == torch.float32 and dw.shape == (N, K) and db.shape == (N,)
    assert _same_bits(dw, dw2) and _same_bits(db, db2)
    want_w = (dy.double().t() @ x.double()).cpu()
    want_b = dy.double().sum(0).cpu()
    splits = ops._wgrad_splits(max(rows, 1), N, K)
    bar_w = _wgrad_bar(dy, x, rows, splits)
    bar_b = _wgrad_bar(dy, torch.ones((rows, 1), device=DEV), rows, splits)[:, 0]
    assert bool(((dw.double().cpu() - want_w).abs() <= bar_w).all()), float(((dw.double().cpu() - want_w).abs() / bar_w).max())
    assert bool(((db.double().cpu() - want_b).abs() <= bar_b).all())
    if rows == 0:
        assert float(dw.abs().max()) == 0.0 and float(db.abs().max()) == 0.0


@pytest.mark.parametrize("N,K,rows", [(256, 256, 3000), (192, 256, 76800)])
def test_linear_wgrad_bias_bf16_equals_the_split_form_on_bf16_values(N, K, rows):
    """same tiles, slices and k order as mvg_linear_wgrad_bias_f32: on values that are exactly bf16 the split form's lower parts
    are zero and both give the same bits"""
    g = torch.Generator(device=DEV).manual_seed(rows)
    dy = torch.randn((rows, N), device=DEV, generator=g).to(BF)
    x = torch.randn((rows, K), device=DEV, generator=g).to(BF)
    dw, db = ops.linear_wgrad_bias(dy, x)
    dw32, db32 = ops.linear_wgrad_bias(dy.float(), x.float())
    assert _same_bits(dw, dw32) and _same_bits(db, db32)


# ------------------------------------------------------------------------------------------------ 3./4. layer gradients
class _R(torch.autograd.Function):
    """forward: round to bf16 (a kernel's operand load); backward: the gradient passes unchanged"""

    @staticmethod
    def forward(ctx, x):
        return x.to(BF).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


def _round_dy(g):
    """the backward rounding point of the emulations: dy of a bf16 GEMM (and the gradient of a bf16 tensor) is rounded to bf16"""
    return g.to(BF).to(g.dtype)


class _G(torch.autograd.Function):
    """forward: identity; backward: the gradient is rounded to bf16 (_round_dy)"""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return _round_dy(g)


# ------------------------------------------------------------------------------------------------ LinearBF16 alone
def _dot_bar(a, b):
    """elementwise bar of an fp32-accumulated product a @ b^T of bf16-exact operands against fp64: LAMBDA = 8 times the typical
    size of the accumulation error, u sqrt(n) sqrt(sum t^2) for n terms t (tests/chain_ref.py's lin_err), plus the rounding of
    the result.  Rounding dy to bf16 or not moves a result by ~ 2^-9 / sqrt(3) sqrt(sum t^2): 20x and more above this bar."""
    a, b = a.double().cpu(), b.double().cpu()
    n = a.shape[1]
    return 8.0 * 2.0 ** -24 * ((n ** 0.5) * ((a * a) @ (b * b).t()).sqrt() + (a @ b.t()).abs()) + 1e-30


@pytest.mark.parametrize("rows,K,N,relu,bias,xbf", [(4096, 256, 192, False, True, False), (4000, 256, 1024, True, True, False),
                                                    (2048, 1024, 256, False, False, False), (3000, 256, 256, True, True, True)])
def test_linear_bf16_forward_dgrad_wgrad_against_an_fp64_emulation(rows, K, N, relu, bias, xbf):
    """one LinearBF16 (well conditioned, random data) elementwise against fp64 on the documented rounding points: y from
    bf16(x), bf16(W), fp32 bias (+ ReLU); dx = bf16(dy') bf16(W), dW = bf16(dy')^T bf16(x), db = sum bf16(dy'), dy' = dy masked
    by the ReLU of the kernel's own y (a mask flip at y ~ 0 is a forward question, not a rounding point).  The bars are the
    fp32 accumulation's (_dot_bar): an emulation or a kernel that left dy in fp32 fails them."""
    from mvgformer_amd.functions import LinearBF16, bf16_weights
    from mvgformer_amd.projattn import WeightCache
    g = torch.Generator(device=DEV).manual_seed(rows + K + N)
    x = torch.randn((rows, K), device=DEV, generator=g)
    if xbf:
        x = x.to(BF)
    x.requires_grad_(True)
    W = (torch.randn((N, K), device=DEV, generator=g) / K ** 0.5).requires_grad_(True)
    b = (torch.randn((N,), device=DEV, generator=g) * 0.1).requires_grad_(True) if bias else None
    w16, w16t = bf16_weights(WeightCache(), "w", (W,))
    y = LinearBF16.apply(x, W, b, w16, w16t, relu, False)
    dy = torch.randn((rows, N), device=DEV, generator=g)
    y.backward(dy)
    xr, Wr = x.detach().to(BF).double().cpu(), W.detach().to(BF).double().cpu()
    y_em = xr @ Wr.t() + (b.detach().double().cpu() if bias else 0.0)
    y_bar = _dot_bar(xr, Wr)
    if relu:
        y_em = y_em.clamp_min(0.0)
    assert bool(((y.detach().double().cpu() - y_em).abs() <= y_bar).all())
    dym = dy.double().cpu() * ((y.detach().cpu() > 0).double() if relu else 1.0)
    d16 = _round_dy(dym)
    checks = [("dx", x.grad, d16 @ Wr, _dot_bar(d16, Wr.t())),
              ("dW", W.grad, d16.t() @ xr, _dot_bar(d16.t(), xr.t()))]
    if bias:
        ones = torch.ones((1, rows), dtype=torch.float64)
        checks.append(("db", b.grad, d16.sum(0), _dot_bar(d16.t(), ones)[:, 0]))
    for name, got, want, bar in checks:
        if got.dtype == BF:                   # the gradient of a bf16 input is handed back in bf16: one more rounding
            bar = bar + 2.0 ** -8 * want.abs()
        else:
            assert got.dtype == torch.float32, name
        err = (got.detach().double().cpu() - want).abs()
        assert bool((err <= bar).all()), (name, float((err / bar).max()))


def _lin16(x, W, b):
    return _G.apply(_R.apply(x) @ _R.apply(W).t() + b)


def _emulate_layer(O, prm, tgt, query_pos, case, threshold, indices):
    """fp64 emulation of forward_autograd at training dtype bf16: oracle/decoder_ref.py's decoder_layer_forward, its pieces
    reused, with the rounding points of the forward_autograd docstring for a layer run on its own (fp32 maps: the
    reference-point input is fp32 and rounded as the GEMM's operand)."""
    dt = torch.float64
    P_ = lambda n: prm["layers.0." + n]
    B, Lq, C = tgt.shape
    src_views, shapes, lsi, meta = case.src_views, case.spatial_shapes, case.level_start_index, case.meta
    L = len(src_views)
    V = src_views[0].shape[0] // B
    J, M, Pn = 15, 8, 8
    NQ = Lq // J
    img = torch.tensor(case.img_size, dtype=dt)
    WH = shapes.flip(-1).to(dt)
    pa = "proj_attn."
    attn_views, r_views = [], []
    for v in range(V):
        src_v = [s[v * B:(v + 1) * B].to(dt) for s in src_views]
        r, inside = O.project_ref_points(case.reference_points, meta[v]["camera"], meta[v]["center"], meta[v]["scale"],
                                         case.img_size, dt)
        ref_lvl = r.unsqueeze(2) * WH / (WH - 1)
        grid = torch.clamp(ref_lvl * 2.0 - 1.0, -1.1, 1.1)
        feats = torch.stack([O.bilinear_zeros(src_v[l], grid[:, :, l]) for l in range(L)], 2)
        flat = torch.cat([s.flatten(2) for s in src_v], -1).transpose(1, 2)
        value = _G.apply(_R.apply(_lin16(flat, P_(pa + "rayconv.weight"), P_(pa + "rayconv.bias")))).reshape(B, -1, M, C // M)
        x = feats + (tgt + query_pos).unsqueeze(2)
        Woa = torch.cat([P_(pa + "sampling_offsets.weight"), P_(pa + "attention_weights.weight")], 0)
        boa = torch.cat([P_(pa + "sampling_offsets.bias"), P_(pa + "attention_weights.bias")], 0)
        oa = _lin16(x, Woa, boa)
        n_off = P_(pa + "sampling_offsets.weight").shape[0]
        off = oa[..., :n_off].reshape(B, Lq, M, L, Pn, 2)
        aw = torch.softmax(oa[..., n_off:].reshape(B, Lq, M, L * Pn), -1).view(B, Lq, M, L, Pn)
        norm = torch.stack([shapes[:, 1], shapes[:, 0]], -1).to(dt)
        loc = ref_lvl[:, :, None, :, None, :] + off / norm[None, None, None, :, None, :]
        samp = _G.apply(_R.apply(O.msda_forward(value, shapes, lsi, loc, aw)))
        a = _lin16(samp, P_(pa + "output_proj.weight"), P_(pa + "output_proj.bias"))
        attn_views.append(inside.unsqueeze(-1).to(dt) * a)
        r_views.append(r)
    mean = torch.stack(attn_views, 0).mean(0)
    t1 = O._ln(tgt + _lin16(mean, P_("feature_update_mlp.weight"), P_("feature_update_mlp.bias")), P_("norm2.weight"),
               P_("norm2.bias"))
    h = torch.relu(_lin16(t1, P_("linear1.weight"), P_("linear1.bias")))
    tgt_update = O._ln(t1 + _lin16(h, P_("linear2.weight"), P_("linear2.bias")), P_("norm3.weight"), P_("norm3.bias"))
    logits = tgt_update @ P_("class_embed.weight").t() + P_("class_embed.bias")          # 2-output head: fp32 path
    prob = torch.sigmoid(logits.view(B, NQ, J, 2)).mean(2)
    if indices is not None:
        valid = torch.zeros((B, NQ), dtype=torch.bool)
        for b, q in enumerate(indices):
            valid[b, torch.as_tensor(q, dtype=torch.long)] = True
    else:
        valid = prob[..., 1] > threshold
    if not bool(valid.any()):
        valid[0, 0] = True
    ref2d, proj2d, logit = [], [], []
    for v in range(V):
        hcur = torch.relu(_lin16(attn_views[v], P_("pose_embed.MLP.layers.0.weight"), P_("pose_embed.MLP.layers.0.bias")))
        hcur = torch.relu(_lin16(hcur, P_("pose_embed.MLP.layers.1.weight"), P_("pose_embed.MLP.layers.1.bias")))
        o = hcur @ P_("pose_embed.MLP.layers.2.weight").t() + P_("pose_embed.MLP.layers.2.bias")   # 3-output head: fp32 path
        ref2d.append((r_views[v] + o[..., :2] / img) * img)
        proj2d.append(r_views[v] * img)
        logit.append(o[..., 2])
    ref2d, proj2d = torch.stack(ref2d, 1), torch.stack(proj2d, 1)
    conf = torch.softmax(torch.stack(logit, 1), 1)
    cam_q = {k_: v_.repeat_interleave(NQ, 0) for k_, v_ in O._stack_cam(meta, dt).items()}
    kp = ref2d.view(B, V, NQ, J, 2).permute(0, 2, 1, 3, 4).reshape(B * NQ, V, J, 2)
    cf = conf.view(B, V, NQ, J).permute(0, 2, 1, 3).reshape(B * NQ, V, J)
    Ainv = torch.stack([m["inv_affine_trans"][:, :2, :] for m in meta], 1).float().to(dt).repeat_interleave(NQ, 0)
    uo = torch.matmul(torch.cat([kp, torch.ones_like(kp[..., :1])], -1), Ainv.transpose(2, 3))
    X3, _ = O.dlt_triangulate(O.projection_matrices(cam_q, dt), O.undistort_points(uo, cam_q, dt), cf)
    X3 = X3.view(B, NQ, J, 3)
    new_ref = torch.where(valid.view(B, NQ, 1, 1), X3, torch.zeros_like(X3)).reshape(B, Lq, 3)
    vm2 = valid.view(B, 1, NQ, 1, 1)
    ref2d_o = torch.where(vm2, ref2d.view(B, V, NQ, J, 2), torch.zeros((), dtype=dt)).reshape(B, V, Lq, 2)
    proj2d_o = torch.where(vm2, proj2d.view(B, V, NQ, J, 2), torch.zeros((), dtype=dt)).reshape(B, V, Lq, 2)
    return tgt_update, new_ref, ref2d_o, proj2d_o, prob


def _layer_grads(cname, dtype):
    case = _case(cname)
    idx = GRAD_CASES[cname]["indices"]
    thr = LAYER_CASES[cname].get("threshold", 0.1)
    dec = build_decoder_for_case(case, DEV)
    gc = case_to_device(case, DEV)
    layer = dec.layers[0].set_training_dtype(dtype)
    layer.eval()
    tgt = gc.tgt.clone().requires_grad_(True)
    out = layer(tgt, gc.query_pos, gc.reference_points[:, :, None], gc.src_views, gc.spatial_shapes, gc.level_start_index,
                gc.meta, indices=None if idx is None else [torch.tensor(q, device=DEV) for q in idx], threshold=thr)
    layer_loss(out).backward()
    got = {"tgt": tgt.grad}
    got.update({n: p.grad for n, p in layer.named_parameters() if p.grad is not None})
    return got, out


def _fp64_grads(O, cname, emulate):
    case = _case(cname)
    idx = GRAD_CASES[cname]["indices"]
    thr = LAYER_CASES[cname].get("threshold", 0.1)
    prm = {k: v.double().requires_grad_(k.startswith("layers.0.")) for k, v in to_torch_state(case.weights).items()}
    t64 = case.tgt.double().clone().requires_grad_(True)
    if emulate:
        o64 = _emulate_layer(O, prm, t64, case.query_pos.double(), case, thr, idx)
    else:
        o64 = O.decoder_layer_forward(prm, "layers.0.", t64, case.query_pos, case.reference_points, case.src_views,
                                      case.spatial_shapes, case.level_start_index, case.meta, case.img_size, threshold=thr,
                                      dtype=torch.float64, indices=idx)
    layer_loss(o64).backward()
    want = {"tgt": t64.grad}
    want.update({k[len("layers.0."):]: v.grad for k, v in prm.items() if v.grad is not None})
    return want


@pytest.fixture(scope="module")
def O():
    from oracle import decoder_ref
    return decoder_ref


def _fro_cos(a, w):
    a = a.detach().double().cpu().reshape(-1)
    w = w.detach().double().cpu().reshape(-1)
    return float((a - w).norm() / w.norm().clamp_min(1e-300)), float(a @ w / (a.norm() * w.norm()).clamp_min(1e-300))


@pytest.mark.parametrize("cname", ["mini5_all", "mini5_half", "mini5_b2"])
def test_layer_gradients_bf16_against_the_bf16_emulation(cname, O):
    """d(loss)/d(tgt) and d(loss)/d(every trained parameter) of the bf16 training path against an fp64 autograd emulation that
    rounds to bf16 at the documented points (forward: GEMM operands, the value and the sampling output; backward: dy of every
    bf16 GEMM and the gradients of the bf16 tensors); the same tensors receive a gradient as on the fp32 path.  Teacher-forced
    GRAD_CASES (the filter's outcome is fixed).

    Elementwise agreement is not attainable on these cases: where an fp32 value and its fp64 emulation sit on opposite sides
    of a bf16 rounding boundary or of a ReLU's zero, the two take different branches, and these synthetic layers are
    sensitive to that -- the emulation itself is 0.4 x absmax (max-abs) / 0.19 (Frobenius) away from plain fp64 on the pose
    MLP.  Per tensor, measured on MI355X: relative Frobenius error <= 3.5e-2 (pose_embed.MLP.layers.0, mini5_all; <= 1.3e-2
    on everything outside the pose MLP and linear1), cosine >= 0.99939 -- bars 5e-2 / 0.999.  And the emulation is the
    nearer reference: summed over the tensors, the distance to it is below 0.6 x the distance to plain fp64 (measured
    0.25-0.4).  These bars cannot see the backward rounding of dy (an emulation without it moves by <= 5e-3 per tensor):
    test_linear_bf16_forward_dgrad_wgrad_against_an_fp64_emulation checks that rounding point elementwise."""
    got, _ = _layer_grads(cname, BF)
    ref32, _ = _layer_grads(cname, torch.float32)
    assert set(got) == set(ref32), set(got) ^ set(ref32)
    want = _fp64_grads(O, cname, emulate=True)
    plain = _fp64_grads(O, cname, emulate=False)
    d_em = d_64 = 0.0
    for n, g in got.items():
        fro, cos = _fro_cos(g, want[n])
        assert torch.isfinite(g).all() and fro <= 5e-2 and cos >= 0.999, (n, fro, cos)
        d_em += fro
        d_64 += _fro_cos(g, plain[n])[0]
    print("bf16 vs emulation, %s: summed Frobenius distance %.3f, to plain fp64 %.3f" % (cname, d_em, d_64))
    assert d_em < 0.6 * d_64, (d_em, d_64)


@pytest.mark.parametrize("cname", ["mini5_all", "mini5_half", "mini5_b2"])
def test_layer_gradients_bf16_against_plain_fp64(cname, O):
    """sanity against the fp64 oracle without any bf16 rounding: finite, and per tensor a relative Frobenius error <= 0.25 and a
    cosine >= 0.98 (measured on MI355X: <= 0.185 and >= 0.9827, both pose_embed.MLP.layers.1.bias on mini5_b2 -- the
    emulation of the bf16 rounding points is as far from fp64 there, see the test above)"""
    got, _ = _layer_grads(cname, BF)
    want = _fp64_grads(O, cname, emulate=False)
    for n, g in got.items():
        assert torch.isfinite(g).all(), n
        fro, cos = _fro_cos(g, want[n])
        assert fro <= 0.25 and cos >= 0.98, (n, fro, cos)


# ------------------------------------------------------------------------------------------------ 5. four layers at cfg-2
def _decoder_step(dec, g):
    for p in dec.parameters():
        p.grad = None
    out = dec(g.tgt, g.reference_points, g.src_views, g.meta, g.spatial_shapes, g.level_start_index, None,
              query_pos=g.query_pos, threshold=0.1)
    loss = out[0].float().pow(2).mean() + 1e-6 * out[1].float().pow(2).mean() + sum(c.float().sum() for c in out[4]) * 1e-3
    loss.backward()
    return {n: p.grad.clone() for n, p in dec.named_parameters() if p.grad is not None}


def test_four_layer_decoder_cfg2_bf16_step_is_finite_and_reproducible():
    """a bf16 forward + backward of the 4-layer decoder at cfg-2 gives finite gradients for every parameter that gets one in
    fp32; a second identical step (eval(): dropout off) gives the same bits"""
    case = build_case("cfg2", seed=0)
    dec = build_decoder_for_case(case, DEV, torch.float32)
    g = case_to_device(case, DEV)
    for p in dec.parameters():
        p.requires_grad_(True)
    dec.eval()
    g32 = _decoder_step(dec, g)
    dec.set_training_dtype(BF)
    g16 = _decoder_step(dec, g)
    g16b = _decoder_step(dec, g)
    torch.cuda.synchronize()
    assert set(g16) == set(g32), set(g16) ^ set(g32)
    for n in g16:
        assert torch.isfinite(g16[n]).all(), n
        assert _same_bits(g16[n], g16b[n]), n


def test_four_layer_decoder_cfg2_bf16_step_on_a_bf16_packed_pyramid(monkeypatch):
    """compute_dtype bf16 as well: the decoder packs the pyramid in bf16 and the bf16 training path takes it as it is (rayconv on the
    bf16 pyramid, the reference-point gather from it through RefGatherAdd).  Finite gradients on the same tensors as with the
    fp32 pyramid, bit-identical on a repeat, and close to the fp32-pyramid bf16 step (per tensor cosine >= 0.98; measured
    >= 0.9916 on MI355X)."""
    case = build_case("cfg2", seed=0)
    dec = build_decoder_for_case(case, DEV, torch.float32).set_training_dtype(BF)
    g = case_to_device(case, DEV)
    for p in dec.parameters():
        p.requires_grad_(True)
    dec.eval()
    ref = _decoder_step(dec, g)
    dec.set_compute_dtype(BF)
    seen = []
    gather = ops.gather_ref
    monkeypatch.setattr(ops, "gather_ref", lambda feat, *a: seen.append(feat.dtype) or gather(feat, *a))
    got = _decoder_step(dec, g)
    again = _decoder_step(dec, g)
    torch.cuda.synchronize()
    assert seen and all(d == BF for d in seen), seen        # the reference-point gather read the bf16 pyramid
    assert set(got) == set(ref), set(got) ^ set(ref)
    worst = 1.0
    for n in got:
        assert torch.isfinite(got[n]).all(), n
        assert _same_bits(got[n], again[n]), n
        a, w = got[n].double().reshape(-1), ref[n].double().reshape(-1)
        cos = float(a @ w / (a.norm() * w.norm()).clamp_min(1e-300))
        worst = min(worst, cos)
        assert cos >= 0.98, (n, cos)
    print("bf16 pyramid vs fp32 pyramid, worst cosine %.6f" % worst)


# ------------------------------------------------------------------------------------------------ 6. no effect at the default
def test_switching_back_to_fp32_is_the_fp32_path_bit_for_bit():
    """a layer trained one step in bf16 and switched back to fp32 gives a fresh fp32 layer's outputs and gradients bit for bit
    (no bf16 cache leaks into the fp32 path), and the native inference outputs are unchanged by the bf16 step"""
    cname = "mini5_half"
    fresh, out_f = _layer_grads(cname, torch.float32)
    case = _case(cname)
    thr = LAYER_CASES[cname].get("threshold", 0.1)
    dec = build_decoder_for_case(case, DEV)
    gc = case_to_device(case, DEV)
    layer = dec.layers[0]
    layer.eval()
    args = (gc.query_pos, gc.reference_points[:, :, None], gc.src_views, gc.spatial_shapes, gc.level_start_index, gc.meta)
    with torch.no_grad():
        inf0 = layer(gc.tgt, *args, threshold=thr)
    layer.set_training_dtype(BF)
    layer_loss(layer(gc.tgt.clone().requires_grad_(True), *args, threshold=thr)).backward()
    with torch.no_grad():
        inf1 = layer(gc.tgt, *args, threshold=thr)
    for a, b in zip(inf0, inf1):
        assert _same_bits(a, b)
    layer.set_training_dtype(torch.float32)
    layer.zero_grad(set_to_none=True)
    tgt = gc.tgt.clone().requires_grad_(True)
    out = layer(tgt, *args, threshold=thr)
    layer_loss(out).backward()
    got = {"tgt": tgt.grad}
    got.update({n: p.grad for n, p in layer.named_parameters() if p.grad is not None})
    assert set(got) == set(fresh)
    for a, b in zip(out, out_f):
        assert _same_bits(a, b)
    for n in got:
        assert _same_bits(got[n], fresh[n]), n


# ------------------------------------------------------------------------------------------------ 7. short training run
def _train(dtype, steps=30):
    torch.manual_seed(0)
    case = build_case("mini5", seed=3, layers=2)
    dec = build_decoder_for_case(case, DEV, torch.float32).set_training_dtype(dtype)
    g = case_to_device(case, DEV)
    dec.eval()
    for p in dec.parameters():
        p.requires_grad_(True)
    target = torch.randn(tuple(g.tgt.shape), generator=torch.Generator().manual_seed(1)).to(DEV)
    opt = torch.optim.Adam(dec.parameters(), lr=1e-3)
    losses = []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        hs = dec(g.tgt, g.reference_points, g.src_views, g.meta, g.spatial_shapes, g.level_start_index, None,
                 query_pos=g.query_pos, threshold=0.1)[0]
        loss = (hs[-1].float() - target).pow(2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    return losses


def test_short_adam_run_bf16_follows_fp32():
    """30 Adam steps (fp32 master weights) from the same seed: the bf16 loss falls and ends within 5 % of the fp32 run's"""
    l32 = _train(torch.float32)
    l16 = _train(BF)
    assert l16[-1] < 0.9 * l16[0], l16
    assert abs(l16[-1] - l32[-1]) <= 0.05 * l32[-1], (l16[-1], l32[-1])
