"""The init_self_attention block trained on the project's own kernels (DQDecoderLayer.set_self_attention_training("native"),
_attend_queries_native): the block against fp64 autograd, the layer under autograd against the default backend, train() mode
with attention dropout, and the whole training step captured as one HIP graph (factory.build_graphed_train_step).  The layers are
those of tests/selfattn_cases.py (mini5, Lq = 150, B = 2); the graphed step runs tests/test_train_graph_gpu.py's case on a
decoder with the switch on."""
import functools
from types import SimpleNamespace as NS

import pytest
import torch

from tests import mha_ref as R
from tests import mha_train_ref as T
from tests import test_train_graph_gpu as G
from tests.selfattn_cases import SPEC, build_decoder
from tests.test_hip_parity import TOL
from tests.test_selfattn_gpu import _layer_args, _setup

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
THR = SPEC["threshold"]
NAMES = ["self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
         "norm2.weight", "norm2.bias"]


def _layer(backend="native", tdt=F32):
    """layer 0 of the shared fp32 decoder, eval mode, with the backend and training dtype set; callers put both back"""
    c, dec = _setup(F32)
    layer = dec.layers[0]
    layer.set_self_attention_training(backend).set_training_dtype(tdt)
    layer.zero_grad(set_to_none=True)
    return c, layer


def _reset(layer):
    layer.set_self_attention_training("torch").set_training_dtype(F32)
    layer.eval().zero_grad(set_to_none=True)


def _functional(out, w, w2):
    """seeded, with a quadratic term: under a LINEAR functional d/d norm2.bias is the column sum of w -- it never sees the block's
    output, so it would check nothing of the attention (and the bf16 model's error for it, hence its bound, would be exactly 0,
    which no fp32 sum of 90 rows meets: torch's LayerNorm backward measured 4.8e-6 there).  With the quadratic term every listed
    gradient, norm2.bias included, depends on the attended output."""
    return (out * w).sum() + 0.5 * (out * out * w2).sum()


def _block_grads(layer, tgt, pos, w, w2):
    tg = tgt.to(DEV).requires_grad_(True)
    with torch.enable_grad():
        out = layer._attend_queries_autograd(tg, pos.to(DEV))
        _functional(out, w.to(DEV), w2.to(DEV)).backward()
    prm = dict(layer.named_parameters())
    got = dict(zip(["tgt"] + NAMES, [tg.grad] + [prm[n].grad for n in NAMES]))
    got = {n: g.detach().cpu().double() for n, g in got.items()}
    layer.zero_grad(set_to_none=True)
    return out.detach().cpu().double(), got


def _block_fp64(layer, tgt, pos, w, w2, attend):
    prm = dict(layer.named_parameters())
    p64 = [prm[n].detach().cpu().double().requires_grad_(True) for n in NAMES]
    t64 = tgt.double().requires_grad_(True)
    out = R.block(t64, pos, *p64, attend=attend)
    _functional(out, w.double(), w2.double()).backward()
    return out.detach(), dict(zip(["tgt"] + NAMES, [t64.grad] + [p.grad for p in p64]))


@functools.lru_cache(maxsize=None)
def _block_case(tdt):
    """native block at Lq = 45, B = 2, eval mode -> (|out| error, its bound, {tensor: (error, bound, largest gradient)})"""
    c, layer = _layer("native", tdt)
    try:
        gen = torch.Generator().manual_seed(45)
        tgt, pos, w, w2 = (torch.randn(2, 45, 256, generator=gen) for _ in range(4))
        out, got = _block_grads(layer, tgt, pos, w, w2)
        want_out, want = _block_fp64(layer, tgt, pos, w, w2, T.attention_fn())
        if tdt == F32:
            out_bound = TOL["hs"]
            bound = {n: 1e-4 * float(want[n].abs().max()) for n in want}
        else:
            model_out, model = _block_fp64(layer, tgt, pos, w, w2, T.attention_fn(bf16_model=True))
            out_bound = 2 * float((model_out - want_out).abs().max())
            bound = {n: 2 * float((model[n] - want[n]).abs().max()) for n in want}
        return float((out - want_out).abs().max()), out_bound, {n: (float((got[n] - want[n]).abs().max()), bound[n],
                                                                    float(want[n].abs().max())) for n in want}
    finally:
        _reset(layer)


@pytest.mark.parametrize("name", ["out", "tgt"] + NAMES)
@pytest.mark.parametrize("tdt", [F32, BF16], ids=["fp32", "bf16"])
def test_native_block_vs_fp64_autograd(tdt, name):
    """Lq = 45, B = 2, eval mode: the block's output and d/d tgt, in_proj_*, out_proj.*, norm2.* of a seeded functional
    (_functional) against fp64 autograd of tests/mha_ref.block (one run per dtype, one case per tensor).
      fp32: each gradient within 1e-4 of the tensor's largest gradient (the bar of tests/test_selfattn_gpu.py's
            test_gradients_of_the_attended_block_vs_fp64_autograd), the output within TOL["hs"].
      bf16: each within 2 x the error of the same block with mha_train_ref.flash_backward_bf16_model as its attention (q, k, v
            rounded to bf16 on the way in)."""
    out_err, out_bound, grads = _block_case(tdt)
    err, bound, top = (out_err, out_bound, None) if name == "out" else grads[name]
    print("native block %s %-26s max|err| %.3e  allowed %.3e%s"
          % (tdt, name, err, bound, "" if top is None else "  (%.2e of the largest gradient %.3g)" % (err / top, top)))
    assert err <= bound


def test_default_backend_is_todays_block_bit_for_bit():
    """"torch": the layer's own self_attn module, as before the switch existed"""
    c, layer = _layer("torch")
    gen = torch.Generator().manual_seed(46)
    tgt, pos = (torch.randn(2, 45, 256, generator=gen).to(DEV) for _ in range(2))
    with torch.no_grad():
        got = layer._attend_queries_autograd(tgt, pos)
        qk = (tgt + pos).transpose(0, 1)
        want = layer.norm2(tgt + layer.dropout2(layer.self_attn(qk, qk, tgt.transpose(0, 1), need_weights=False)[0].transpose(0, 1)))
    assert layer.self_attention_training == "torch" and torch.equal(got, want)


def _layer_run(layer, c):
    layer.zero_grad(set_to_none=True)
    tgt = c.tgt.clone().requires_grad_(True)
    out = layer(*_layer_args(c, tgt, c.reference_points), threshold=THR)
    out[0].square().sum().backward()
    grads = {n: p.grad.detach().clone() for n, p in layer.named_parameters() if p.grad is not None}
    grads["tgt"] = tgt.grad.detach().clone()
    layer.zero_grad(set_to_none=True)
    return [o.detach().clone() for o in out], grads


def test_layer_under_autograd_native_vs_torch():
    """eval mode, fp32: the two backends give the same layer -- outputs within TOL["hs"], the same validity mask, every parameter
    gradient within 1e-4 of its largest entry"""
    c, layer = _layer("torch")
    try:
        want, gwant = _layer_run(layer, c)
        layer.set_self_attention_training("native")
        got, ggot = _layer_run(layer, c)
        assert float((got[0] - want[0]).abs().max()) < TOL["hs"]
        assert torch.equal(got[4][..., 1] > THR, want[4][..., 1] > THR)
        assert sorted(ggot) == sorted(gwant) and "self_attn.in_proj_weight" in ggot
        worst = 0.0
        for n in gwant:
            top = float(gwant[n].abs().max())
            rel = float((ggot[n] - gwant[n]).abs().max()) / top if top > 0 else float(ggot[n].abs().max())
            worst = max(worst, rel)
            assert rel < 1e-4, (n, rel)
        print("layer gradients, native vs torch: worst %.2e of a tensor's largest entry" % worst)
    finally:
        _reset(layer)


@pytest.mark.parametrize("tdt", [F32, BF16], ids=["fp32", "bf16"])
def test_train_mode_with_attention_dropout(tdt):
    """reseeding repeats the bits, not reseeding changes them; finite results; self_attn receives a gradient"""
    c, layer = _layer("native", tdt)
    try:
        layer.train()
        assert layer.self_attn.dropout == 0.1
        torch.manual_seed(5)
        a, ga = _layer_run(layer, c)
        b, gb = _layer_run(layer, c)
        torch.manual_seed(5)
        a2, ga2 = _layer_run(layer, c)
        assert all(torch.equal(x, y) for x, y in zip(a, a2)) and all(torch.equal(ga[n], ga2[n]) for n in ga)
        assert not torch.equal(a[0], b[0]) and not torch.equal(ga["self_attn.in_proj_weight"], gb["self_attn.in_proj_weight"])
        assert all(bool(torch.isfinite(x).all()) for x in a) and all(bool(torch.isfinite(g).all()) for g in ga.values())
        for n in NAMES[:4]:
            assert float(ga[n].abs().max()) > 0, n
    finally:
        _reset(layer)


class Rig(G.Rig):
    """tests/test_train_graph_gpu.py's rig on a decoder with init_self_attention and the native backend, built through
    factory.build_graphed_train_step; dropout2 / 3 / 4 are off, attn_dropout is the attention's own"""

    def __init__(self, tdt, attn_dropout=0.0):
        from mvgformer_amd.caller import DecoderHead
        from mvgformer_amd.factory import build_criterion_from_cfg, build_graphed_train_step, build_optimizer_from_cfg
        case, self.g = G._data()
        self.dec = build_decoder(case, DEV, F32)
        self.dec.set_training_dtype(tdt).set_self_attention_training("native")
        cfg = NS(DECODER=NS(match_method="KNN", match_method_value=5, decay_method="none", optimizer="adam", lr_linear_proj_mult=0.1),
                 NETWORK=NS(IMAGE_SIZE=list(case.img_size)), TRAIN=NS(LR=0.0004, clip_max_norm=0.1),
                 MULTI_PERSON=NS(SPACE_SIZE=list(case.space_size), SPACE_CENTER=list(case.space_center)))
        criterion, self.weight_dict, decay = build_criterion_from_cfg(cfg)
        torch.manual_seed(0)
        self.head = DecoderHead(self.dec, case.NQ, 15, 256, case.space_size, case.space_center).to(DEV).set_criterion(criterion, decay)
        self.head.train()
        for layer in self.dec.layers:
            layer.dropout2.p = layer.dropout3.p = layer.dropout4.p = 0.0
            layer.self_attn.dropout = attn_dropout
        for p in self.head.parameters():
            p.requires_grad_(True)
        self.opt = build_optimizer_from_cfg(self.head, cfg)
        self.runner = build_graphed_train_step(self.head, self.opt, self.g, self.weight_dict, threshold=0.1, capture=False)
        self.ops16 = self.runner.operands
        self.start = {n: p.detach().clone() for n, p in self.head.named_parameters()}


@pytest.mark.parametrize("tdt", [F32, BF16], ids=["fp32", "bf16"])
def test_graphed_step_without_dropout_equals_eager_steps_bit_for_bit(tdt):
    """the assertion of tests/test_train_graph_gpu.py::test_three_replays_equal_three_eager_steps_bit_for_bit"""
    e1 = G._run(Rig(tdt), 3, replay=False)
    rig = Rig(tdt).captured()
    grads = rig.runner._grads()
    got = G._run(rig, 3, replay=True)
    G._assert_same(got, e1, "replay vs eager")
    assert rig.runner._grads() == grads                                  # no re-capture, no gradient moved
    losses = [float(m[0]) for m in got[0]]
    assert len(set(losses)) == 3 and all(torch.isfinite(m[0]) and float(m[1]) > 0 for m in got[0])
    for layer in rig.dec.layers:
        assert layer.self_attention_training == "native" and layer.init_self_attention
        moved = (layer.self_attn.in_proj_weight.detach() - rig.start["decoder.layers.%d.self_attn.in_proj_weight"
                                                                     % list(rig.dec.layers).index(layer)]).abs().max()
        assert float(moved) > 0                                          # the block's weights are trained by the replays


@pytest.mark.parametrize("tdt", [F32, BF16], ids=["fp32", "bf16"])
def test_graphed_step_draws_a_new_mask_per_replay(tdt):
    """attention dropout 0.1 and no other dropout: three replays are finite, and two replays from the same parameters give
    different losses -- a seed baked into the graph would repeat the mask and with it the loss"""
    rig = Rig(tdt, attn_dropout=0.1).captured()
    marks, _ = G._run(rig, 3, replay=True)
    assert all(bool(torch.isfinite(m[0])) and bool(torch.isfinite(m[1])) for m in marks)
    rig.restore()
    first = rig.runner.replay()[0].detach().clone()
    rig.restore()
    second = rig.runner.replay()[0].detach().clone()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(first)) and bool(torch.isfinite(second)) and not torch.equal(first, second)
