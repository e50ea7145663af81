"""The decoder with init_self_attention on the GPU: the attended block against fp64, exact composition (the layer with the
switch = the same weights without it, fed the attended tgt the new ops produce; the decoder = the manual loop over its layers; a
HIP-graph replay = the eager forward), parity with the fixture the REFERENCE produced with the switch on
(tests/golden/mini5_selfattn.npz) at the tolerances tests/test_hip_parity.py uses for the mini cases, the block's gradients
against fp64 autograd, and the refusal of the query-sharded runners."""
import os

import numpy as np
import pytest
import torch

from mvgformer_amd.synthetic import to_torch_state
from tests import mha_ref as R
from tests.selfattn_cases import FIXTURE, SPEC, build_decoder, selfattn_case
from tests.test_hip_parity import TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
THR = SPEC["threshold"]
_HELD = {}


def _setup(dtype, flag=True):
    """(case on the device, decoder) built once per (dtype, switch)"""
    from mvgformer_amd.factory import case_to_device
    if "case" not in _HELD:
        _HELD["case"] = case_to_device(selfattn_case(), DEV)
        _HELD["prm"] = to_torch_state(selfattn_case(with_features=False).weights)
    if (dtype, flag) not in _HELD:
        _HELD[(dtype, flag)] = build_decoder(_HELD["case"], DEV, dtype, flag)
    return _HELD["case"], _HELD[(dtype, flag)]


def _layer_args(c, tgt, ref):
    return (tgt, c.query_pos, ref[:, :, None] if ref.dim() == 3 else ref, c.src_views, c.spatial_shapes, c.level_start_index, c.meta)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_attended_block_vs_fp64(dtype):
    """DQDecoderLayer.attend_queries (GEMMs + mvg_self_attention + add_layernorm) against tests/mha_ref.block in fp64; the bf16
    bound is the model's: the same block with the bf16 attention's rounding points and bf16-rounded projection operands"""
    c, dec = _setup(dtype)
    prm, p = _HELD["prm"], "layers.0.self_attn."
    with torch.no_grad():
        got = dec.layers[0].attend_queries(c.tgt, c.query_pos).cpu().double()
    args = (c.tgt.cpu(), c.query_pos.cpu(), prm[p + "in_proj_weight"], prm[p + "in_proj_bias"], prm[p + "out_proj.weight"],
            prm[p + "out_proj.bias"], prm["layers.0.norm2.weight"], prm["layers.0.norm2.bias"])
    want = R.block(*args)
    err = float((got - want).abs().max())
    print("attend_queries %s: max |err| vs fp64 %.3e" % (dtype, err))
    assert got.shape == want.shape and float((want - c.tgt.cpu().double()).abs().max()) > 0.1
    assert err < (TOL["hs"] if dtype == torch.float32 else 6e-2)          # the layer bars of tests/test_hip_parity.py


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_layer_with_the_switch_is_the_plain_layer_on_the_attended_query(dtype):
    """bit for bit: flag on == flag off with query_tgt = attend_queries(tgt, query_pos) (the attended tgt stands in for tgt in the
    projective attention's query; the residual of the feature update stays the layer's own tgt, as in the reference)"""
    from mvgformer_amd.decoder import DecoderContext
    c, on = _setup(dtype, True)
    _, off = _setup(dtype, False)
    with torch.no_grad():
        got = on.layers[0](*_layer_args(c, c.tgt, c.reference_points), threshold=THR)
        plain = off.layers[0](*_layer_args(c, c.tgt, c.reference_points), threshold=THR)
        lay = off.layers[0]
        ctx = DecoderContext.build(c.src_views, c.spatial_shapes, c.level_start_index, c.meta, lay.img_size, dtype, c.tgt.shape[0])
        att = lay.attend_queries(c.tgt, c.query_pos)
        st = lay.forward_features(c.tgt, c.query_pos, c.reference_points[:, :, None], ctx, THR, query_tgt=att)
        want = lay.forward_triangulate(st, ctx)
    torch.cuda.synchronize()
    assert _same(got, want)
    assert not torch.equal(got[0], plain[0]) and float((att - c.tgt).abs().max()) > 0.1      # the switch does something


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_decoder_is_the_manual_loop_over_its_layers(dtype):
    """a 2-layer DQDecoder (side stream, hand-offs between the layers) == its layers called one by one, bit for bit: a query term
    handed over by layer 0's chain B (computed from tgt' + query_pos) would be stale for a layer that attends first"""
    c, dec = _setup(dtype)
    with torch.no_grad():
        hs, refs, r2d, p2d, cls = dec(c.tgt, c.reference_points, c.src_views, c.meta, c.spatial_shapes, c.level_start_index, None,
                                      query_pos=c.query_pos, threshold=THR)
        tgt, ref = c.tgt, c.reference_points
        for l, layer in enumerate(dec.layers):
            out = layer(*_layer_args(c, tgt, ref), threshold=THR)
            assert _same(out, (hs[l], refs[l], r2d[l], p2d[l], cls[l])), (l, str(dtype))
            tgt, ref = out[0], out[1]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_graphed_decoder_replays_the_eager_forward(dtype):
    from mvgformer_amd.serving import GraphedDecoder
    c, dec = _setup(dtype)
    run = GraphedDecoder(dec, c.meta, c.spatial_shapes, c.level_start_index, batch=c.tgt.shape[0], num_queries=SPEC["NQ"], threshold=THR)
    run.load(src_views=c.src_views, tgt=c.tgt, query_pos=c.query_pos, reference_points=c.reference_points)
    got = run.replay()
    got = [t.clone() for t in got[:4]] + [[p.clone() for p in got[4]]]
    with torch.no_grad():
        want = dec(c.tgt, c.reference_points, c.src_views, c.meta, c.spatial_shapes, c.level_start_index, None,
                   query_pos=c.query_pos, threshold=THR)
    torch.cuda.synchronize()
    assert _same(got[:4], want[:4]) and _same(got[4], want[4])
    again = run.replay()
    assert _same(again[:4], want[:4])


def test_fp32_layers_and_decoder_vs_the_reference_fixture():
    """teacher-forced layers at the fp32 mini-case tolerances of tests/test_hip_parity.py, then the free-running decoder at that
    file's free-running bounds"""
    g = np.load(os.path.join(GOLD, FIXTURE))
    c, dec = _setup(torch.float32)
    tgt, ref = c.tgt, c.reference_points
    for l in range(len(dec.layers)):
        with torch.no_grad():
            out = dec.layers[l](*_layer_args(c, tgt, ref), threshold=THR)
        hs, new_ref, r2d, p2d, cls = (t.cpu() for t in out)
        e = dict(cls=float((cls - torch.from_numpy(g["cls"][l])).abs().max()), hs=float((hs - torch.from_numpy(g["hs"][l])).abs().max()),
                 p2d=float((p2d - torch.from_numpy(g["projs2d"][l])).abs().max()), r2d=float((r2d - torch.from_numpy(g["refs2d"][l])).abs().max()),
                 mm=float((new_ref - torch.from_numpy(g["refs"][l])).norm(dim=-1).max()))
        print("layer %d vs reference:" % l, e)
        assert np.array_equal((cls[..., 1] > THR).numpy(), g["cls"][l][..., 1] > THR)
        assert e["cls"] < TOL["cls"] and e["hs"] < TOL["hs"] and e["p2d"] < TOL["px"] and e["r2d"] < TOL["px"] and e["mm"] < TOL["mm"]
        assert torch.equal(new_ref == 0, torch.from_numpy(g["refs"][l]) == 0)
        tgt, ref = torch.from_numpy(g["hs"][l]).to(DEV), torch.from_numpy(g["refs"][l]).to(DEV)
    with torch.no_grad():
        hs, refs, r2d, p2d, cls = dec(c.tgt, c.reference_points, c.src_views, c.meta, c.spatial_shapes, c.level_start_index, None,
                                      query_pos=c.query_pos, threshold=THR)
    cls = torch.stack(cls).cpu()
    assert np.array_equal((cls[..., 1] > THR).numpy(), g["cls"][..., 1] > THR)
    assert float((hs.cpu() - torch.from_numpy(g["hs"])).abs().max()) < 2e-2
    assert float((r2d.cpu() - torch.from_numpy(g["refs2d"])).abs().max()) < 0.5
    assert float((refs.cpu() - torch.from_numpy(g["refs"])).norm(dim=-1).max()) < 3.0


def test_bf16_layer_vs_the_reference_fixture():
    """layer 0 in bf16 at the bars of test_decoder_bf16_vs_fp32_oracle for the queries whose validity agrees; the agreement of
    the validity mask is reported on its own (about half of the queries sit near the 0.1 threshold by construction)"""
    g = np.load(os.path.join(GOLD, FIXTURE))
    c, dec = _setup(torch.bfloat16)
    with torch.no_grad():
        hs, new_ref, r2d, p2d, cls = (t.cpu() for t in dec.layers[0](*_layer_args(c, c.tgt, c.reference_points), threshold=THR))
    mine, theirs = cls[..., 1] > THR, torch.from_numpy(g["cls"][0][..., 1] > THR)
    agree = mine == theirs
    print("bf16 layer 0: validity mask agrees for %d of %d queries; |cls| err %.2e" %
          (int(agree.sum()), agree.numel(), float((cls - torch.from_numpy(g["cls"][0])).abs().max())))
    assert float((cls - torch.from_numpy(g["cls"][0])).abs().max()) < 2e-2           # the bf16 class-probability bar of that file
    # ... so only a query whose reference probability lies within that bar of the threshold may change sides
    far = torch.from_numpy(np.abs(g["cls"][0][..., 1] - THR) > 2e-2)
    assert bool(agree[far].all())
    B, NQ, J = agree.shape[0], agree.shape[1], 15
    tok = agree.view(B, NQ, 1).expand(B, NQ, J).reshape(B, NQ * J)
    assert float((hs - torch.from_numpy(g["hs"][0])).abs().max()) < 6e-2
    assert float(((p2d - torch.from_numpy(g["projs2d"][0])).abs().amax(-1) * tok[:, None]).max()) < 2e-3
    assert float(((r2d - torch.from_numpy(g["refs2d"][0])).abs().amax(-1) * tok[:, None]).max()) < 0.5
    assert float(((new_ref - torch.from_numpy(g["refs"][0])).norm(dim=-1) * tok).max()) < 6.0


def test_gradients_of_the_attended_block_vs_fp64_autograd():
    """forward_autograd's block (the layer's own self_attn module, need_weights=False, fp32) at Lq = 45, B = 2: d/d tgt, in_proj_*,
    out_proj.*, norm2.* of a seeded linear functional against torch autograd of tests/mha_ref.block in fp64 on the CPU, each within
    1e-4 of the tensor's largest gradient (the fp64 bar of test_layer_gradients_vs_reference_autograd)"""
    c, dec = _setup(torch.float32)
    layer = dec.layers[0]
    gen = torch.Generator().manual_seed(45)
    tgt, pos, w = (torch.randn(2, 45, 256, generator=gen) for _ in range(3))
    names = ["self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
             "norm2.weight", "norm2.bias"]
    prm = dict(layer.named_parameters())
    p64 = [prm[n].detach().cpu().double().requires_grad_(True) for n in names]
    t64 = tgt.double().requires_grad_(True)
    (R.block(t64, pos, *p64) * w.double()).sum().backward()
    want = dict(zip(["tgt"] + names, [t64.grad] + [p.grad for p in p64]))
    layer.zero_grad(set_to_none=True)
    tg = tgt.to(DEV).requires_grad_(True)
    with torch.enable_grad():
        out = layer._attend_queries_autograd(tg, pos.to(DEV))
        (out * w.to(DEV)).sum().backward()
    assert float((out.detach().cpu().double() - R.block(tgt, pos, *[p.detach() for p in p64])).abs().max()) < TOL["hs"]
    got = dict(zip(["tgt"] + names, [tg.grad] + [prm[n].grad for n in names]))
    worst = 0.0
    for n in want:
        rel = float((got[n].detach().cpu().double() - want[n]).abs().max() / want[n].abs().max())
        worst = max(worst, rel)
        assert rel < 1e-4, (n, rel)
    print("attended block gradients vs fp64 autograd: worst %.2e of the tensor's largest gradient" % worst)
    layer.zero_grad(set_to_none=True)


def test_training_path_runs_the_block_and_matches_the_native_layer():
    """the layer under autograd (forward_autograd, eval mode: no dropout) gives the native layer's outputs to fp32 rounding and
    sends a gradient into the self_attn parameters"""
    c, dec = _setup(torch.float32)
    layer = dec.layers[0]
    with torch.no_grad():
        want = layer(*_layer_args(c, c.tgt, c.reference_points), threshold=THR)
    layer.zero_grad(set_to_none=True)
    tgt = c.tgt.clone().requires_grad_(True)
    out = layer(*_layer_args(c, tgt, c.reference_points), threshold=THR)
    assert float((out[0] - want[0]).abs().max()) < TOL["hs"] and torch.equal(out[4][..., 1] > THR, want[4][..., 1] > THR)
    out[0].square().sum().backward()
    g = layer.self_attn.in_proj_weight.grad
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    layer.zero_grad(set_to_none=True)


def test_query_sharded_runners_refuse_coupled_queries():
    """at entry, before any collective: no process group exists in this process"""
    from mvgformer_amd import dist as D
    c, dec = _setup(torch.float32)
    args = (dec, c.tgt, c.reference_points, c.src_views)
    with pytest.raises(NotImplementedError, match="couples the queries"):
        D.sharded_decoder_forward(dec, c.tgt, c.reference_points, c.src_views, c.meta, c.spatial_shapes, c.level_start_index,
                                  c.query_pos, THR)
    for runner in (D.GraphedShardedDecoder, D.SpeculativeShardedDecoder):
        with pytest.raises(NotImplementedError, match="couples the queries"):
            runner(*args, c.query_pos, None, THR, SPEC["NQ"])
    D.refuse_coupled_queries(_setup(torch.float32, False)[1])       # a plain decoder passes
