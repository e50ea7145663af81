"""Pin the fp64 chain statements of tests/chain_ref.py (rounding off) to the oracle (oracle/decoder_ref.py), which
tests/test_oracle_golden.py pins to the reference's fixtures.  CPU only: the GPU tests of the bf16 chains
(tests/test_chains_fp64.py) then rest on the oracle, not on another kernel."""
import pytest
import torch

from mvgformer_amd.synthetic import build_case, to_torch_state
from oracle import decoder_ref as O
from tests import chain_ref as R
from tests.golden.cases import LAYER_CASES


ORACLE_CASES = ["mini5_half", "mini5_b2"]


def check_statements_against_oracle_layer(cname, chain_a, chain_b):
    """one oracle layer against the chain statements `chain_a` / `chain_b` (signatures of chain_ref.chain_a / chain_b, rounding
    off); tests/test_f32h_ref_cpu.py sends the f32h statements down the same route."""
    spec = LAYER_CASES[cname]
    case = build_case(spec["config"], B=spec.get("B", 1), seed=spec["seed"], NQ=spec.get("NQ"), layers=spec.get("layers"),
                      valid_fraction=spec.get("valid_fraction"))
    prm = to_torch_state(case.weights)
    P = lambda n: prm["layers.0." + n].double()
    dt = torch.float64
    thr = 0.1
    (hs, _, _, _, prob), ex = O.decoder_layer_forward(prm, "layers.0.", case.tgt, case.query_pos, case.reference_points,
                                                      case.src_views, case.spatial_shapes, case.level_start_index, case.meta,
                                                      case.img_size, threshold=thr, dtype=dt, extras=True)
    B, Lq, C = case.tgt.shape
    J, V = 15, case.V
    rows = B * Lq
    attn = torch.stack(ex["attn_views"], 0).reshape(V, rows, C)
    # chain B: view mean, update Linear, LN2, FFN, LN3, class head (fp64 throughout on both sides)
    ffn = [P(n) for n in ("feature_update_mlp.weight", "feature_update_mlp.bias", "norm2.weight", "norm2.bias", "linear1.weight",
                          "linear1.bias", "linear2.weight", "linear2.bias", "norm3.weight", "norm3.bias",
                          "class_embed.weight", "class_embed.bias")]
    b = chain_b(attn, case.tgt.reshape(rows, C).double(), *ffn, thr, J)
    assert float((b["tgt"] - hs.reshape(rows, C)).abs().max()) < 1e-12
    assert float((b["prob"] - prob.reshape(-1, 2)).abs().max()) < 1e-14
    assert torch.equal(b["valid"], (prob[..., 1] > thr).reshape(-1))
    # chain A: output projection x in-image flag against the oracle's attn rows, pose MLP against its dense 2-D points and
    # view confidences
    WH = case.spatial_shapes.flip(-1).double()
    img = torch.tensor(case.img_size, dtype=dt)
    pose = [P("pose_embed.MLP.layers.%d.%s" % (i, w)) for i in range(3) for w in ("weight", "bias")]
    pa = {k: v.double() for k, v in prm.items() if k.startswith("layers.0.proj_attn.")}
    logits = []
    for v in range(V):
        r, inside = O.project_ref_points(case.reference_points, case.meta[v]["camera"], case.meta[v]["center"],
                                         case.meta[v]["scale"], case.img_size, dt)
        src_v = [s[v * B:(v + 1) * B].double() for s in case.src_views]
        _, it = O.proj_attn_forward(pa, "layers.0.proj_attn.", case.tgt.double() + case.query_pos.double(), r.unsqueeze(2) * WH / (WH - 1),
                                    src_v, case.spatial_shapes, case.level_start_index, return_intermediates=True)
        a = chain_a(it["sampled"].reshape(rows, C), inside.reshape(rows), P("proj_attn.output_proj.weight"),
                    P("proj_attn.output_proj.bias"), *pose)
        assert float((a["attn"] - attn[v]).abs().max()) < 1e-12
        assert int((inside.reshape(rows) == 0).sum()) > 0 and bool((a["attn"][inside.reshape(rows) == 0] == 0).all())
        ref2d = (r.reshape(rows, 2) + a["o"][:, :2] / img) * img
        assert float((ref2d - ex["ref2d_dense"][:, v].reshape(rows, 2)).abs().max()) < 1e-9        # px
        logits.append(a["o"][:, 2])
    conf = torch.softmax(torch.stack(logits, 0), 0)
    assert float((conf - ex["conf"].transpose(0, 1).reshape(V, rows)).abs().max()) < 1e-14


@pytest.mark.parametrize("cname", ORACLE_CASES)
def test_chain_statements_match_the_oracle_layer(cname):
    check_statements_against_oracle_layer(cname, R.chain_a, R.chain_b)


def test_bf16_bounds_cover_an_fp32_emulation_of_the_kernels():
    """the bounds of the rounded statements cover a plain fp32 computation with the same bf16 rounding points (torch on the CPU,
    another summation order than the kernels'), and the rounded statements differ from the unrounded ones: a bound that did
    not cover this stand-in could not hold a kernel to anything."""
    gen = torch.Generator().manual_seed(4)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    bf = R.bf
    mk = lambda n, k: (bf(rnd(n, k) / k ** 0.5).float(), (rnd(n) * 0.1).float())
    f32 = lambda x, W, b: x.float() @ W.t() + b
    rows, J, V = 60, 15, 3
    (Wp, bp), (W0, b0), (W1, b1), (W2, b2) = mk(256, 256), mk(256, 256), mk(256, 256), mk(3, 256)
    samp, inside = bf(rnd(rows, 256)).float(), (torch.rand(rows, generator=gen) < 0.7).to(torch.uint8)
    a = bf(f32(samp, Wp, bp) * inside[:, None].float())
    o = f32(bf(torch.relu(f32(bf(torch.relu(f32(a, W0, b0))), W1, b1))), W2, b2)
    rd = R.chain_a(samp, inside, Wp, bp, W0, b0, W1, b1, W2, b2, bf16=True, attn=a)
    ex = R.chain_a(samp, inside, Wp, bp, W0, b0, W1, b1, W2, b2)
    assert bool(((a.double() - bf(rd["attn_exact"])).abs() <= R.round_err(rd["attn_exact"], rd["attn_err"], rms=False)).all())
    assert bool(((o.double() - rd["o"]).abs() <= rd["o_err"]).all()) and float((rd["o"] - ex["o"]).abs().max()) > 0
    (Wu, bu), (Wf1, bf1), (Wf2, bf2), (Wc, bc), (Wn, bn) = mk(256, 256), mk(1024, 256), mk(256, 1024), mk(2, 256), mk(256, 256)
    g2, be2, g3, be3 = ((1 + 0.1 * rnd(256)).float() for _ in range(4))
    attn, tgt, qpos = bf(rnd(V, rows, 256)).float(), rnd(rows, 256).float(), rnd(rows, 256).float()
    tgt[:4] = 1e3 + tgt[:4]                                           # LayerNorm inputs with a large common offset
    tgt[4:8] = 0.25 - bu + 1e-3 * tgt[4:8]                            # ... and nearly constant ones (variance ~ 1e-6 < eps)
    attn[:, 4:8] = 0
    ln32 = lambda x, g, b: torch.nn.functional.layer_norm(x, (256,), g, b, 1e-5)
    for has_ffn in (True, False):
        t1 = ln32(tgt + f32(bf(attn.sum(0) * (1.0 / V)), Wu, bu), g2, be2)
        t = ln32(t1 + f32(bf(torch.relu(f32(bf(t1), Wf1, bf1))), Wf2, bf2), g3, be3) if has_ffn else t1
        prob = torch.sigmoid(f32(t, Wc, bc)).view(-1, J, 2).mean(1)
        xw = f32(bf(t + qpos), Wn, bn)[:, :192]
        args = (attn, tgt, Wu, bu, g2, be2, Wf1, bf1, Wf2, bf2, g3, be3, Wc, bc, 0.5, J)
        kw = dict(has_ffn=has_ffn, qpos=qpos, Wn=Wn, bn=bn, n_next=192)
        rd, ex = R.chain_b(*args, bf16=True, **kw), R.chain_b(*args, **kw)
        for key, got in (("tgt", t), ("prob", prob), ("xw", xw)):
            d = (got.double() - rd[key]).abs()
            print("fp32 emulation, has_ffn %d, %s: max err / bound %.3f  err %.2e  bound median %.2e max %.2e" % (has_ffn, key, float((d / rd[key + "_err"]).max()), float(d.max()), float(rd[key + "_err"].median()), float(rd[key + "_err"].max())))
            assert bool((d <= rd[key + "_err"]).all()), key
            assert float((rd[key] - ex[key]).abs().max()) > 0, key
