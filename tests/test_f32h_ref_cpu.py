"""The fp64 statements and bounds of the fp32 kernels on two-part fp16 operands (tests/chain_ref.py: pyramid_f32h, chain_a_f32h,
chain_b_f32h) without a GPU: pinned to the oracle, checked to cover a CPU emulation of the kernels' arithmetic
(tests/f32h_cases.py) and NOT to cover a one-part (11-bit) emulation; the host-side weight split of ops.split_swizzle_weight_h2;
and the ambiguity condition of the chain B cases tests/test_f32h_fp64.py runs on the device."""
import math

import pytest
import torch

from tests import chain_ref as R
from tests import f32h_cases as F
from tests.test_chain_ref_oracle import ORACLE_CASES, check_statements_against_oracle_layer


@pytest.mark.parametrize("cname", ORACLE_CASES)
def test_f32h_statements_match_the_oracle_layer(cname):
    check_statements_against_oracle_layer(cname, lambda *a: R.chain_a_f32h(*a, bounds=False),
                                          lambda *a: R.chain_b_f32h(*a, bounds=False))


def _ratio(name, got, ref, bound):
    err = (got.double() - ref).abs()
    r = float((err / bound.clamp_min(1e-300)).max())
    print("%s: max err %.2e, max err / bound %.3f" % (name, float(err.max()), r))
    return r


def test_split_h2_and_row_scale_follow_the_fp16_format():
    x = torch.tensor([0.0, 1e-45, 1.0, 1.5, 2.0, torch.nextafter(torch.tensor(2.0), torch.tensor(0.0)).item(), 3e38, 1e-38])
    s = R.row_scale(x)
    assert s.tolist() == [100, 100, 13, 13, 12, 13, -114, 100]
    for v, sv in zip(x[2:7], s[2:7]):
        assert 2.0 ** 13 <= float(v) * 2.0 ** int(sv) < 2.0 ** 14
    # the operand term of one entry: |x 2^s - h - l| <= max(H2_PART |x 2^s|, 2^-25), entries down to 2^-40 of the maximum
    xs = torch.randn(4096, generator=torch.Generator().manual_seed(0)).double() * 2.0 ** torch.linspace(13, -27, 4096).double()
    h, l = R.split_h2(xs.float(), 0)
    d = (xs.float().double() - h.double() - l.double()).abs()
    assert bool((d <= torch.maximum(R.H2_PART * xs.abs(), torch.tensor(2.0 ** -25, dtype=torch.float64))).all())
    assert bool((l.double().abs() <= 2.0 ** -11 * xs.abs() + 2.0 ** -25).all())                  # H2_LL: |l_a l_w| <= 2^-22 |a w|


# ------------------------------------------------------------------------------------------------ bounds against emulations
def _operand_term(x, W):
    """error of the three products alone, fp64 accumulation, relative to sum |a| |w| (the figure the kernel's comment quotes)."""
    sx, sw = R.row_scale(x.abs().amax(-1, keepdim=True)), R.weight_scale(W)
    (xh, xl), (wh, wl) = (tuple(t.double() for t in R.split_h2(x, sx))), (tuple(t.double() for t in R.split_h2(W, sw)))
    acc = torch.ldexp(xl @ wh.t() + xh @ wl.t() + xh @ wh.t(), -(sx + sw).double())
    return float(((acc - R.lin(x, W)).abs() / R.lin_abs(x, W).clamp_min(1e-300)).max())


def test_operand_term_is_plausible():
    """the operand error alone (fp64 accumulation) on K = 256, weights randn / 16: 4e-8 of sum |a| |w| on well-scaled rows, below
    H2_LL + 2 H2_PART = 4.8e-7 (one term's worst case) everywhere."""
    W = torch.randn(256, 256, generator=torch.Generator().manual_seed(1)) / 16
    for kind in ("randn", "rows_12_decades", "entries_6_decades"):
        r = _operand_term(F.operand_rows(kind, 256, 2), W)
        print("operand term [%s]: %.2e of sum|a||w|" % (kind, r))
        assert r < R.H2_LL + 2 * R.H2_PART
        assert kind == "entries_6_decades" or r < 1e-7


def _pyr_weights():
    gen = torch.Generator().manual_seed(21)
    return (torch.randn(256, 256, generator=gen) / 16, torch.randn(256, generator=gen), torch.randn(192, 256, generator=gen) / 16)


def _a_case(kind):
    W = F.chain_a_weights()
    samp = F.operand_rows(kind, 96, 5)
    inside = (torch.rand(96, generator=torch.Generator().manual_seed(6)) < 0.7).to(torch.uint8)
    return W, samp, inside


@pytest.mark.parametrize("kind", F.OPERAND_KINDS)
def test_bounds_cover_an_emulation_pyramid_and_chain_a(kind):
    """two-part emulation inside the bounds for every output; one-part emulation (l = 0) outside them on every output tensor."""
    Wv, bv, Wg = _pyr_weights()
    feat = F.operand_rows(kind, 96, 3)
    ref = R.pyramid_f32h(feat, Wv, bv, Wg)
    for parts in (2, 1):
        rv = _ratio("pyramid value [%s] parts %d" % (kind, parts), F.emu_lin(feat, Wv, bv, parts), ref["value"], ref["value_err"])
        rg = _ratio("pyramid G [%s] parts %d" % (kind, parts), F.emu_lin(feat, Wg, None, parts), ref["G"], ref["G_err"])
        assert (rv <= 1 and rg <= 1) if parts == 2 else (rv > 1 and rg > 1)
    W, samp, inside = _a_case(kind)
    wl = [W[k] for k in F.A_KEYS]
    ref = R.chain_a_f32h(samp, inside, *wl)
    for parts in (2, 1):
        attn, o = F.emu_chain_a(samp, inside, *wl, parts=parts)
        ra = _ratio("chain A attn [%s] parts %d" % (kind, parts), attn, ref["attn"], ref["attn_err"])
        ro = _ratio("chain A o [%s] parts %d" % (kind, parts), o, ref["o"], ref["o_err"])
        assert (ra <= 1 and ro <= 1) if parts == 2 else (ra > 1 and ro > 1)
        assert bool((attn[inside == 0] == 0).all())


@pytest.mark.parametrize("wmul", [(2.0 ** -30, 1.0, 1.0), (1.0, 2.0 ** 20, 2.0 ** -30), (2.0 ** 20, 2.0 ** -30, 1.0)])
def test_bounds_cover_an_emulation_weight_scales(wmul):
    """weights near 2^-30 and 2^20: the tensor scale takes both signs."""
    W = F.chain_a_weights(wmul=wmul)
    sc = [R.weight_scale(W[k]) for k in ("Wp", "W0", "W1")]
    assert min(sc) < 0 < max(sc) or max(wmul) == 1.0, sc
    samp, inside = F.operand_rows("randn", 64, 8), torch.ones(64, dtype=torch.uint8)
    wl = [W[k] for k in F.A_KEYS]
    ref = R.chain_a_f32h(samp, inside, *wl)
    attn, o = F.emu_chain_a(samp, inside, *wl)
    assert bool(torch.isfinite(o).all())
    assert _ratio("chain A attn wmul %s" % (wmul,), attn, ref["attn"], ref["attn_err"]) <= 1
    assert _ratio("chain A o wmul %s" % (wmul,), o, ref["o"], ref["o_err"]) <= 1


@pytest.mark.parametrize("has_ffn", [True, False])
@pytest.mark.parametrize("edges", [None, "ln", "operands"])
def test_bounds_cover_an_emulation_chain_b(has_ffn, edges):
    W = F.chain_b_weights()
    c = F.chain_b_inputs(1, 6, 15, 3, seed=4, nxt=("q", 192), ln_edges=edges == "ln", edges=edges)
    ref = F.chain_b_ref(c, W, has_ffn)
    kw = dict(has_ffn=has_ffn, qpos=c["qpos"], Wn=W["Wn"][:192], bn=W["bn"][:192])
    for parts in (2, 1):
        emu = F.emu_chain_b(c["attn"], c["tgt"], *[W[k] for k in F.B_KEYS], c["J"], parts=parts, **kw)
        rs = [_ratio("chain B %s ffn %d edges %s parts %d" % (k, has_ffn, edges, parts), emu[k], ref[k], ref[k + "_err"])
              for k in ("tgt", "prob", "xw")]
        assert all(r <= 1 for r in rs) if parts == 2 else all(r > 1 for r in rs)


# ---------------------------------------------------------------------------------------------- ops.split_swizzle_weight_h2
def _unswizzle(planes, Np, K):
    """the inverse of ops.swizzle_weight for both planes: (2, Np, K)."""
    t = planes.view(2, Np // 256, 4, K // 16, 2, 2, 32, 8)            # plane, nb, wn, ks, j, h, rl, e
    return t.permute(0, 1, 2, 4, 6, 3, 5, 7).reshape(2, Np, K)


@pytest.mark.parametrize("case", ["randn", "max_pow2", "max_under_pow2", "tiny", "huge", "zero", "inf", "nan", "n192"])
def test_split_swizzle_weight_h2(case):
    from mvgformer_amd import ops
    gen = torch.Generator().manual_seed(17)
    N, K = (192 if case == "n192" else 256), 256
    w = torch.randn(N, K, generator=gen) / 16
    two = torch.tensor(2.0)
    if case in ("max_pow2", "max_under_pow2"):
        w = w.clamp(-0.2, 0.2)
        w[7, 9] = -0.25 if case == "max_pow2" else float(torch.nextafter(two, torch.tensor(0.0)) / 8)
    w = {"tiny": w * 2.0 ** -30, "huge": w * 2.0 ** 20, "zero": w * 0}.get(case, w)
    if case in ("inf", "nan"):
        w[3, 4] = float(case)
    planes, s = ops.split_swizzle_weight_h2(w)
    assert planes.dtype == torch.float16 and planes.numel() == 2 * 256 * K
    assert s == R.weight_scale(w)
    hl = _unswizzle(planes, 256, K)
    wp = torch.cat([w, w.new_zeros(256 - N, K)], 0)
    h, l = R.split_h2(wp, s)
    assert torch.equal(hl[0].view(torch.int16), h.view(torch.int16)) and torch.equal(hl[1].view(torch.int16), l.view(torch.int16))
    if N < 256:
        assert bool((hl[:, N:] == 0).all())
    if case in ("zero", "inf", "nan"):
        assert s == 0
        return
    mx = float(w.abs().max()) * 2.0 ** s
    assert 2.0 ** 13 <= mx < 2.0 ** 14 and float(hl[0].float().abs().max()) <= 2.0 ** 14 < 65504
    assert (s > 0) == (case != "huge")
    back = torch.ldexp(hl[0].double() + hl[1].double(), torch.tensor(-s))
    d = (back - wp.double()).abs()
    assert bool((d <= torch.maximum(R.H2_PART * wp.double().abs(), torch.tensor(2.0 ** -25 * 2.0 ** -s, dtype=torch.float64))).all())
    assert math.isfinite(float(back.abs().max()))


# ------------------------------------------------------------------------------------------------ the device cases, on the CPU
@pytest.mark.parametrize("k,case", list(enumerate(F.B_CASES)), ids=["B%d_NQ%d_J%d_V%d" % c for c in F.B_CASES])
def test_chain_b_cases_have_no_person_near_the_threshold(k, case):
    """every `valid` comparison of tests/test_f32h_fp64.py covers all persons: the reference alone decides that no fp64 prob_1 lies
    within its bound of the case's threshold."""
    opt = F.b_options(k)
    c = F.chain_b_inputs(*case, seed=100 + k, nxt=opt["nxt"], forced=opt["forced"])
    ref = F.chain_b_ref(c, F.chain_b_weights(), opt["has_ffn"])
    assert not bool(ref["ambiguous"].any())
    if c["forced"] is None and ref["valid"].numel() > 1:
        assert bool(ref["valid"].any()) and not bool(ref["valid"].all())


@pytest.mark.parametrize("name", F.B_EDGE_NAMES)
def test_chain_b_edge_cases_have_no_person_near_the_threshold(name):
    c, variant, has_ffn = F.b_edge_cases(256)[name]                   # 256 CUs: the MI355X
    ref = F.chain_b_ref(c, F.chain_b_weights(variant=variant), has_ffn)
    assert not bool(ref["ambiguous"].any()) and bool(ref["valid"].any()) and not bool(ref["valid"].all())
    assert all(bool(torch.isfinite(ref[k]).all()) for k in ("tgt", "prob", "xw", "tgt_err", "prob_err", "xw_err"))
