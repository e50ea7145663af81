"""The fp32 kernels on two-part fp16 operands (mvg_pyramid_f32h, mvg_chain_attn_pose_f32h, mvg_chain_update_ffn_class_f32h:
csrc/f32s.hip) through the C ABI against the plain fp64 operation (tests/chain_ref.py: pyramid_f32h, chain_a_f32h, chain_b_f32h,
pinned to the oracle by tests/test_f32h_ref_cpu.py), at the shapes where their code switches paths and at the edges of the
operand split.  The only pass condition is err <= bound elementwise, the bounds being the derived ones of chain_ref (fp32 unit
roundoff, K, the fp16 format, LAMBDA); each assertion prints max |err| / bound.  Every output is a slice of a larger buffer whose
guard must come back untouched, pre-filled with NaN so that an element the kernel does not write fails."""
import ctypes as C

import pytest
import torch

from tests import chain_ref as R
from tests import f32h_cases as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 1024
SENT_F, SENT_U8, FILL_U8 = -7.25e5, 0xA5, 0x5A
BADARG = 10001                  # MVG_E_BADARG


def _lib():
    from mvgformer_amd import _lib as L
    return L


def _cus():
    return _lib().device_info()[1]


def _guarded(n, dtype=torch.float32, front=0):
    """(buffer, view of n elements at offset `front`): guard = sentinel, payload = NaN (uint8: a value that is neither 0 nor 1)."""
    u8 = dtype == torch.uint8
    buf = torch.full((front + n + GUARD,), SENT_U8 if u8 else SENT_F, dtype=dtype, device=DEV)
    buf[front:front + n] = FILL_U8 if u8 else float("nan")
    return buf, buf[front:front + n]


def _guard_ok(buf, n, front=0):
    s = SENT_U8 if buf.dtype == torch.uint8 else SENT_F
    return bool((buf[:front] == s).all()) and bool((buf[front + n:] == s).all())


def _check(name, got, ref, bound):
    err = (got.double() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print("%s: max err %.2e, max err / bound %.3f" % (name, float(err.max()) if err.numel() else 0.0, ratio))
    assert bool((err <= bound).all()), (name, ratio)          # NaN (an element never written) fails too


_PLANES = {}


def _planes(w):
    """(planes, scale) of an fp32 weight on the device (ops.split_swizzle_weight_h2), cached by tensor."""
    from mvgformer_amd import ops
    key = (w.data_ptr(), tuple(w.shape))
    if key not in _PLANES:
        _PLANES[key] = (w,) + tuple(ops.split_swizzle_weight_h2(w))
    return _PLANES[key][1:]


def _dev(W):
    return {k: v.to(DEV).contiguous() for k, v in W.items()}


_WA, _WB = {}, {}


def _wa(wmul=(1.0, 1.0, 1.0), **over):
    key = (wmul, tuple(sorted(over.items())))
    if key not in _WA:
        W = F.chain_a_weights(wmul=wmul)
        for k, v in over.items():
            W[k] = torch.full_like(W[k], v)
        _WA[key] = _dev(W)
    return _WA[key]


def _wb(variant=None):
    if variant not in _WB:
        _WB[variant] = _dev(F.chain_b_weights(variant=variant))
    return _WB[variant]


# ------------------------------------------------------------------------------------------------------------------- chain A
def _run_a(samp, inside, W, order=None, o_masked=None, rows=None, samp_ptr=None, attn_off=0, scales=None, expect=0):
    L = _lib()
    rows = samp.shape[0] if rows is None else rows
    n = samp.shape[0]
    abuf, attn = _guarded(n * 256, front=GUARD)
    obuf, o = _guarded(n * 3)
    (Wp, sp), (W0, s0), (W1, s1) = _planes(W["Wp"]), _planes(W["W0"]), _planes(W["W1"])
    if scales is not None:
        sp, s0, s1 = scales
    rc = L.load().mvg_chain_attn_pose_f32h(
        L.ptr(samp) if samp_ptr is None else samp_ptr, L.ptr(inside), L.ptr(Wp), sp, L.ptr(W["bp"]), L.ptr(W0), s0, L.ptr(W["b0"]),
        L.ptr(W1), s1, L.ptr(W["b1"]), L.ptr(W["W2"]), L.ptr(W["b2"]), C.c_void_p(attn.data_ptr() + attn_off), L.ptr(o),
        L.ptr(order), L.ptr(o_masked), rows, L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, rc
    assert _guard_ok(abuf, n * 256, front=GUARD) and _guard_ok(obuf, n * 3)
    return attn.view(n, 256).clone(), o.view(n, 3).clone()


def _o_masked(W):
    from mvgformer_amd import ops
    (Wp, sp), (W0, s0), (W1, s1) = _planes(W["Wp"]), _planes(W["W0"]), _planes(W["W1"])
    return ops.chain_masked_row_output_f32h(Wp, sp, W["bp"], W0, s0, W["b0"], W1, s1, W["b1"], W["W2"], W["b2"])


def _check_a(name, attn, o, samp, inside, W, o_masked=None):
    ref = R.chain_a_f32h(samp, inside, *[W[k] for k in F.A_KEYS])
    assert bool(torch.isfinite(attn).all()) and bool(torch.isfinite(o).all()), name
    _check("chain A attn %s" % name, attn, ref["attn"], ref["attn_err"])         # MI355X: max err / bound 0.13 over all cases
    _check("chain A o %s" % name, o, ref["o"], ref["o_err"])                     # MI355X: 0.015 (masked rows included)
    out = inside == 0
    assert bool((attn[out] == 0).all()), name
    if o_masked is not None:
        assert torch.equal(o[out], o_masked.view(1, 3).expand(int(out.sum()), 3)), name


def _a_rows():
    cus = _cus()
    return [1, 31, 32, 33, 63, 64, 65, 97, 64 * (cus - 1), 64 * (cus - 1) + 1]   # the last two: both sides of the 64-row-tile switch


@pytest.mark.parametrize("mask", ["mixed", "all_in", "all_masked", "mixed_tiles"])
@pytest.mark.parametrize("ri", range(10))
def test_chain_a_against_fp64(ri, mask):
    """attn and o within their elementwise bounds of the fp64 chain; masked rows: attn = 0 exactly, o the cached constant bit
    for bit (and within bound of the fp64 chain of a zero row); tile size 0 / 32 / 64, the processing order (none, in-image
    first, a random permutation) and the all-masked-tile shortcut (o_masked) give bit-identical rows."""
    rows = _a_rows()[ri]
    W = _wa()
    gen = torch.Generator().manual_seed(rows)
    samp = (torch.randn(rows, 256, generator=gen) * torch.exp(torch.randn(rows, 1, generator=gen))).to(DEV)
    if mask in ("mixed", "mixed_tiles"):
        inside = (torch.rand(rows, generator=gen) < 0.6).to(torch.uint8)
        if mask == "mixed_tiles":
            inside[: min(rows, 64)] = 0                               # whole masked tiles of either size without reordering too
            inside[128:256] = 0
    else:
        inside = torch.full((rows,), 1 if mask == "all_in" else 0, dtype=torch.uint8)
    inside = inside.to(DEV)
    orders = {"none": None, "in_first": torch.argsort(1 - inside.int(), stable=True).to(torch.int32),
              "random": torch.randperm(rows, generator=gen).to(torch.int32).to(DEV)}
    om = _o_masked(W)
    res = {}
    for r in (0, 32, 64):
        with _lib().tuning(f32h_rows=r):
            for oname, order in orders.items():
                for given in (False, True):
                    res[(r, oname, given)] = _run_a(samp, inside, W, order, om if given else None)
    base = res[(0, "none", False)]
    _check_a("rows %d %s" % (rows, mask), base[0], base[1], samp, inside, W, om)
    for key, (attn, o) in res.items():
        assert torch.equal(attn, base[0]) and torch.equal(o, base[1]), key


@pytest.mark.parametrize("kind", ["rows_1e-30_1e30", "entries_6_decades", "max_under_2^14", "zero_h0", "zero_h1",
                                  "w_tiny_1_1", "w_1_huge_tiny", "w_huge_tiny_1"])
def test_chain_a_operand_edges(kind):
    """rows from 1e-30 to 1e30, heavy-tailed rows, scaled maxima just under 2^14, all-zero h0 / h1 rows, weight scales of both
    signs: finite and inside the bounds."""
    rows = 97
    wmul = {"w_tiny_1_1": (2.0 ** -30, 1.0, 1.0), "w_1_huge_tiny": (1.0, 2.0 ** 20, 2.0 ** -30), "w_huge_tiny_1": (2.0 ** 20, 2.0 ** -30, 1.0)}
    W = _wa(b0=-1e3) if kind == "zero_h0" else _wa(b1=-1e3) if kind == "zero_h1" else _wa(wmul.get(kind, (1.0, 1.0, 1.0)))
    if kind in wmul:
        sc = [_planes(W[k])[1] for k in ("Wp", "W0", "W1")]
        assert min(sc) < 0 < max(sc) or kind == "w_tiny_1_1", sc
    samp = F.operand_rows(kind if kind in ("rows_1e-30_1e30", "entries_6_decades", "max_under_2^14") else "randn", rows, 31).to(DEV)
    inside = (torch.arange(rows) % 5 != 0).to(torch.uint8).to(DEV)
    attn, o = _run_a(samp, inside, W)
    _check_a(kind, attn, o, samp, inside, W, _o_masked(W))
    if kind in ("zero_h0", "zero_h1"):
        assert bool((o == o[0]).all())                             # every row ends in the same constant


def test_chain_a_non_finite_inputs_stay_in_their_rows():
    """include/mvg_decoder.h: "a non-finite input value makes its output row NaN".  A NaN and an Inf in two inside = 1 rows:
    those rows' attn and o are non-finite, every other row is bit-identical to a run with the two rows zeroed; in inside = 0
    rows the same values give attn = 0 and o = o_masked.  (Regression: ReLU by fmaxf turned the NaN rows of h0 into zeros, so
    o of a NaN row came out finite.)"""
    rows, W = 97, _wa()
    gen = torch.Generator().manual_seed(2)
    samp = torch.randn(rows, 256, generator=gen).to(DEV)
    inside = torch.ones(rows, dtype=torch.uint8, device=DEV)
    inside[[3, 50, 64]] = 0
    bad = samp.clone()
    bad[5, 7], bad[40, 255] = float("nan"), float("inf")            # inside = 1 (rows of two different 32-row tiles)
    bad[3, 0], bad[50, 100] = float("nan"), float("-inf")           # inside = 0
    zero = samp.clone()
    zero[[5, 40]] = 0
    om = _o_masked(W)
    for r in (32, 64):
        with _lib().tuning(f32h_rows=r):
            a1, o1 = _run_a(bad, inside, W, None, om)
            a0, o0 = _run_a(zero, inside, W, None, om)
            for row in (5, 40):
                assert not bool(torch.isfinite(a1[row]).any()) and not bool(torch.isfinite(o1[row]).any()), (r, row)
            others = torch.ones(rows, dtype=torch.bool, device=DEV)
            others[[5, 40]] = False
            assert torch.equal(a1[others], a0[others]) and torch.equal(o1[others], o0[others]), r
            for row in (3, 50, 64):
                assert bool((a1[row] == 0).all()) and torch.equal(o1[row], om), (r, row)


def test_chain_a_argument_checks():
    W = _wa()
    samp = torch.randn(33, 256, device=DEV)
    inside = torch.ones(33, dtype=torch.uint8, device=DEV)
    attn, o = _run_a(samp, inside, W, rows=0)                       # rows = 0: returns 0 and writes nothing
    assert bool(torch.isnan(attn).all()) and bool(torch.isnan(o).all())
    good = [_planes(W[k])[1] for k in ("Wp", "W0", "W1")]
    for i in range(3):
        for bad in (101, -101):
            sc = list(good)
            sc[i] = bad
            attn, o = _run_a(samp, inside, W, scales=sc, expect=BADARG)
            assert bool(torch.isnan(attn).all()) and bool(torch.isnan(o).all())
    big = torch.randn(34 * 256, device=DEV)
    attn, o = _run_a(samp, inside, W, samp_ptr=C.c_void_p(big.data_ptr() + 4), expect=BADARG)
    assert bool(torch.isnan(attn).all())
    attn, o = _run_a(samp, inside, W, rows=32, attn_off=4, expect=BADARG)
    assert bool(torch.isnan(attn).all()) and bool(torch.isnan(o).all())


# ------------------------------------------------------------------------------------------------------------------- chain B
def _run_b(c, W, thr, has_ffn=True, any0=0, call=None):
    """raw C-ABI launch of a case of F.chain_b_inputs (tensors on the device) with guarded outputs; tgt_out is a slice in the
    middle of a larger buffer.  call: overrides of the raw arguments for the argument checks."""
    L = _lib()
    B, NQ, J, V = c["B"], c["NQ"], c["J"], c["V"]
    a = dict(B=B, NQ=NQ, J=J, V=V, n_next=c["n_next"], expect=0, b_next=True, W1=True, scales={})
    a.update(call or {})
    rows, nq = B * NQ * J, B * NQ
    n_next = c["n_next"]
    tbuf, tout = _guarded(rows * 256, front=GUARD)
    pbuf, prob = _guarded(nq * 2)
    vbuf, valid = _guarded(nq, torch.uint8)
    xbuf, xw = _guarded(rows * n_next) if n_next else (None, None)
    anyv = torch.full((1,), any0, dtype=torch.int32, device=DEV)
    pl = {k: _planes(W[k]) for k in ("Wu", "W1", "W2")}
    sc = {k: a["scales"].get(k, pl[k][1]) for k in pl}
    Wn, sn = _planes(W["Wn"][:n_next]) if n_next else (None, 0)
    sn = a["scales"].get("Wn", sn)
    rc = L.load().mvg_chain_update_ffn_class_f32h(
        L.ptr(c["attn"]), a["V"], L.ptr(c["tgt"]), L.ptr(pl["Wu"][0]), sc["Wu"], L.ptr(W["bu"]), L.ptr(W["g2"]), L.ptr(W["be2"]),
        L.ptr(pl["W1"][0]) if a["W1"] else None, sc["W1"], L.ptr(W["b1"]), L.ptr(pl["W2"][0]), sc["W2"], L.ptr(W["b2"]), L.ptr(W["g3"]),
        L.ptr(W["be3"]), L.ptr(W["Wc"]), L.ptr(W["bc"]), float(thr), L.ptr(c["forced"]), L.ptr(tout), L.ptr(prob), L.ptr(valid),
        L.ptr(anyv), L.ptr(c["qpos"]), L.ptr(Wn), sn, L.ptr(W["bn"]) if (n_next and a["b_next"]) else None, L.ptr(xw), a["n_next"],
        a["B"], a["NQ"], a["J"], 1 if has_ffn else 0, L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == a["expect"], rc
    assert _guard_ok(tbuf, rows * 256, front=GUARD) and _guard_ok(pbuf, nq * 2) and _guard_ok(vbuf, nq)
    if n_next:
        assert _guard_ok(xbuf, rows * n_next)
    return dict(tgt=tout.view(rows, 256).clone(), prob=prob.view(nq, 2).clone(), valid=valid.clone(), any=int(anyv[0]),
                xw=None if not n_next else xw.view(rows, n_next).clone())


def _case_dev(c):
    return {k: (v.to(DEV).contiguous() if isinstance(v, torch.Tensor) else v) for k, v in c.items()}


def _same(a, b):
    return all((a[k] is None and b[k] is None) or (torch.equal(a[k], b[k]) if isinstance(a[k], torch.Tensor) else a[k] == b[k])
               for k in ("tgt", "prob", "valid", "any", "xw"))


def _check_b(name, out, ref, any0):
    # MI355X, max err / bound over all cases: tgt' 0.044, prob 0.018, xw_next 0.042
    _check("chain B tgt' %s" % name, out["tgt"], ref["tgt"], ref["tgt_err"])
    _check("chain B prob %s" % name, out["prob"], ref["prob"], ref["prob_err"])
    if out["xw"] is not None:
        _check("chain B xw_next %s" % name, out["xw"], ref["xw"], ref["xw_err"])
    assert not bool(ref["ambiguous"].any()), name                   # no person is left out of the comparison
    assert torch.equal(out["valid"], ref["valid"].to(torch.uint8)), name
    assert out["any"] == int(bool(any0) or bool(ref["valid"].any())), name


def _run_check_b(name, c, W, has_ffn, any0=0, thr=None):
    c = _case_dev(c)
    ref = F.chain_b_ref(c, W, has_ffn, thr)
    outs = {}
    for r in (0, 32, 64):
        with _lib().tuning(f32h_rows=r):
            outs[r] = _run_b(c, W, ref["thr"], has_ffn, any0)
    _check_b(name, outs[0], ref, any0)
    assert _same(outs[32], outs[0]) and _same(outs[64], outs[0]), name
    return c, ref, outs[0]


@pytest.mark.parametrize("k,case", list(enumerate(F.B_CASES)), ids=["B%d_NQ%d_J%d_V%d" % c for c in F.B_CASES])
def test_chain_b_against_fp64(k, case):
    """tgt', prob and xw_next within their bounds, valid exact for EVERY person (the thresholds keep all fp64 prob_1 away from
    them: tests/test_f32h_ref_cpu.py), any_valid = its initial value or any valid.  J 1 .. 32, persons one below / at / above a
    multiple of the persons per tile of both tile sizes, B 1 / 2, V 1 .. 31; has_ffn, forced_valid, any_valid's initial value,
    qpos and n_next (none, 32, 64, 192, 256) cycle over the cases; tile sizes 0 / 32 / 64 bit-identical."""
    opt = F.b_options(k)
    c = F.chain_b_inputs(*case, seed=100 + k, nxt=opt["nxt"], forced=opt["forced"])
    _run_check_b("%s %s" % (case, opt), c, _wb(), opt["has_ffn"], opt["any0"])


@pytest.mark.parametrize("name", F.B_EDGE_NAMES)
def test_chain_b_edge_cases(name):
    """both sides of the tile-size switch (J = 15: 64-row tiles start at ceil(B NQ / 4) > 3 CUs / 4); LayerNorm edge rows (a
    common offset of 1e3, variance 1e-6, variance 1e-5 and constant rows against eps = 1e-5) with and without FFN; view rows
    over 12 decades with tgt rows at 1e-20 and 1e4; a hidden chunk that is entirely zero next to a large one (the per-chunk row
    scale rsh against rs)."""
    c, variant, has_ffn = F.b_edge_cases(_cus())[name]
    _run_check_b(name, c, _wb(variant), has_ffn)


def test_chain_b_threshold_is_strict():
    """valid = prob_1 > threshold: at a person's own fp32 prob_1 it is invalid, one fp32 step below valid."""
    c = _case_dev(F.chain_b_inputs(1, 6, 15, 3, seed=3))
    W = _wb()
    out = _run_b(c, W, 0.5)
    p1 = out["prob"][2, 1].cpu()
    at = _run_b(c, W, float(p1))
    under = _run_b(c, W, float(torch.nextafter(p1, torch.tensor(-float("inf")))))
    assert int(at["valid"][2]) == 0 and int(under["valid"][2]) == 1
    assert torch.equal(at["prob"], out["prob"]) and torch.equal(under["prob"], out["prob"])


def test_chain_b_non_finite_inputs_stay_in_their_rows():
    """a NaN in one view's attn row / in one tgt row: that row of tgt' and xw_next is NaN, the person's prob NaN and valid 0;
    every other row and person -- those of the same tile included -- is bit-identical to a clean run."""
    J, V = 15, 3
    c = _case_dev(F.chain_b_inputs(1, 7, J, V, seed=12, nxt=("q", 192)))
    W = _wb()
    bad = dict(c)
    bad["attn"], bad["tgt"] = c["attn"].clone(), c["tgt"].clone()
    ra, rt = 1 * J + 4, 4 * J + 14                                   # person 1 (shares its tiles with 0 / 0, 2, 3), person 4
    bad["attn"][1, ra, 200] = float("nan")
    bad["tgt"][rt, 0] = float("nan")
    rows_ok = torch.ones(7 * J, dtype=torch.bool, device=DEV)
    rows_ok[[ra, rt]] = False
    pers_ok = torch.ones(7, dtype=torch.bool, device=DEV)
    pers_ok[[1, 4]] = False
    for r in (32, 64):
        with _lib().tuning(f32h_rows=r):
            clean, got = _run_b(c, W, 0.0), _run_b(bad, W, 0.0)        # threshold 0: every clean person is valid
            assert bool(clean["valid"].all())
            for k in ("tgt", "xw"):
                assert bool(torch.isnan(got[k][[ra, rt]]).all()), (r, k)
                assert torch.equal(got[k][rows_ok], clean[k][rows_ok]), (r, k)
            assert bool(torch.isnan(got["prob"][[1, 4]]).all()) and got["valid"][[1, 4]].tolist() == [0, 0], r
            assert torch.equal(got["prob"][pers_ok], clean["prob"][pers_ok]) and torch.equal(got["valid"][pers_ok], clean["valid"][pers_ok])


def test_chain_b_person_permutation():
    """persons in another order (B = 2): every person's rows are bit-identical."""
    B, NQ, J, V = 2, 5, 15, 3
    c = _case_dev(F.chain_b_inputs(B, NQ, J, V, seed=13, nxt=("q", 192)))
    W = _wb()
    nq = B * NQ
    perm = torch.randperm(nq, generator=torch.Generator().manual_seed(1)).to(DEV)
    rperm = (perm[:, None] * J + torch.arange(J, device=DEV)[None]).reshape(-1)
    p = dict(c)
    p["attn"], p["tgt"], p["qpos"] = c["attn"][:, rperm].contiguous(), c["tgt"][rperm].contiguous(), c["qpos"][rperm].contiguous()
    a, b = _run_b(c, W, 0.5), _run_b(p, W, 0.5)
    assert torch.equal(b["tgt"], a["tgt"][rperm]) and torch.equal(b["xw"], a["xw"][rperm])
    assert torch.equal(b["prob"], a["prob"][perm]) and torch.equal(b["valid"], a["valid"][perm])


def test_chain_b_argument_checks():
    c = _case_dev(F.chain_b_inputs(1, 2, 15, 2, seed=1, nxt=("q", 192)))
    W = _wb()
    bad_calls = [dict(J=33), dict(J=0), dict(V=0), dict(n_next=48), dict(n_next=288), dict(b_next=False), dict(W1=False)]
    bad_calls += [dict(scales={k: s}) for k in ("Wu", "W1", "W2", "Wn") for s in (101, -101)]
    for call in bad_calls:
        out = _run_b(c, W, 0.5, call=dict(call, expect=BADARG))
        assert bool(torch.isnan(out["tgt"]).all()) and bool(torch.isnan(out["prob"]).all()) and bool((out["valid"] == FILL_U8).all()), call
    for call in (dict(B=0), dict(NQ=0)):                            # B * NQ = 0: returns 0, writes nothing
        out = _run_b(c, W, 0.5, call=dict(call, expect=0))
        assert bool(torch.isnan(out["tgt"]).all()) and bool(torch.isnan(out["xw"]).all()) and out["any"] == 0, call


# ------------------------------------------------------------------------------------------------------------------- pyramid
def pyr_split(rows, n_g, cus):
    """(tiles, (slots of value, slots of G)) per XCD.  Restates the launcher mvg_pyramid_f32h in csrc/f32s.hip, from
    `const long ntiles_ws = (rows + WS_RM - 1) / WS_RM;` to `p.slots[0] = s0; p.slots[1] = per_xcd - s0;`."""
    ntiles = (rows + 31) // 32
    per_xcd = max(min(cus // 8, 32), 2)
    per_xcd = min(per_xcd, (ntiles + 7) // 8 * 2)
    s0 = (per_xcd * 256 + (256 + n_g) // 2) // (256 + n_g)
    s0 = min(max(s0, 1), per_xcd - 1)
    return ntiles, (s0, per_xcd - s0)


def pyr_tile_counts(rows, n_g, cus):
    """per product, the set of tile counts its workgroups process: workgroup (xcd, slot i) of a product with s slots starts at
    tile 8 i + xcd and steps by 8 s (pyramid_ws_f32h_kernel: `first`, `G`)."""
    ntiles, slots = pyr_split(rows, n_g, cus)
    return [{-(-(ntiles - f) // (8 * s)) for f in range(8 * s) if f < ntiles} for s in slots]


def pyr_rows(n_g, cus):
    """the small row counts plus two computed from the slot split: 3 and 4 tiles per workgroup with rows % 32 = 1, and 1 and 2
    tiles with rows % 32 = 31."""
    _, slots = pyr_split(1 << 20, n_g, cus)
    gmax = 8 * max(slots)
    return [1, 31, 32, 33, 255, 256, 257, 288, 32 * (3 * gmax) + 1, 32 * (gmax + 1) + 31]


_PYR_W = {}


def _pyr_weights(n_g):
    if n_g not in _PYR_W:
        gen = torch.Generator().manual_seed(21 + n_g)
        _PYR_W[n_g] = tuple(t.to(DEV) for t in (torch.randn(256, 256, generator=gen) / 16, torch.randn(256, generator=gen),
                                                 torch.randn(n_g, 256, generator=gen) / 16))
    return _PYR_W[n_g]


def _run_pyr(feat, n_g, rows=None, n_g_arg=None, feat_off=0, scales=None, expect=0):
    L = _lib()
    Wv, bv, Wg = _pyr_weights(n_g)
    n = feat.shape[0]
    rows = n if rows is None else rows
    (pv, sv), (pg, sg) = _planes(Wv), _planes(Wg)
    if scales is not None:
        sv, sg = scales
    vbuf, value = _guarded(n * 256, front=GUARD)
    gbuf, G = _guarded(n * n_g, front=GUARD)
    rc = L.load().mvg_pyramid_f32h(C.c_void_p(feat.data_ptr() + feat_off), L.ptr(pv), sv, L.ptr(bv), L.ptr(pg), sg, L.ptr(value), L.ptr(G),
                                   rows, n_g if n_g_arg is None else n_g_arg, L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, rc
    assert _guard_ok(vbuf, n * 256, front=GUARD) and _guard_ok(gbuf, n * n_g, front=GUARD)
    return value.view(n, 256).clone(), G.view(n, n_g).clone()


def _check_pyr(name, feat, n_g, value, G):
    Wv, bv, Wg = _pyr_weights(n_g)
    ref = R.pyramid_f32h(feat, Wv, bv, Wg)
    _check("pyramid value %s" % name, value, ref["value"], ref["value_err"])      # MI355X: max err / bound 0.13 over all cases
    _check("pyramid G %s" % name, G, ref["G"], ref["G_err"])                      # MI355X: 0.13


def test_pyramid_row_counts_cover_every_tile_path():
    """across the cases of test_pyramid_against_fp64, workgroups of each product process 1, 2, 3 and >= 4 tiles (tile_body's
    <no previous, no next>, <first, last> and <middle> cases), with a ragged last tile of 1 and of 31 rows."""
    cus = _cus()
    seen = [set(), set()]
    for n_g in (32, 64, 192, 256):
        for rows in pyr_rows(n_g, cus):
            for j, s in enumerate(pyr_tile_counts(rows, n_g, cus)):
                seen[j] |= s
        assert {r % 32 for r in pyr_rows(n_g, cus)[-2:]} == {1, 31}
    for s in seen:
        assert {1, 2, 3} <= s and max(s) >= 4, seen


@pytest.mark.parametrize("ri", range(10))
@pytest.mark.parametrize("n_g", [32, 64, 192, 256])
def test_pyramid_against_fp64(n_g, ri):
    """value (with bias) and G within their elementwise bounds, guards intact; rows permuted: bit-identical."""
    rows = pyr_rows(n_g, _cus())[ri]
    gen = torch.Generator().manual_seed(rows + n_g)
    feat = (torch.randn(rows, 256, generator=gen) * torch.exp(torch.randn(rows, 1, generator=gen))).to(DEV)
    value, G = _run_pyr(feat, n_g)
    _check_pyr("rows %d n_g %d" % (rows, n_g), feat, n_g, value, G)
    perm = torch.randperm(rows, generator=gen).to(DEV)
    v2, G2 = _run_pyr(feat[perm].contiguous(), n_g)
    assert torch.equal(v2, value[perm]) and torch.equal(G2, G[perm])


@pytest.mark.parametrize("kind", ["rows_12_decades", "rows_1e-30_1e30", "entries_6_decades", "zero_rows", "max_under_2^14"])
def test_pyramid_operand_edges(kind):
    feat = F.operand_rows(kind, 289, 41).to(DEV)
    value, G = _run_pyr(feat, 192)
    assert bool(torch.isfinite(value).all()) and bool(torch.isfinite(G).all())
    _check_pyr(kind, feat, 192, value, G)
    if kind == "zero_rows":
        assert torch.equal(value[::3], _pyr_weights(192)[1].view(1, 256).expand(value[::3].shape[0], 256)) and bool((G[::3] == 0).all())


def test_pyramid_argument_checks():
    feat = torch.randn(65, 256, device=DEV)
    untouched = lambda v, g: bool(torch.isnan(v).all()) and bool(torch.isnan(g).all())
    for bad in (0, 33, 288):
        assert untouched(*_run_pyr(feat, 32, n_g_arg=bad, expect=BADARG)), bad
    good = [_planes(w)[1] for w in (_pyr_weights(32)[0], _pyr_weights(32)[2])]
    for i in range(2):
        for bad in (101, -101):
            sc = list(good)
            sc[i] = bad
            assert untouched(*_run_pyr(feat, 32, scales=sc, expect=BADARG)), (i, bad)
    assert untouched(*_run_pyr(feat, 32, rows=64, feat_off=4, expect=BADARG))
    assert untouched(*_run_pyr(feat, 32, rows=0))
