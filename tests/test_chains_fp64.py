"""The bf16 chains (mvg_chain_attn_pose, mvg_chain_update_ffn_class: csrc/chain.hip) and the layer-tail kernels of the
unfused path (mvg_mean_views, mvg_add_layernorm, mvg_class_head, mvg_rowdot3: csrc/geom.hip) against fp64 statements of their
own operation (tests/chain_ref.py, pinned to the oracle by tests/test_chain_ref_oracle.py), at the shapes where their code
switches paths.  Bounds come from the kernels' rounding points (chain_ref's notes); each assertion prints max |err| / bound.
Every output buffer carries a guard region filled with a sentinel, which must come back untouched."""
import pytest
import torch

from tests import chain_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 1024                    # elements past the end of every output (and in front of tgt_out)
SENT_F, SENT_U8 = -7.25e5, 0xA5
BADARG = 10001                  # MVG_E_BADARG


def _lib():
    from mvgformer_amd import _lib as L
    return L


def _guarded(n, dtype, front=0):
    """(buffer, view of n elements at offset `front`): the rest of the buffer is the guard, filled with the sentinel."""
    buf = torch.full((front + n + GUARD,), SENT_U8 if dtype == torch.uint8 else SENT_F, dtype=dtype, device=DEV)
    return buf, buf[front:front + n]


def _guard_ok(buf, n, front=0):
    s = SENT_U8 if buf.dtype == torch.uint8 else SENT_F
    return bool((buf[:front] == s).all()) and bool((buf[front + n:] == s).all())


def _check(name, got, ref, bound, factor=1.0):
    """|got - ref| <= factor * bound elementwise (factor LAMBDA: a typical error size from chain_ref.lin_err / ln_err)."""
    bound = factor * bound
    err = (got.double() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print("%s: max err %.2e, max err / bound %.3f" % (name, float(err.max()) if err.numel() else 0.0, ratio))
    assert bool((err <= bound).all()), (name, ratio)


def _bf16_w(gen, n, k):
    return (torch.randn(n, k, generator=gen) / k ** 0.5).to(torch.bfloat16).to(DEV)


def _f32(gen, *s, scale=1.0):
    return (torch.randn(*s, generator=gen) * scale).to(DEV)


# ------------------------------------------------------------------------------------------------------------------- chain A
def _chain_a_weights(seed):
    gen = torch.Generator().manual_seed(seed)
    W = dict(Wp=_bf16_w(gen, 256, 256), W0=_bf16_w(gen, 256, 256), W1=_bf16_w(gen, 256, 256))
    W.update(bp=_f32(gen, 256, scale=0.1), b0=_f32(gen, 256, scale=0.1), b1=_f32(gen, 256, scale=0.1),
             W2=_f32(gen, 3, 256, scale=1 / 16), b2=_f32(gen, 3))
    return W


def _run_chain_a(samp, inside, W, order=None, o_masked=None):
    L = _lib()
    rows = samp.shape[0]
    abuf, attn = _guarded(rows * 256, torch.bfloat16)
    obuf, o = _guarded(rows * 3, torch.float32)
    sw = {k: R_swz(W[k]) for k in ("Wp", "W0", "W1")}
    L.check(L.load().mvg_chain_attn_pose(L.ptr(samp), L.ptr(inside), L.ptr(sw["Wp"]), L.ptr(W["bp"]), L.ptr(sw["W0"]),
                                         L.ptr(W["b0"]), L.ptr(sw["W1"]), L.ptr(W["b1"]), L.ptr(W["W2"]), L.ptr(W["b2"]),
                                         L.ptr(attn), L.ptr(o), L.ptr(order), L.ptr(o_masked), rows, L.stream_ptr()),
            "mvg_chain_attn_pose")
    torch.cuda.synchronize()
    assert abuf.view(torch.int16)[rows * 256:].eq(torch.tensor(SENT_F, dtype=torch.bfloat16).view(torch.int16).item()).all()
    assert _guard_ok(obuf, rows * 3)
    return attn.view(rows, 256).clone(), o.view(rows, 3).clone()


_SWZ = {}


def R_swz(w):
    from mvgformer_amd import ops
    key = w.data_ptr()
    if key not in _SWZ:
        _SWZ[key] = (w, ops.swizzle_weight(w))
    return _SWZ[key][1]


def _bf_next(x, up):
    """the bf16 value next to the bf16-valued x towards +inf (up) or -inf, by its bit pattern."""
    t = x.to(torch.bfloat16)
    b = t.view(torch.int16).int()
    if up:
        n = torch.where(t > 0, b + 1, torch.where(t < 0, b - 1, torch.ones_like(b)))
    else:
        n = torch.where(t > 0, b - 1, torch.where(t < 0, b + 1, torch.full_like(b, -32767)))
    return n.to(torch.int16).view(torch.bfloat16).double()


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 127, 128, 129, 40960, 40961, 76800])
@pytest.mark.parametrize("mask", ["mixed", "all_in", "all_masked"])
def test_chain_a_against_fp64(rows, mask):
    """attn: one of the two bf16 neighbours of the exact value (>= 99.9 % the nearest); o within the bound of the bf16
    roundings of h0 / h1 (chain_ref.chain_a, run on the kernel's own attn rows); masked rows: attn = 0 and o = the chain of a
    zero row.  64- / 128-row tiles and auto_small give bit-identical rows (chain.hip: mvg_chain_attn_pose) -- with and without
    the processing order / all-masked-tile skip; 256-row tiles are bounded against fp64 on their own."""
    from mvgformer_amd import ops
    W = _chain_a_weights(7)
    gen = torch.Generator().manual_seed(rows)
    samp = torch.randn(rows, 256, generator=gen).to(torch.bfloat16).to(DEV)
    if mask == "mixed":
        inside = (torch.rand(rows, generator=gen) < 0.6).to(torch.uint8)
        inside[64:192] = 0                                           # whole masked tiles without reordering too
    else:
        inside = torch.full((rows,), 1 if mask == "all_in" else 0, dtype=torch.uint8)
    inside = inside.to(DEV)
    order = torch.argsort(1 - inside.int(), stable=True).to(torch.int32)
    wl = [W[k] for k in ("Wp", "bp", "W0", "b0", "W1", "b1", "W2", "b2")]
    sw = [R_swz(W["Wp"]), W["bp"], R_swz(W["W0"]), W["b0"], R_swz(W["W1"]), W["b1"], W["W2"], W["b2"]]
    res = {}
    for rm, small in ((128, 1), (128, 0), (64, 1), (256, 1)):
        with _lib().tuning(chain_rm=rm, auto_small=small):
            o_masked = ops.chain_masked_row_output(*sw)
            for ordered in (False, True):
                res[(rm, small, ordered)] = _run_chain_a(samp, inside, W, order if ordered else None, o_masked if ordered else None)
    keep = inside != 0
    for key, (attn, o) in res.items():
        ref = R.chain_a(samp, inside, *wl, bf16=True, attn=attn)
        ex = ref["attn_exact"]
        near = R.bf(ex)
        # one of the two neighbours of exact (widened by the fp32 accumulation where the value cancels to below it)
        step = R.round_err(ex, ref["attn_err"], rms=False)
        lo, hi = torch.minimum(near, R.bf(ex - ref["attn_err"])), torch.maximum(near, R.bf(ex + ref["attn_err"]))
        nb_lo = torch.where(near <= ex, near, _bf_next(near, up=False))
        nb_hi = torch.where(near >= ex, near, _bf_next(near, up=True))
        a = attn.double()
        assert bool(((a >= torch.minimum(lo, nb_lo)) & (a <= torch.maximum(hi, nb_hi))).all()), key
        if bool(keep.any()):
            off = int((a[keep] != near[keep]).sum())
            print("chain A %s rows %d %s: attn not nearest %d of %d, widest step %.2e" % (key, rows, mask, off, a[keep].numel(), float(step.max())))
            # >= 99.9 % the nearest (2 spare for one-row launches); MI355X: 6.6e-5 of all elements, 2 of 9984 at worst
            assert off <= 2 + 1e-3 * a[keep].numel(), key
        assert bool((attn[~keep] == 0).all())
        _check("chain A o %s" % (key,), o, ref["o"], ref["o_err"])           # MI355X: max err / bound 0.27
        if not bool(keep.all()):                                     # masked rows: the fp64 chain of a zero row
            z = R.chain_a(torch.zeros(1, 256, device=DEV), torch.zeros(1, dtype=torch.uint8, device=DEV), *wl, bf16=True,
                          attn=torch.zeros(1, 256, device=DEV))
            _check("chain A masked o", o[~keep], z["o"].expand(int((~keep).sum()), 3), z["o_err"].expand(int((~keep).sum()), 3))
    base = res[(128, 1, False)]
    for key in ((128, 1, True), (128, 0, False), (128, 0, True), (64, 1, False), (64, 1, True)):
        assert torch.equal(res[key][0], base[0]) and torch.equal(res[key][1], base[1]), key


# ------------------------------------------------------------------------------------------------------------------- chain B
def _chain_b_weights(seed):
    gen = torch.Generator().manual_seed(seed)
    W = dict(Wu=_bf16_w(gen, 256, 256), W1=_bf16_w(gen, 1024, 256), W2=_bf16_w(gen, 256, 1024), Wn=_bf16_w(gen, 256, 256))
    W.update(bu=_f32(gen, 256, scale=0.1), b1=_f32(gen, 1024, scale=0.1), b2=_f32(gen, 256, scale=0.1),
             g2=1 + _f32(gen, 256, scale=0.1), be2=_f32(gen, 256, scale=0.1), g3=1 + _f32(gen, 256, scale=0.1),
             be3=_f32(gen, 256, scale=0.1), Wc=_f32(gen, 2, 256, scale=1 / 16), bc=_f32(gen, 2), bn=_f32(gen, 256, scale=0.1))
    return W


def _run_chain_b(attn, V, tgt, W, threshold, B, NQ, J, has_ffn=True, forced=None, qpos=None, n_next=0, inside=None,
                 any_valid=None):
    """raw C-ABI launch with guarded outputs; tgt_out is a slice in the middle of a larger buffer."""
    L = _lib()
    rows, nq = B * NQ * J, B * NQ
    tbuf, tout = _guarded(rows * 256, torch.float32, front=GUARD)
    pbuf, prob = _guarded(nq * 2, torch.float32)
    vbuf, valid = _guarded(nq, torch.uint8)
    xbuf, xw = _guarded(rows * n_next, torch.float32) if n_next else (None, None)
    if any_valid is None:
        any_valid = torch.zeros(1, dtype=torch.int32, device=DEV)
    sw = lambda k: R_swz(W[k])
    L.check(L.load().mvg_chain_update_ffn_class(
        L.ptr(attn), V, L.ptr(tgt), L.ptr(sw("Wu")), L.ptr(W["bu"]), L.ptr(W["g2"]), L.ptr(W["be2"]), L.ptr(sw("W1")),
        L.ptr(W["b1"]), L.ptr(sw("W2")), L.ptr(W["b2"]), L.ptr(W["g3"]), L.ptr(W["be3"]), L.ptr(W["Wc"]), L.ptr(W["bc"]),
        float(threshold), L.ptr(forced), L.ptr(tout), L.ptr(prob), L.ptr(valid), L.ptr(any_valid), L.ptr(qpos),
        L.ptr(sw("Wn")) if n_next else None, L.ptr(W["bn"]) if n_next else None, L.ptr(xw), n_next, B, NQ, J,
        1 if has_ffn else 0, L.ptr(inside), L.stream_ptr()), "mvg_chain_update_ffn_class")
    torch.cuda.synchronize()
    assert _guard_ok(tbuf, rows * 256, front=GUARD) and _guard_ok(pbuf, nq * 2) and _guard_ok(vbuf, nq)
    if n_next:
        assert _guard_ok(xbuf, rows * n_next)
    return dict(tgt=tout.view(rows, 256).clone(), prob=prob.view(nq, 2).clone(), valid=valid.clone(), any=any_valid.clone(),
                xw=None if not n_next else xw.view(rows, n_next).clone())


def _check_b(out, ref):
    # MI355X, max err / bound over all cases: tgt' 0.24, prob 0.06, xw_next 0.26
    _check("chain B tgt'", out["tgt"], ref["tgt"], ref["tgt_err"])
    _check("chain B prob", out["prob"], ref["prob"], ref["prob_err"])
    if out["xw"] is not None:
        _check("chain B xw_next", out["xw"], ref["xw"], ref["xw_err"])
    # valid: exact, except where the fp64 prob_1 is within its bound of the threshold
    amb = (ref["prob"][:, 1] - ref["thr"]).abs() <= ref["prob_err"][:, 1]
    if ref["forced"] is not None:
        amb = torch.zeros_like(amb)
    assert torch.equal(out["valid"].bool()[~amb], ref["valid"][~amb])
    assert int(out["any"][0]) == int(ref["any0"] or bool(out["valid"].any()))


def _chain_b_case(B, NQ, J, V, has_ffn, with_inside, nxt, forced, seed, ln_edges=False, any0=0, thr=0.5):
    W = _chain_b_weights(11)
    gen = torch.Generator().manual_seed(seed)
    rows, nq = B * NQ * J, B * NQ
    attn = torch.randn(V, rows, 256, generator=gen).to(torch.bfloat16)
    inside = (torch.rand(V, rows, generator=gen) < 0.7).to(torch.uint8) if with_inside else None
    if inside is not None:
        attn[inside == 0] = 0                                      # chain A's rows outside the image are zero
    tgt = torch.randn(rows, 256, generator=gen)
    if ln_edges:                                                   # LayerNorm inputs: a large common offset, nearly constant rows
        n = min(rows, 4 * J)
        attn[:, :n] = 0
        bu = W["bu"].cpu()
        tgt[: n // 4] = 1e3 + tgt[: n // 4]
        tgt[n // 4: n // 2] = 0.25 - bu + 1e-3 * tgt[n // 4: n // 2]            # variance ~ 1e-6 (< eps)
        tgt[n // 2: 3 * n // 4] = -1.5 - bu + 3e-3 * tgt[n // 2: 3 * n // 4]    # ~ 1e-5 (= eps)
        tgt[3 * n // 4: n] = 0.5 - bu                                             # ~ 0
        if inside is not None:
            inside[:, :n] = 0
    attn, tgt = attn.to(DEV), tgt.to(DEV)
    inside = None if inside is None else inside.to(DEV)
    qpos, n_next = (None, 0) if nxt is None else ((None if nxt[0] is None else _f32(gen, rows, 256)), nxt[1])
    fv = None if not forced else (torch.rand(nq, generator=gen) < 0.5).to(torch.uint8).to(DEV)
    anyv = torch.full((1,), any0, dtype=torch.int32, device=DEV)
    out = _run_chain_b(attn.view(V * rows, 256), V, tgt, W, thr, B, NQ, J, has_ffn, fv, qpos, n_next, inside, anyv)
    ref = R.chain_b(attn, tgt, W["Wu"], W["bu"], W["g2"], W["be2"], W["W1"], W["b1"], W["W2"], W["b2"], W["g3"], W["be3"],
                    W["Wc"], W["bc"], thr, J, has_ffn=has_ffn, forced=fv, qpos=qpos, Wn=W["Wn"] if n_next else None,
                    bn=W["bn"], n_next=n_next, bf16=True)
    ref.update(thr=thr, forced=fv, any0=any0)
    return out, ref, dict(attn=attn, tgt=tgt, W=W, inside=inside, qpos=qpos, n_next=n_next, fv=fv)


_NEXT = [None, (None, 4), ("q", 192), ("q", 256)]
_B_CASES = ([(2, 64 // J + 1 if J <= 32 else 3, J, V) for J, V in zip((1, 14, 15, 16, 17, 21, 32, 33, 64), (3, 5, 6, 1, 7, 10, 4, 9, 2))]
            + [(1, 9, 15, V) for V in (1, 3, 4, 5, 6, 7, 8, 9, 10, 16, 17, 31)]
            + [(2, 256, 15, 5), (2, 257, 15, 5), (1, 511, 15, 3), (1, 513, 15, 3)])


@pytest.mark.parametrize("k,case", list(enumerate(_B_CASES)), ids=["B%d_NQ%d_J%d_V%d" % c for c in _B_CASES])
def test_chain_b_against_fp64(k, case):
    """tgt', prob and xw_next within the bounds of the kernel's rounding points; valid exact away from the threshold; any_valid.
    Persons per tile ragged (64 // J per 64-row tile), J up to 64, the V > 5 view-mean path, both sides of the 32 / 64-row
    tile switch (<= 128 tiles); has_ffn, attn_inside, next_query_proj (qpos None / given, n_next 4 / 192 / 256) and forced
    cycle over the cases."""
    B, NQ, J, V = case
    out, ref, _ = _chain_b_case(B, NQ, J, V, has_ffn=k % 3 != 2, with_inside=k % 2 == 0, nxt=_NEXT[k % 4], forced=k % 5 == 3,
                                seed=100 + k, any0=k % 7 == 1, thr=0.5)
    _check_b(out, ref)


@pytest.mark.parametrize("has_ffn", [0, 1])
def test_chain_b_layernorm_edge_rows(has_ffn):
    """rows with a common offset of 1e3 and nearly constant rows (variance 1e-6, 1e-5, 0 against eps = 1e-5): the epsilon and
    the two-pass variance of LN2 (and LN3) are pinned."""
    out, ref, _ = _chain_b_case(2, 9, 15, 3, has_ffn=bool(has_ffn), with_inside=True, nxt=("q", 192), forced=False, seed=5,
                                ln_edges=True)
    _check_b(out, ref)


def test_chain_b_does_not_read_masked_attn_rows():
    """attn rows whose attn_inside flag is 0 are not read: filled with NaN they give finite outputs, bit-identical to zeros there."""
    out, ref, c = _chain_b_case(1, 20, 15, 6, has_ffn=True, with_inside=True, nxt=("q", 192), forced=False, seed=9)
    _check_b(out, ref)
    nan_attn = c["attn"].clone()
    nan_attn[c["inside"] == 0] = float("nan")
    B, NQ, J, V = 1, 20, 15, 6
    o2 = _run_chain_b(nan_attn.view(V * B * NQ * J, 256), V, c["tgt"], c["W"], 0.5, B, NQ, J, True, None, c["qpos"], 192,
                      c["inside"])
    assert all(bool(torch.isfinite(o2[k]).all()) for k in ("tgt", "prob", "xw"))
    for k in ("tgt", "prob", "valid", "xw"):
        assert torch.equal(o2[k], out[k]), k


def test_chain_b_threshold_is_strict():
    """valid = prob_1 > threshold: at threshold = the query's own fp32 prob_1 it is invalid, one fp32 step below valid."""
    _, _, c = _chain_b_case(1, 6, 15, 3, has_ffn=True, with_inside=False, nxt=None, forced=False, seed=3)
    run = lambda thr: _run_chain_b(c["attn"].view(-1, 256), 3, c["tgt"], c["W"], thr, 1, 6, 15)
    out = run(0.5)
    p1 = out["prob"][2, 1].float().cpu()
    below = float(torch.nextafter(p1, torch.tensor(-float("inf"))))
    at, under = run(float(p1)), run(below)
    assert int(at["valid"][2]) == 0 and int(under["valid"][2]) == 1
    assert torch.equal(at["prob"], out["prob"])


# --------------------------------------------------------------------------------------------------------- layer-tail kernels
def _mean_ref(a, V, rows, C):
    return a.double().view(V, rows, C).mean(0)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V", [1, 2, 5, 31])
def test_mean_views_against_fp64(dt, V):
    L = _lib()
    rows, C = 37, 260                                               # rows * C / 4 = 2405: a ragged last workgroup
    gen = torch.Generator().manual_seed(V)
    a = torch.randn(V * rows, C, generator=gen).to(dt).to(DEV)
    buf, out = _guarded(rows * C, dt)
    L.check(L.load().mvg_mean_views(L.ptr(a), L.dtype_code(dt), L.ptr(out), V, rows, C, L.stream_ptr()), "mvg_mean_views")
    torch.cuda.synchronize()
    if dt == torch.bfloat16:
        assert buf.view(torch.int16)[rows * C:].eq(torch.tensor(SENT_F, dtype=torch.bfloat16).view(torch.int16).item()).all()
    else:
        assert _guard_ok(buf, rows * C)
    m = _mean_ref(a, V, rows, C)
    d = (V + 2) * R.U32 * a.double().view(V, rows, C).abs().mean(0)            # fp32 sum of V terms, the division
    bound = R.round_err(m, d, rms=False) if dt == torch.bfloat16 else d         # MI355X: bf16 exact, f32 0.37 of d
    _check("mean_views %s V=%d" % (dt, V), out.view(rows, C), R.bf(m) if dt == torch.bfloat16 else m, bound)


def _ln_rows(gen, rows, C):
    res = torch.randn(rows, C, generator=gen)
    res[0] += 1e3                                                    # a large common offset
    res[1] = 0.25 + 1e-3 * res[1]                                    # variance ~ 1e-6 < eps
    res[2] = -1.5 + 3e-3 * res[2]                                    # ~ 1e-5 = eps
    res[3] = 0.5                                                     # constant
    return res


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [4, 64, 256, 260, 1024])
def test_add_layernorm_against_fp64(dt, C):
    L = _lib()
    rows = 4 * 9 + 3
    gen = torch.Generator().manual_seed(C)
    res = _ln_rows(gen, rows, C).to(DEV)
    h = torch.randn(rows, C, generator=gen)
    h[1:4] = 0
    h = h.to(dt).to(DEV)
    g, b = (1 + 0.1 * torch.randn(C, generator=gen)).to(DEV), (0.1 * torch.randn(C, generator=gen)).to(DEV)
    buf, y = _guarded(rows * C, torch.float32)
    L.check(L.load().mvg_add_layernorm(L.ptr(res), L.ptr(h), L.dtype_code(dt), L.ptr(g), L.ptr(b), L.ptr(y), rows, C,
                                       L.stream_ptr()), "mvg_add_layernorm")
    torch.cuda.synchronize()
    assert _guard_ok(buf, rows * C)
    x = res.double() + h.double()                                    # MI355X: max err / bound 0.03
    _check("add_layernorm %s C=%d" % (dt, C), y.view(rows, C), R.ln(x, g, b),
           R.ln_err(x, R.U32 * x.abs(), g) + R.U32 * (b.double().abs() + R.ln(x, g, b).abs()), R.LAMBDA)


@pytest.mark.parametrize("C", [256, 64])
@pytest.mark.parametrize("J", [1, 15, 16, 17, 32, 33])
def test_class_head_against_fp64(C, J):
    """prob = mean_j sigmoid(Wc tgt + bc) (the C = 256 path reduces joints in chunks of 16), valid, any_valid, forced, and
    the strict threshold."""
    L = _lib()
    B, NQ = 2, 7
    nq, rows = B * NQ, B * NQ * J
    gen = torch.Generator().manual_seed(J * 1000 + C)
    tgt = torch.randn(rows, C, generator=gen).to(DEV)
    Wc, bc = (torch.randn(2, C, generator=gen) / C ** 0.5).to(DEV), torch.randn(2, generator=gen).to(DEV)
    sg = torch.sigmoid(R.lin(tgt, Wc, bc))
    pr = sg.view(nq, J, 2).mean(1)
    el = R.lin_err(tgt, None, Wc, bc)
    el = R.LAMBDA * el
    pe = ((sg * (1 - sg) + el).clamp(max=0.25) * el + 4 * R.U32 * sg).view(nq, J, 2).mean(1) + (J + 1) * R.U32 * pr

    def run(thr, forced=None, any0=0):
        pbuf, prob = _guarded(nq * 2, torch.float32)
        vbuf, valid = _guarded(nq, torch.uint8)
        anyv = torch.full((1,), any0, dtype=torch.int32, device=DEV)
        L.check(L.load().mvg_class_head(L.ptr(tgt), L.ptr(Wc), L.ptr(bc), float(thr), L.ptr(forced),
                                        L.ptr(prob), L.ptr(valid), L.ptr(anyv), B, NQ, J, C, L.stream_ptr()), "mvg_class_head")
        torch.cuda.synchronize()
        assert _guard_ok(pbuf, nq * 2) and _guard_ok(vbuf, nq)
        return prob.view(nq, 2).clone(), valid.clone(), int(anyv[0])

    thr = float(pr[:, 1].median())
    prob, valid, anyv = run(thr)
    _check("class_head C=%d J=%d" % (C, J), prob, pr, pe)                 # MI355X: max err / bound 0.08
    amb = (pr[:, 1] - thr).abs() <= pe[:, 1]
    assert torch.equal(valid.bool()[~amb], (pr[:, 1] > thr)[~amb]) and anyv == int(bool(valid.any()))
    forced = (torch.arange(nq) % 3 == 0).to(torch.uint8).to(DEV)
    _, v2, a2 = run(2.0, forced)
    assert torch.equal(v2, forced) and a2 == 1
    _, v3, a3 = run(2.0, None, any0=1)                             # a caller-owned flag that is already 1 stays 1
    assert int(v3.sum()) == 0 and a3 == 1
    p1 = prob[3, 1].cpu()
    _, v_at, _ = run(float(p1))
    _, v_below, _ = run(float(torch.nextafter(p1, torch.tensor(-float("inf")))))
    assert int(v_at[3]) == 0 and int(v_below[3]) == 1


def test_class_head_rejects_zero_joints():
    L = _lib()
    t = torch.zeros(64, 256, device=DEV)
    Wc, bc = torch.zeros(2, 256, device=DEV), torch.zeros(2, device=DEV)
    prob, valid = torch.zeros(8, 2, device=DEV), torch.zeros(8, dtype=torch.uint8, device=DEV)
    anyv = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = L.load().mvg_class_head(L.ptr(t), L.ptr(Wc), L.ptr(bc), 0.5, None, L.ptr(prob), L.ptr(valid), L.ptr(anyv), 2, 4, 0, 256,
                                 L.stream_ptr())
    assert rc == BADARG


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [256, 64, 512])
def test_rowdot3_against_fp64(dt, C):
    L = _lib()
    rows = 4 * 11 + 1
    gen = torch.Generator().manual_seed(C)
    h = torch.randn(rows, C, generator=gen).to(dt).to(DEV)
    W3, b3 = (torch.randn(3, C, generator=gen) / C ** 0.5).to(DEV), torch.randn(3, generator=gen).to(DEV)
    buf, o = _guarded(rows * 3, torch.float32)
    L.check(L.load().mvg_rowdot3(L.ptr(h), L.dtype_code(dt), L.ptr(W3), L.ptr(b3), L.ptr(o), rows, C, L.stream_ptr()), "mvg_rowdot3")
    torch.cuda.synchronize()
    assert _guard_ok(buf, rows * 3)
    # MI355X: max err / bound 0.05
    _check("rowdot3 %s C=%d" % (dt, C), o.view(rows, 3), R.lin(h, W3, b3), R.lin_err(h, None, W3, b3), R.LAMBDA)
