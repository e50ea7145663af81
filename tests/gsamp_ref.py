"""TEST INFRASTRUCTURE ONLY.  fp64 restatement of the decoder's fused sampling operation -- offsets and logits gathered from G at the
reference point, the memory reinterpretation, softmax, locations, sampling -- with the error scale of every output element: the reference
that tests/test_gsamp_fp64.py holds msda_gsamp_kernel / msda_gsamp_pipe_kernel, msda_gfused_f32_hp_kernel and msda_fused_kernel
(csrc/msda.hip, csrc/gsamp_dev.h) to.  Built from the operation's definition, oracle/decoder_ref.proj_attn_forward, and the G-commutation
    Linear(bilinear(feat, p) + x) = bilinear(feat @ W^T, p) + (x @ W^T + b);
pinned to the oracle by tests/test_gsamp_ref_cpu.py.

Inputs are in the kernels' own layout: value as head planes (n_img, 8, S, 32) or row-major (n_img, S, 256); G (n_img * S, 192) and
xw (B * Lq, 192) with their columns in ops.gsamp_column_order() (COLUMN_ORDER below restates it); ref_lvl (n_img, Lq, L, 2) as (x, y);
shapes (L, 2) int64 (H, W); starts (L,); image n takes the xw rows of batch item n % B; pair_mask / order (n_img * Lq) or None.
fused() takes oa (pairs * L, 192) in the Linear's natural column order instead of G and xw (msda_fused_kernel).

The statement, per (image, query) pair:
  footprint   grid = clamp(2 r_l - 1, -1.1, 1.1); ix = ((grid_x + 1) W_l - 1) / 2 (align_corners = False); the four corners of the cell
              floor(ix), floor(iy) with bilinear weights, a corner outside the map contributes 0 (zeros padding);
              x_l = sum_c w_c G_l[c] + xw                                                                   (L rows of 192 columns)
  view        the (L, 128) offset columns are VIEWED as (M, L, P, 2) and the (L, 64) logit columns as (M, L * P)   (M = P = 8)
  softmax     over a head's L * P logits
  locations   loc = r_l + off / (W_l, H_l)
  sampling    tests/msda_ref.msda (bounds test, zero-padded bilinear taps, weighted sum)

Every intermediate carries its value and an error scale E in units of the working epsilon: an evaluation in that precision, in any
order, is within a few eps * E of the value.
  x (phase A)     sum_c |w_c G_c| + |xw| + Dx * Ex + Dy * Ey: D the slope of G's bilinear surface at the footprint (a Lipschitz bound, see
                  _lipschitz), Ex the sum of the absolute values of the terms of ix
  a_i             relative scale 1 + E(logit_i) + max_j E(logit_j) + |logit_i - lse|: the logit's own error, the error of the
                  denominator, and what an exp evaluated as exp2(x * log2 e) loses on an exponent of that size
  out             out_A = the sum of the absolute values of the output's terms with the weights a_i * (their relative scale), plus per
                  sample a_i * (Dw * Ew + Dh * Eh): Ew = |r_x| W + E(off_x) + 0.5 the scale of the pixel coordinate's terms, Dw / Dh a
                  Lipschitz bound of the zero-padded bilinear surface of the value around the sample
The forward is continuous in the location (a tap's weight reaches 0 where the bounds test or the zero padding removes it), and the
Lipschitz bound holds across a cell border and across the map's edge, so a sample whose cell differs between two evaluations is
covered by its location term: no output element is ever left out of a comparison.
dtype = float32 evaluates the same statement in fp32 on the CPU after the inputs: the yardstick k is measured with (never a kernel).

`wrong` selects a deliberately wrong variant of the statement (WRONG): tests/test_gsamp_ref_cpu.py shows that the cases of
tests/gsamp_cases.py tell each of them from the right one."""
import torch
import torch.nn.functional as TF

from tests import msda_ref as R

F32, F64 = torch.float32, torch.float64
M, P, D, NG = 8, 8, 32, 192


def _column_order():
    j = torch.arange(NG)
    g, w = j // 24, j % 24
    return torch.where(w < 16, 16 * g + w, 128 + 8 * g + (w - 16))


COLUMN_ORDER = _column_order()          # column j of G / xw holds row COLUMN_ORDER[j] of [sampling_offsets (128); attention_weights (64)]

WRONG = {
    "sample_clamp": "sampling: a corner outside the map reads the clamped pixel with its weight",
    "foot_clamp": "footprint: a corner outside the map reads the clamped pixel with its weight",
    "no_half_pixel": "sampling: the half-pixel shift of the pixel coordinate is dropped",
    "no_grid_clamp": "footprint: the clamp of 2 r - 1 to +-1.1 is dropped",
    "natural_view": "the natural (level, head) mapping replaces the viewed one",
    "ref_level0": "level 0's reference point is used on all levels",
    "first_footprint": "the footprint of a head's first level row is used for its second one",
    "xw_n_div_b": "xw is indexed by n / B instead of n % B",
    "softmax_per_level": "softmax over the P logits of a level instead of a head's L * P",
    "order_ignored": "the store ignores order: the row computed for pair order[s] lands on row s",
    "mask_by_slot": "pair_mask is indexed by the slot, not by the pair",
}


def natural(t):
    """columns from ops.gsamp_column_order() to the Linear's own order ([offsets (128) | logits (64)])."""
    out = torch.empty_like(t)
    out[..., COLUMN_ORDER] = t
    return out


def value_rows(value):
    """head planes (n_img, 8, S, 32) or row-major (n_img, S, 256) -> (n_img, S, 8, 32)."""
    if value.dim() == 4:
        return value.permute(0, 2, 1, 3).contiguous()
    return value.reshape(value.shape[0], value.shape[1], M, D)


def _lipschitz(mp):
    """mp (n, H, W, C) -> Dw, Dh (n, H + 5, W + 5, C), indexed [y0 + 3, x0 + 3] by a cell (y0, x0) with -3 <= y0 <= H + 1, -3 <= x0 <= W + 1:
    the largest |difference of horizontally (vertically) adjacent pixels| over the cell and its eight neighbours, padding counted as
    pixels of value 0.  Inside a cell d/dx of the bilinear surface is a convex combination of the horizontal differences of the cell's two
    rows, so |f(p) - f(p')| <= Dw |dx| + Dh |dy| for p' in the cell or a neighbouring one, the map's edge included."""
    pad = TF.pad(mp.permute(0, 3, 1, 2), (4, 4, 4, 4))
    dx = (pad[..., :, 1:] - pad[..., :, :-1]).abs()
    dy = (pad[..., 1:, :] - pad[..., :-1, :]).abs()
    Dw = TF.max_pool2d(dx, (4, 3), 1).permute(0, 2, 3, 1)
    Dh = TF.max_pool2d(dy, (3, 4), 1).permute(0, 2, 3, 1)
    return Dw, Dh


def _bilinear(mp, iy, ix, clamp_pad=False):
    """zero-padded bilinear taps of mp (n, H, W, C) at pixel coordinates iy, ix (n, Q) -> value, sum of |terms| (n, Q, C), y0, x0 (n, Q).
    clamp_pad (a WRONG variant): a corner outside the map reads the clamped pixel."""
    n, H, W, _ = mp.shape
    y0f, x0f = torch.floor(iy), torch.floor(ix)
    ty, tx = iy - y0f, ix - x0f
    y0, x0 = y0f.long(), x0f.long()
    nidx = torch.arange(n).view(n, 1)
    val, A = 0, 0
    for yy, xx, w in ((y0, x0, (1 - tx) * (1 - ty)), (y0, x0 + 1, tx * (1 - ty)), (y0 + 1, x0, (1 - tx) * ty), (y0 + 1, x0 + 1, tx * ty)):
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        g = mp[nidx, yy.clamp(0, H - 1), xx.clamp(0, W - 1)]
        if not clamp_pad:
            w = w * ok.to(w.dtype)
        val = val + w.unsqueeze(-1) * g
        A = A + w.abs().unsqueeze(-1) * g.abs()
    return val, A, y0, x0


def footprint_coordinates(ref_lvl, shapes, dtype=F64, grid_clamp=True):
    """ix, iy (n_img, Lq, L) pixel coordinates of the footprint on G, Ex, Ey their error scales, clamped (n_img, Lq, L, 2) bool (x, y)."""
    r = ref_lvl.to(dtype)
    Ws, Hs = shapes[:, 1].to(dtype), shapes[:, 0].to(dtype)
    g = r * 2.0 - 1.0
    clamped = (g < -1.1) | (g > 1.1)
    if grid_clamp:
        g = torch.clamp(g, -1.1, 1.1)
    ix, iy = ((g[..., 0] + 1) * Ws - 1) / 2, ((g[..., 1] + 1) * Hs - 1) / 2
    Ag = 2 * r.abs() + 2                                           # terms of (2 r - 1) + 1
    return ix, iy, (Ag[..., 0] * Ws + 1) / 2, (Ag[..., 1] * Hs + 1) / 2, clamped


def phase_a(G, xw, ref_lvl, shapes, starts, B, dtype=F64, wrong=None):
    """x, E (n_img, Lq, L, 192) in the Linear's natural column order: level row l = bilinear(G_l, footprint of r_l) + xw."""
    n_img, Lq, L, _ = ref_lvl.shape
    S = G.shape[0] // n_img
    Gn = natural(G.to(dtype)).view(n_img, S, NG)
    xn = natural(xw.to(dtype)).view(B, Lq, NG)
    b = torch.arange(n_img) % B
    if wrong == "xw_n_div_b":
        b = (torch.arange(n_img) // B).clamp_max(B - 1)
    xq = xn[b]                                                     # (n_img, Lq, 192)
    r = ref_lvl[:, :, :1].expand_as(ref_lvl) if wrong == "ref_level0" else ref_lvl
    ix, iy, Ex, Ey, _ = footprint_coordinates(r, shapes, dtype, grid_clamp=wrong != "no_grid_clamp")
    nidx = torch.arange(n_img).view(n_img, 1)
    rows, errs = [], []
    for l in range(L):
        H, W, st = int(shapes[l, 0]), int(shapes[l, 1]), int(starts[l])
        mp = Gn[:, st:st + H * W].view(n_img, H, W, NG)
        val, A, y0, x0 = _bilinear(mp, iy[:, :, l], ix[:, :, l], clamp_pad=wrong == "foot_clamp")
        Dw, Dh = _lipschitz(mp)
        yc, xc = y0.clamp(-3, H + 1) + 3, x0.clamp(-3, W + 1) + 3
        slope = Dw[nidx, yc, xc] * Ex[:, :, l].unsqueeze(-1) + Dh[nidx, yc, xc] * Ey[:, :, l].unsqueeze(-1)
        rows.append(val + xq)
        errs.append(A + xq.abs() + slope)
    x, E = torch.stack(rows, 2), torch.stack(errs, 2)
    if wrong == "first_footprint":                                 # head m's flat groups m L .. m L + L - 1; level row = group >> 3
        x, E = x.clone(), E.clone()
        for m in range(M):
            l_lo = (m * L) >> 3
            for fg in range(m * L, m * L + L):
                if (fg >> 3) != l_lo:
                    g = fg & 7
                    for cols in (slice(16 * g, 16 * g + 16), slice(128 + 8 * g, 128 + 8 * g + 8)):
                        x[:, :, fg >> 3, cols] = rows[l_lo][:, :, cols]
                        E[:, :, fg >> 3, cols] = errs[l_lo][:, :, cols]
    return x, E


def _view(x, L, wrong=None):
    """(n_img, Lq, L, 192) -> offsets (n_img, Lq, M, L, P, 2), logits (n_img, Lq, M, L * P): a VIEW of the rows' memory, not a transpose."""
    n_img, Lq = x.shape[:2]
    off, lg = x[..., :128].contiguous(), x[..., 128:].contiguous()
    if wrong == "natural_view":
        return off.view(n_img, Lq, L, M, P, 2).transpose(2, 3).contiguous(), lg.view(n_img, Lq, L, M, P).transpose(2, 3).reshape(n_img, Lq, M, L * P)
    return off.view(n_img, Lq, M, L, P, 2), lg.view(n_img, Lq, M, L * P)


def _tail(value, x, E, ref_lvl, shapes, starts, dtype, wrong):
    """the view, softmax, locations and sampling on the phase-A rows -> dict (see gsamp)."""
    n_img, Lq, L, _ = ref_lvl.shape
    value = value_rows(value).to(dtype)
    r = ref_lvl.to(dtype)
    if wrong == "ref_level0":
        r = r[:, :, :1].expand_as(r)
    off, lg = _view(x, L, wrong)
    E_off, E_lg = _view(E, L, wrong)
    if wrong == "softmax_per_level":
        lgl = lg.view(n_img, Lq, M, L, P)
        lse = torch.logsumexp(lgl, -1, keepdim=True).expand_as(lgl).reshape(n_img, Lq, M, L * P)
    else:
        lse = torch.logsumexp(lg, -1, keepdim=True)
    a = torch.exp(lg - lse)
    rel = 1 + E_lg + E_lg.amax(-1, keepdim=True) + (lg - lse).abs()
    a, rel = a.view(n_img, Lq, M, L, P), rel.view(n_img, Lq, M, L, P)
    WH = torch.stack([shapes[:, 1], shapes[:, 0]], -1).to(dtype)                       # (L, 2) as (W, H)
    loc = r[:, :, None, :, None, :] + off / WH[None, None, None, :, None, :]
    sloc = loc + 0.5 / WH[None, None, None, :, None, :] if wrong == "no_half_pixel" else loc
    form = "f64" if dtype == F64 else "plain"
    if wrong == "sample_clamp":
        res = _sample_clamped(value, shapes, starts, sloc, a)
    else:
        res = R.msda(value, shapes, starts, sloc, a, None, dtype, form)
    out, out_abs = res["out"], res["out_A"]
    out_A = R.msda(value, shapes, starts, sloc, a * rel, None, dtype, form)["out_A"].view(n_img, Lq, M, D)
    nidx = torch.arange(n_img).view(n_img, 1, 1, 1)
    midx = torch.arange(M).view(1, 1, M, 1)
    S = value.shape[1]
    h_all, w_all = R.coordinates(sloc, shapes, form)
    for l in range(L):
        H, W, st = int(shapes[l, 0]), int(shapes[l, 1]), int(starts[l])
        mp = value[:, st:st + H * W].reshape(n_img, H, W, M * D)
        Dw, Dh = _lipschitz(mp)
        Dw, Dh = Dw.view(n_img, H + 5, W + 5, M, D), Dh.view(n_img, H + 5, W + 5, M, D)
        yc = torch.floor(h_all[:, :, :, l]).clamp(-3, H + 1).long() + 3                # (n_img, Lq, M, P)
        xc = torch.floor(w_all[:, :, :, l]).clamp(-3, W + 1).long() + 3
        Ew = r[:, :, None, l, None, 0].abs() * W + E_off[:, :, :, l, :, 0] + 0.5
        Eh = r[:, :, None, l, None, 1].abs() * H + E_off[:, :, :, l, :, 1] + 0.5
        t = Dw[nidx, yc, xc, midx] * Ew.unsqueeze(-1) + Dh[nidx, yc, xc, midx] * Eh.unsqueeze(-1)     # (n_img, Lq, M, P, D)
        out_A = out_A + (a[:, :, :, l].unsqueeze(-1) * t).sum(3)
    return dict(out=out.reshape(n_img * Lq, M * D), out_abs=out_abs.reshape(n_img * Lq, M * D), out_A=out_A.reshape(n_img * Lq, M * D),
                x=x, x_E=E, offsets=off, logits=lg, weights=a, locations=loc, inside=res["inside"], h=h_all, w=w_all)


def _sample_clamped(value, shapes, starts, loc, wgt):
    """WRONG variant of the sampling: corners outside the map read the clamped pixel with their weight (the bounds test stays)."""
    n_img, S, _, _ = value.shape
    Lq, L = loc.shape[1], loc.shape[3]
    h_all, w_all = R.coordinates(loc, shapes, "f64" if loc.dtype == F64 else "plain")
    inside_all = R.anchors(h_all, w_all, shapes)[0]
    out = torch.zeros(n_img, Lq, M, D, dtype=value.dtype)
    for l in range(L):
        H, W, st = int(shapes[l, 0]), int(shapes[l, 1]), int(starts[l])
        for m in range(M):
            mp = value[:, st:st + H * W, m].reshape(n_img, H, W, D)
            v = _bilinear(mp, h_all[:, :, m, l].reshape(n_img, -1).to(value.dtype), w_all[:, :, m, l].reshape(n_img, -1).to(value.dtype), True)[0]
            a = (wgt[:, :, m, l] * inside_all[:, :, m, l].to(value.dtype)).unsqueeze(-1)
            out[:, :, m] += (a * v.view(n_img, Lq, P, D)).sum(2)
    return dict(out=out.reshape(n_img, Lq, M * D), out_A=out.abs().reshape(n_img, Lq, M * D), inside=inside_all)


def _rows(res, n_pairs, pair_mask, order, wrong):
    """what the launch leaves in samp: slot s works on pair order[s] (s itself without an order); a pair whose mask byte is 0 gets a row
    of zeros."""
    if pair_mask is None and order is None:
        return res
    slot = torch.arange(n_pairs)
    pair = slot if order is None else order.long()
    dst = slot if wrong == "order_ignored" else pair
    keep = torch.ones(n_pairs, dtype=torch.bool) if pair_mask is None else (pair_mask[slot if wrong == "mask_by_slot" else pair] != 0)
    for k in ("out", "out_abs", "out_A"):
        t = torch.zeros_like(res[k])
        t[dst] = res[k][pair] * keep.to(res[k].dtype).unsqueeze(-1)
        res[k] = t
    return res


def gsamp(value, G, xw, ref_lvl, shapes, starts, B, pair_mask=None, order=None, dtype=F64, wrong=None):
    """the fused operation on G and xw -> dict of `dtype` tensors: out, out_abs, out_A (n_img * Lq, 256) -- the sampled rows, the sum of
    the absolute values of their terms, their error scale in units of eps --, and the intermediates x, x_E (n_img, Lq, L, 192, natural
    columns), offsets, locations (n_img, Lq, M, L, P, 2), logits (n_img, Lq, M, L * P), weights, inside, h, w (n_img, Lq, M, L, P)."""
    assert wrong is None or wrong in WRONG
    n_img, Lq = ref_lvl.shape[:2]
    x, E = phase_a(G, xw, ref_lvl, shapes, starts, B, dtype, wrong)
    res = _tail(value, x, E, ref_lvl, shapes, starts, dtype, wrong)
    return _rows(res, n_img * Lq, pair_mask, order, wrong)


def fused(value, oa, ref_lvl, shapes, starts, dtype=F64, wrong=None):
    """the same from oa (pairs * L, 192), natural columns: the operation of msda_fused_kernel.  oa is an input: its error scale is |oa|."""
    n_img, Lq, L, _ = ref_lvl.shape
    x = oa.to(dtype).view(n_img, Lq, L, NG)
    return _tail(value, x, x.abs(), ref_lvl, shapes, starts, dtype, wrong)


def oa_of(G, xw, ref_lvl, shapes, starts, B):
    """oa (pairs * L, 192) fp32 of msda_fused from the G form's operands (phase A in fp64, rounded once)."""
    x, _ = phase_a(G, xw, ref_lvl, shapes, starts, B, F64)
    return x.reshape(-1, NG).float().contiguous()


def yardstick(ref64, ref32):
    """k = 4 x the largest |ref32 - ref64| / (2^-24 out_A) over the rows: how many eps * A the fp32 evaluation of the statement itself
    is off by.  It measures the reference, never a kernel."""
    A = ref64["out_A"]
    ratio = (ref32["out"].double() - ref64["out"]).abs() / (2.0 ** -24 * A)
    return 4.0 * float(ratio[A > 0].max()) if bool((A > 0).any()) else 0.0


def bar(ref, k, kind):
    """elementwise error bar of a kernel's output.  "f32": k * 2^-24 * out_A + 2 ulp of the value (the fp32 kernels).  "gsamp_bf16": that
    plus what msda_gsamp_kernel documents -- the blend weights (bilinear x attention) are rounded to bf16: 2^-8 * out_abs; the output is
    rounded to bf16: 2^-8 * |out| -- on a reference evaluated on the bf16 operands as stored.  "fused_bf16": the output rounding only."""
    b = k * 2.0 ** -24 * ref["out_A"] + 4.0 * 2.0 ** -24 * ref["out"].abs()
    if kind == "gsamp_bf16":
        b = b + 2.0 ** -8 * ref["out_abs"] + 2.0 ** -8 * ref["out"].abs()
    elif kind == "fused_bf16":
        b = b + 2.0 ** -8 * ref["out"].abs()
    else:
        assert kind == "f32"
    return b
