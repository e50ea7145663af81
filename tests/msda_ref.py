"""TEST INFRASTRUCTURE ONLY.  fp64 restatement of the multi-scale deformable sampling op, forward and backward, with the error scale
of every output element -- the reference that tests/test_msda_fp64.py holds the kernels of csrc/msda.hip and csrc/msda_bwd.hip to.
Built from the operation's definition and from oracle/msda_ref.c; pinned to the oracle, the C restatement and the golden vectors by
tests/test_msda_ref_oracle.py.

Coordinates follow the operation as the fp32 kernels compute it: h_im = ly * H - 0.5 and w_im = lx * W - 0.5 in fp32, the bounds test
with strict > and <, the cell by floorf, the fractional parts lh, lw as the exact differences h_im - floor(h_im), w_im - floor(w_im);
everything after that in `dtype`.  The library is built with -ffp-contract=fast, so the device evaluates ly * H - 0.5 as ONE fused
multiply-add and a CPU two roundings: `form` selects "fma" (float32(float64(ly) * H - 0.5): what the device computes), "plain" (two
fp32 roundings: what oracle/msda_ref.c computes) or "f64" (fp64 coordinates: the fp64 kernels, the oracle's autograd and the golden
gradients, which were all produced from loc.double()).  A sample is AMBIGUOUS if "fma" and "plain" disagree on its bounds test or on
its cell: its grad_loc flips between two one-sided derivatives, every other output is continuous across the flip.

For every output element the reference returns the value and A, the sum of the absolute values of its terms: an fp32 evaluation
in any order is within a few 2^-24 A of the value.  dtype = float32 evaluates the same statement in fp32 after the coordinates: the
yardstick the tests measure k with (never the kernel)."""
import torch

F32, F64 = torch.float32, torch.float64
FORMS = ("fma", "plain", "f64")


def coordinates(loc, shapes, form="fma"):
    """loc (N, Lq, M, L, P, 2) as (x, y) -> h_im, w_im (N, Lq, M, L, P): fp32 for "fma" / "plain", fp64 for "f64"."""
    assert form in FORMS
    L = loc.shape[3]
    Hs = shapes[:, 0].view(1, 1, 1, L, 1)
    Ws = shapes[:, 1].view(1, 1, 1, L, 1)
    lx, ly = loc[..., 0], loc[..., 1]
    if form == "plain":
        return ly.float() * Hs.float() - 0.5, lx.float() * Ws.float() - 0.5
    h, w = ly.double() * Hs.double() - 0.5, lx.double() * Ws.double() - 0.5
    return (h, w) if form == "f64" else (h.float(), w.float())


def anchors(h, w, shapes):
    """bounds test and cell of every sample: inside (bool), h_low, w_low (int64, 0 where not inside), lh, lw (fp64, exact)."""
    L = h.shape[3]
    Hs = shapes[:, 0].view(1, 1, 1, L, 1).to(h.dtype)
    Ws = shapes[:, 1].view(1, 1, 1, L, 1).to(h.dtype)
    inside = (h > -1) & (w > -1) & (h < Hs) & (w < Ws)                     # false for NaN
    h = torch.where(inside, h, torch.zeros_like(h))
    w = torch.where(inside, w, torch.zeros_like(w))
    hl, wl = torch.floor(h), torch.floor(w)
    return inside, hl.long(), wl.long(), (h - hl).double(), (w - wl).double()


def ambiguous(loc, shapes):
    """(N, Lq, M, L, P) bool: the fused and the two-rounding form of the coordinates disagree on the bounds test or on the cell."""
    a = anchors(*coordinates(loc, shapes, "fma"), shapes)
    b = anchors(*coordinates(loc, shapes, "plain"), shapes)
    return (a[0] != b[0]) | (a[0] & b[0] & ((a[1] != b[1]) | (a[2] != b[2])))


def bins(loc, shapes, M, T=8, form="fma"):
    """destination bin of every sample as csrc/msda_bwd.hip forms it ((level tile of T x T pixels of the upper-left corner) * M + head,
    -1 outside the map) and the number of tiles of all levels: (N, Lq, M, L, P) int64, T_total."""
    inside, hl, wl, _, _ = anchors(*coordinates(loc, shapes, form), shapes)
    L = loc.shape[3]
    tw = (shapes[:, 1] + T - 1) // T
    th = (shapes[:, 0] + T - 1) // T
    tile0 = torch.cat([tw.new_zeros(1), (tw * th).cumsum(0)])
    tile = tile0[:L].view(1, 1, 1, L, 1) + (hl.clamp_min(0) // T) * tw.view(1, 1, 1, L, 1) + wl.clamp_min(0) // T
    m = torch.arange(M).view(1, 1, M, 1, 1)
    return torch.where(inside, tile * M + m, torch.full_like(tile, -1)), int(tile0[L])


def msda(value, shapes, starts, loc, wgt, grad_out=None, dtype=F64, form="fma"):
    """value (N, S, M, D), shapes (L, 2) int64 (H, W), starts (L,), loc (N, Lq, M, L, P, 2), wgt (N, Lq, M, L, P), grad_out (N, Lq, M * D)
    or None.  Returns a dict of `dtype` tensors:
      out, out_A (N, Lq, M * D)                                                the forward and its error scale
      grad_value, grad_value_A (N, S, M, D), grad_value_cnt (N, S, M) int64    cnt: contributions (corners inside the map) per pixel, head
      grad_loc, grad_loc_A (N, Lq, M, L, P, 2), grad_attn, grad_attn_A (N, Lq, M, L, P)
      inside (N, Lq, M, L, P) bool."""
    N, S, M, D = value.shape
    _, Lq, _, L, P, _ = loc.shape
    value = value.to(dtype)
    h_all, w_all = coordinates(loc, shapes, form)
    inside_all, hl_all, wl_all, lh_all, lw_all = anchors(h_all, w_all, shapes)
    res = {"inside": inside_all, "out": torch.zeros(N, Lq, M, D, dtype=dtype), "out_A": torch.zeros(N, Lq, M, D, dtype=dtype)}
    bwd = grad_out is not None
    if bwd:
        go = grad_out.to(dtype).view(N, Lq, M, 1, D)
        for k, shp in (("grad_value", (N * S * M, D)), ("grad_loc", (N, Lq, M, L, P, 2)), ("grad_attn", (N, Lq, M, L, P))):
            res[k] = torch.zeros(shp, dtype=dtype)
            res[k + "_A"] = torch.zeros(shp, dtype=dtype)
        res["grad_value_cnt"] = torch.zeros(N * S * M, dtype=torch.int64)
    bidx = torch.arange(N).view(N, 1, 1, 1)
    midx = torch.arange(M).view(1, 1, M, 1)
    for l in range(L):
        H, W, start = int(shapes[l, 0]), int(shapes[l, 1]), int(starts[l])
        inside, hl, wl = inside_all[:, :, :, l], hl_all[:, :, :, l], wl_all[:, :, :, l]
        lh, lw = lh_all[:, :, :, l].to(dtype), lw_all[:, :, :, l].to(dtype)
        hh, hw = 1 - lh, 1 - lw
        aw = wgt[:, :, :, l].to(dtype)
        cws = (hh * hw, hh * lw, lh * hw, lh * lw)
        v, oks, rows = [], [], []
        for hi, wi in ((hl, wl), (hl, wl + 1), (hl + 1, wl), (hl + 1, wl + 1)):
            ok = inside & (hi >= 0) & (hi <= H - 1) & (wi >= 0) & (wi <= W - 1)
            idx = start + hi.clamp(0, H - 1) * W + wi.clamp(0, W - 1)                       # (N, Lq, M, P)
            v.append(value[bidx, idx, midx] * ok.to(dtype).unsqueeze(-1))                   # (N, Lq, M, P, D), 0 outside the map
            oks.append(ok)
            rows.append((bidx * S + idx) * M + midx)
        samp = sum(c.unsqueeze(-1) * x for c, x in zip(cws, v))
        samp_A = sum(c.unsqueeze(-1) * x.abs() for c, x in zip(cws, v))
        res["out"] += (aw.unsqueeze(-1) * samp).sum(3)
        res["out_A"] += (aw.abs().unsqueeze(-1) * samp_A).sum(3)
        if not bwd:
            continue
        top = go * aw.unsqueeze(-1)                                                           # (N, Lq, M, P, D)
        res["grad_attn"][:, :, :, l] = (go * samp).sum(-1)
        res["grad_attn_A"][:, :, :, l] = (go.abs() * samp_A).sum(-1)
        dw = hh.unsqueeze(-1) * (v[1] - v[0]) + lh.unsqueeze(-1) * (v[3] - v[2])
        dh = hw.unsqueeze(-1) * (v[2] - v[0]) + lw.unsqueeze(-1) * (v[3] - v[1])
        dw_A = hh.unsqueeze(-1) * (v[1] - v[0]).abs() + lh.unsqueeze(-1) * (v[3] - v[2]).abs()
        dh_A = hw.unsqueeze(-1) * (v[2] - v[0]).abs() + lw.unsqueeze(-1) * (v[3] - v[1]).abs()
        res["grad_loc"][:, :, :, l, :, 0] = (dw * top).sum(-1) * W
        res["grad_loc"][:, :, :, l, :, 1] = (dh * top).sum(-1) * H
        res["grad_loc_A"][:, :, :, l, :, 0] = (dw_A * top.abs()).sum(-1) * W
        res["grad_loc_A"][:, :, :, l, :, 1] = (dh_A * top.abs()).sum(-1) * H
        for c, ok, row in zip(cws, oks, rows):
            r = row[ok]
            t = (c.unsqueeze(-1) * top)[ok]                                                   # (K, D)
            res["grad_value"].index_add_(0, r, t)
            res["grad_value_A"].index_add_(0, r, t.abs())
            res["grad_value_cnt"].index_add_(0, r, torch.ones_like(r))
    res["out"] = res["out"].reshape(N, Lq, M * D)
    res["out_A"] = res["out_A"].reshape(N, Lq, M * D)
    if bwd:
        res["grad_value"] = res["grad_value"].view(N, S, M, D)
        res["grad_value_A"] = res["grad_value_A"].view(N, S, M, D)
        res["grad_value_cnt"] = res["grad_value_cnt"].view(N, S, M)
    return res
