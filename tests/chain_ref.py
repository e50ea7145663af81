"""fp64 statements of the fused Linear chains (csrc/chain.hip) and of the unfused layer-tail kernels (csrc/geom.hip), with the
bf16 roundings of the kernels as an option, and first-order error bounds that say how far a kernel may be from them.

Not a test module: tests/test_chain_ref_oracle.py pins these helpers (rounding off) to oracle/decoder_ref.py, and
tests/test_chains_fp64.py holds the kernels to them.  Weights are plain (N, K) matrices; a test swizzles them for the kernels.

Rounding points (what `bf16=True` rounds, read off the kernels):
  chain A  attn (stored bf16, write_act_pre), h0 (write_act_pre), h1 (write_act); the last layer runs in fp32 on bf16 h1.
  chain B  the view mean (the GEMM operand), t1 as the FFN operand (the fp32 t1 stays the residual), the FFN hidden chunk
           (hbuf, write_act_pre) and tgt' + query_pos as the operand of the next layer's query-term GEMM.

Error bounds ("err" entries) are elementwise, first order and probabilistic in the sense of Higham & Mary (SIAM J. Sci.
Comput. 41, 2019): rounding errors are independent and of either sign, so the helpers below carry the typical size (root
mean square) of every error through the chain -- a sum of K of them grows like sqrt(K) -- and the returned bounds are LAMBDA
times that size (a sum of independent terms leaves LAMBDA sqrt(sum e_i^2) with probability <= 2 exp(-LAMBDA^2 / 2), 3e-14 at
LAMBDA = 8).  The worst-case bound K u sum|terms| is not used: pushed through a 1024-wide FFN and two LayerNorms it grows
past the values themselves.  The pieces (all typical sizes):
  lin_err   an fp32 dot product of K terms, u sqrt(K) sqrt(sum (w x)^2) plus the rounding of the result, and an input error
            e (independent per element) through the Linear, sqrt(W^2 e^2) (prop);
  round_err a bf16 rounding point: zero unless the interval the kernel's fp32 input may lie in straddles a rounding
            boundary, else one bf16 step (a flip), weighted by the probability of the flip when it goes on through a Linear;
  ln_err    LayerNorm's first-order derivative d x_hat = (e - mean e) / sigma - x_hat mean(x_hat e) / sigma, plus the fp32
            arithmetic of the kernels' LayerNorm carried as input error.
Tests compare with the returned bounds as they are and print max |err| / bound; a test that uses lin_err / ln_err directly
multiplies by LAMBDA itself.

The fp32 kernels on two-part fp16 operands (csrc/f32s.hip, "f32h": pyramid_f32h, chain_a_f32h, chain_b_f32h below).  The truth
is the plain fp64 operation with NO operand rounding; the bound says how far a kernel that forms every product as
  x 2^s = h + l,  h = fp16(x 2^s),  l = fp16(x 2^s - h)   (split_h2; s = row_scale of the row maximum, one s per weight tensor),
  a w ~ 2^-(s_a + s_w) (l_a h_w + h_a l_w + h_a h_w),      fp32 accumulation of the 3 K terms, exact ldexpf, + bias
may be from it.  The constants come from the fp16 format (11 significand bits, normal down to 2^-14, subnormal spacing 2^-24):
  H2_LL   2^-22 |a w|: the dropped l_a l_w (|l| <= 2^-11 |x 2^s|: half a unit in the last place of h);
  H2_PART 2^-23 |x|:   x 2^s - h - l, half a unit in the last place of l (|l| < 2^-11 |h|'s binade);
  H2_SUB  2^-24 2^-s:  where x 2^s - h falls into fp16's subnormal range (entries under 2^-16 of the maximum) the rounding of l
          is absolute, half the subnormal spacing 2^-25 in scaled units -- times 2 because the kernel takes s from the maximum of
          ITS row, which may sit in the binade under the reference's (the reference takes s from max (|x| + dx)).  With
          2^-s <= 2^-13 max|row| this is 2^-37 of the row / tensor maximum; for rows under 2^-87 (s capped at 100) it is 2^-124.
Where worst case, where typical size: H2_LL / H2_PART / H2_SUB are WORST-case sizes of one product term's error; the K terms of
a dot product are combined as independent errors (root sum of squares, lin_err_h2), times LAMBDA.  No sqrt(K) averaging is assumed
for a row: a heavy-tailed row, whose sum is one term, gets that term's worst case times LAMBDA.  The fp32 accumulation is
lin_err's, over 3 K + 1 terms.  Rounding points of the chains (the errors carried on through prop / ln_err):
  chain A  the planes of samp, of h0 and of h1 (re-split after ReLU, s from the row maximum over the eight wavefronts' partial
           maxima); attn is stored as the exact fp32 stage result; the 3-output layer runs in fp32 on the fp32 h1.
  chain B  the planes of the view mean (fp32 sum over the views in order, divided by (float)V); the planes of t1 as the FFN operand
           (the fp32 t1 stays the residual); the planes of each 256-column hidden chunk with a row scale of its own, the four
           chunk results added in fp32; the planes of tgt' + query_pos for the next layer's term.  LayerNorms, sigmoid and the
           joint mean as in chain_b.
"""
import torch

U32 = 2.0 ** -24          # fp32 unit roundoff
LN_EPS = 1e-5
LAMBDA = 8.0
H2_LL, H2_PART, H2_SUB = 2.0 ** -22, 2.0 ** -23, 2.0 ** -24      # two-part fp16 operands, see the module notes


def bf(x, on=True):
    """round to bf16 (nearest even), back in the tensor's dtype."""
    return x.to(torch.bfloat16).to(x.dtype) if on else x


def round_err(x, d, on=True, rms=True):
    """a kernel rounds to bf16 a value within d of the reference's unrounded x; the reference rounds x.  rms=False: the largest
    possible |bf(x') - bf(x)| (one bf16 step where [x - d, x + d] straddles a rounding boundary, else 0).  rms=True: that step
    times sqrt(min(1, 2 d / step)) -- the root mean square of a flip that happens with probability ~ 2 d / step -- the size
    `prop` takes for an error that goes on through a Linear (a flip everywhere d reaches a boundary would make every later
    rounding point flip in the bound, and the bound of a 1024-wide FFN exceed its values)."""
    if not on:
        return d
    r = bf(x)
    step = torch.maximum((bf(x + d) - r).abs(), (bf(x - d) - r).abs())
    if not rms:
        return step
    # x within d (a typical error) of a boundary -- above all the exact ties that means of bf16 values often are -- flips with
    # a probability the distance does not bound: a full step there
    tie = (bf(x + d) != r) | (bf(x - d) != r)
    return torch.where(tie, step, step * torch.sqrt(torch.clamp(2 * d / step.clamp_min(1e-300), max=1.0)))


def lin(x, W, b=None):
    x = x.double()
    y = x @ W.double().t()
    return y if b is None else y + b.double()


def lin_abs(x, W, b=None):
    y = x.double().abs() @ W.double().abs().t()
    return y if b is None else y + b.double().abs()


def prop(dx, W):
    """an input error bounded by dx (independent per element) through x W^T."""
    return torch.sqrt((dx.double() ** 2) @ (W.double() ** 2).t())


def lin_err(x, dx, W, b=None):
    """error of an fp32-accumulated  x W^T + b  whose input is off by at most dx (None: exact input)."""
    K = W.shape[1]
    x = x.double()
    sq = (x ** 2) @ (W.double() ** 2).t() + (0 if b is None else b.double() ** 2)
    e = U32 * (K + 1) ** 0.5 * torch.sqrt(sq) + U32 * lin(x, W, b).abs()
    return e if dx is None else e + prop(dx, W)


def ln(x, g, b, eps=LN_EPS):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g.double() + b.double()


def ln_err(x, dx, g, eps=LN_EPS):
    """bound on |LN_fp32(x') - LN(x)| (no affine shift error) for |x' - x| <= dx, see the module notes."""
    C = x.shape[-1]
    mu = x.mean(-1, keepdim=True)
    sig = torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + eps)
    xh = (x - mu) / sig
    mean_of = lambda t: torch.sqrt((t ** 2).mean(-1, keepdim=True) / C)     # the mean of C independent errors of sizes t
    d = dx + U32 * C ** 0.5 * x.abs().mean(-1, keepdim=True) + U32 * (x - mu).abs()
    dxh = (d + mean_of(d) + xh.abs() * mean_of(xh * d)) / sig + xh.abs() * (U32 * C ** 0.5 + 4 * U32)
    return g.double().abs() * dxh + 2 * U32 * (xh * g.double()).abs()


def chain_a(samp, inside, Wp, bp, W0, b0, W1, b1, W2, b2, bf16=False, attn=None):
    """chain A per row: attn = inside (samp Wp^T + bp), o = W2 relu(W1 relu(W0 attn + b0) + b1) + b2.
    attn: the stored attention rows to run the pose MLP on (e.g. a kernel's own, already checked); default: this function's.
    Returns dict(attn_exact, attn, h0, h1, o) and, with bf16, the bounds attn_err (of attn_exact's fp32 sum) and o_err."""
    keep = inside.double().view(-1, 1) != 0
    a_exact = torch.where(keep, lin(samp, Wp, bp), torch.zeros((), dtype=torch.float64, device=samp.device))
    a = bf(a_exact, bf16) if attn is None else attn.double()
    h0 = bf(torch.relu(lin(a, W0, b0)), bf16)
    h1 = bf(torch.relu(lin(h0, W1, b1)), bf16)
    o = lin(h1, W2, b2)
    out = dict(attn_exact=a_exact, attn=a, h0=h0, h1=h1, o=o)
    if bf16:
        out["attn_err"] = torch.where(keep, LAMBDA * lin_err(samp, None, Wp, bp), torch.zeros((), dtype=torch.float64, device=samp.device))
        e0 = round_err(torch.relu(lin(a, W0, b0)), lin_err(a, None, W0, b0))
        e1 = round_err(torch.relu(lin(h0, W1, b1)), lin_err(h0, e0, W1, b1))
        out["o_err"] = LAMBDA * lin_err(h1, e1, W2, b2)
    return out


def chain_b(attn, tgt, Wu, bu, g2, be2, W1, b1, W2, b2, g3, be3, Wc, bc, threshold, J, has_ffn=True, forced=None,
            qpos=None, Wn=None, bn=None, n_next=0, bf16=False):
    """chain B per joint token: attn (V, rows, 256) -> mean over views, t1 = LN2(tgt + Wu mean + bu),
    tgt' = LN3(t1 + W2 relu(W1 t1 + b1) + b2) (t1 when has_ffn is off), prob = mean_j sigmoid(Wc tgt' + bc) per person of
    J tokens, valid = prob[:, 1] > threshold or `forced`; with Wn: xw = (tgt' + qpos) Wn^T + bn, first n_next columns.
    Returns dict(mean, t1, tgt, prob, valid[, xw]) and, with bf16, the bounds tgt_err, prob_err[, xw_err]."""
    V = attn.shape[0]
    a = attn.double()
    tg = tgt.double()
    m_exact = a.mean(0)
    m = bf(m_exact, bf16)
    u = tg + lin(m, Wu, bu)
    t1 = ln(u, g2, be2)
    if has_ffn:
        t1b = bf(t1, bf16)
        hid = bf(torch.relu(lin(t1b, W1, b1)), bf16)
        y = t1 + lin(hid, W2, b2)
        t = ln(y, g3, be3)
    else:
        t = t1
    logit = lin(t, Wc, bc)
    sg = torch.sigmoid(logit)
    prob = sg.view(-1, J, 2).mean(1)
    valid = (forced != 0) if forced is not None else prob[:, 1] > threshold
    out = dict(mean=m, t1=t1, tgt=t, prob=prob, valid=valid)
    if Wn is not None:
        xb = bf(t + (0 if qpos is None else qpos.double()), bf16)
        out["xw"] = lin(xb, Wn, bn)[:, :n_next]
    if bf16:
        dm = (V + 2) * U32 * a.abs().mean(0)                       # fp32 sum over the views, times the fp32 1 / V (worst case)
        em = round_err(m_exact, dm)
        eu = lin_err(m, em, Wu, bu) + U32 * (tg.abs() + u.abs())
        et1 = ln_err(u, eu, g2)
        if has_ffn:
            e1b = round_err(t1, et1)
            eh = round_err(torch.relu(lin(t1b, W1, b1)), lin_err(t1b, e1b, W1, b1))
            ey = et1 + lin_err(hid, eh, W2, b2) + U32 * (t1.abs() + y.abs())
            et = ln_err(y, ey, g3)
        else:
            et = et1
        el = lin_err(t, et, Wc, bc)
        es = (sg * (1 - sg) + el).clamp(max=0.25) * el + 4 * U32 * sg     # sigmoid' <= 1/4, expf and the division
        out["tgt_err"] = LAMBDA * et
        out["prob_err"] = LAMBDA * (es.view(-1, J, 2).mean(1) + (J + 1) * U32 * prob)
        if Wn is not None:
            x = t + (0 if qpos is None else qpos.double())
            exb = round_err(x, et + U32 * x.abs())
            out["xw_err"] = LAMBDA * lin_err(xb, exb, Wn, bn)[:, :n_next]
    return out


# ------------------------------------------------------------------------------------- two-part fp16 operands (csrc/f32s.hip)
def row_scale(m):
    """f32s_dev.h::row_scale: min(13 - exponent(m), 100) from the fp32 bit pattern of m >= 0 (zero / subnormal maxima: 100)."""
    e = ((m.float().contiguous().view(torch.int32) >> 23) & 0xFF) - 127
    return torch.clamp(13 - e, max=100)


def weight_scale(W):
    """the tensor scale ops.split_swizzle_weight_h2 returns: row_scale of max |W| within [-100, 100]; 0 for a zero / non-finite maximum."""
    m = W.detach().float().abs().max()
    if not (bool(m > 0) and bool(torch.isfinite(m))):
        return 0
    return int(row_scale(m).clamp(min=-100))


def split_h2(x, s):
    """(h, l) as f32s_dev.h::split4_h2 and ops.split_swizzle_weight_h2 form them: fp16(x 2^s) and fp16(x 2^s - h), fp32 arithmetic.
    s: int or an integer tensor that broadcasts against x."""
    xs = torch.ldexp(x.float(), torch.as_tensor(s, device=x.device))
    h = xs.to(torch.float16)
    return h, (xs - h.float()).to(torch.float16)


def lin_err_h2(x, dx, W, b=None, w_scale=None):
    """typical size of the error of  x W^T + b  formed on two-part fp16 operands with fp32 accumulation (module notes), the
    input off by at most dx (None: exact).  w_scale: the scale of the tensor W is a block of (default: W's own)."""
    K = W.shape[1]
    x, Wd = x.double(), W.double()
    ax, aW = x.abs(), Wd.abs()
    sq = (x ** 2) @ (Wd ** 2).t()
    acc = U32 * (3 * K + 1) ** 0.5 * torch.sqrt(sq + (0 if b is None else b.double() ** 2)) + U32 * lin(x, W, b).abs()
    m = (ax if dx is None else ax + dx.double()).amax(-1, keepdim=True)
    qx = H2_SUB * torch.ldexp(torch.ones_like(m), -row_scale(m).double())               # absolute part of an activation entry
    qw = H2_SUB * 2.0 ** -(weight_scale(W) if w_scale is None else w_scale)              # ... of a weight entry
    c = H2_LL + 2 * H2_PART
    # sum over k of (c |x w| + qx |w| + |x| qw)^2, expanded
    op2 = (c * c * sq + qx ** 2 * (Wd ** 2).sum(1) + qw ** 2 * (x ** 2).sum(-1, keepdim=True)
           + 2 * c * qx * (ax @ (Wd ** 2).t()) + 2 * c * qw * ((x ** 2) @ aW.t()) + 2 * qx * qw * (ax @ aW.t()))
    e = acc + torch.sqrt(op2)
    return e if dx is None else e + prop(dx, W)


def pyramid_f32h(feat, Wv, bv, Wg):
    """value = feat Wv^T + bv, G = feat Wg^T (fp64) and the bounds of mvg_pyramid_f32h: dict(value, G, value_err, G_err)."""
    return dict(value=lin(feat, Wv, bv), G=lin(feat, Wg), value_err=LAMBDA * lin_err_h2(feat, None, Wv, bv),
                G_err=LAMBDA * lin_err_h2(feat, None, Wg))


def chain_a_f32h(samp, inside, Wp, bp, W0, b0, W1, b1, W2, b2, bounds=True):
    """chain A in fp64 (chain_a, no rounding) with the bounds of mvg_chain_attn_pose_f32h: attn_err, o_err."""
    out = chain_a(samp, inside, Wp, bp, W0, b0, W1, b1, W2, b2)
    if bounds:
        keep = inside.double().view(-1, 1) != 0
        ea = torch.where(keep, lin_err_h2(samp, None, Wp, bp), torch.zeros((), dtype=torch.float64, device=samp.device))
        e0 = lin_err_h2(out["attn"], ea, W0, b0)                   # ReLU does not enlarge an error
        e1 = lin_err_h2(out["h0"], e0, W1, b1)
        out["attn_err"] = LAMBDA * ea
        out["o_err"] = LAMBDA * lin_err(out["h1"], e1, W2, b2)
    return out


def chain_b_f32h(attn, tgt, Wu, bu, g2, be2, W1, b1, W2, b2, g3, be3, Wc, bc, threshold, J, has_ffn=True, forced=None,
                 qpos=None, Wn=None, bn=None, n_next=0, bounds=True):
    """chain B in fp64 (chain_b, no rounding) with the bounds of mvg_chain_update_ffn_class_f32h: tgt_err, prob_err[, xw_err]."""
    out = chain_b(attn, tgt, Wu, bu, g2, be2, W1, b1, W2, b2, g3, be3, Wc, bc, threshold, J, has_ffn=has_ffn, forced=forced,
                  qpos=qpos, Wn=Wn, bn=bn, n_next=n_next)
    if not bounds:
        return out
    V = attn.shape[0]
    a, tg = attn.double(), tgt.double()
    m, t1, t = out["mean"], out["t1"], out["tgt"]
    dm = (V + 2) * U32 * a.abs().mean(0)
    u = tg + lin(m, Wu, bu)
    et1 = ln_err(u, lin_err_h2(m, dm, Wu, bu) + U32 * (tg.abs() + u.abs()), g2)
    if has_ffn:
        hid = torch.relu(lin(t1, W1, b1))
        eh = lin_err_h2(t1, et1, W1, b1)
        s2 = weight_scale(W2)
        e2sq, part = 0, 0
        for c in range(0, W2.shape[1], 256):                        # one row scale per 256-column chunk, the results added in fp32
            e2sq = e2sq + lin_err_h2(hid[:, c:c + 256], eh[:, c:c + 256], W2[:, c:c + 256], None, w_scale=s2) ** 2
            part = part + lin(hid[:, c:c + 256], W2[:, c:c + 256]).abs()
        y = t1 + lin(hid, W2, b2)
        ey = et1 + torch.sqrt(e2sq) + U32 * (part + (y - t1).abs() + t1.abs() + y.abs())
        et = ln_err(y, ey, g3)
    else:
        et = et1
    sg = torch.sigmoid(lin(t, Wc, bc))
    el = lin_err(t, et, Wc, bc)
    es = (sg * (1 - sg) + el).clamp(max=0.25) * el + 4 * U32 * sg
    out["tgt_err"] = LAMBDA * et
    # the J rows of a person carry independent errors (each row its own operand roundings and sums): root sum of squares / J
    out["prob_err"] = LAMBDA * (torch.sqrt((es ** 2).view(-1, J, 2).sum(1)) / J + (J + 1) * U32 * out["prob"])
    if Wn is not None:
        x = t + (0 if qpos is None else qpos.double())
        out["xw_err"] = LAMBDA * lin_err_h2(x, et + U32 * x.abs(), Wn, bn)[:, :n_next]
    return out
