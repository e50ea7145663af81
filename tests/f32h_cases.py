"""Inputs, case tables and a CPU emulation for the tests of the fp32 kernels on two-part fp16 operands (csrc/f32s.hip).
Not a test module: tests/test_f32h_ref_cpu.py checks the bounds of tests/chain_ref.py against the emulation and the case
tables against the ambiguity condition; tests/test_f32h_fp64.py runs the same cases on the device.  Everything here is made on
the CPU from seeded generators, so both files see the same numbers."""
import torch

from tests import chain_ref as R


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def mk_w(gen, n, k, wmul=1.0, bmul=0.1):
    return torch.randn(n, k, generator=gen) / k ** 0.5 * wmul, torch.randn(n, generator=gen) * bmul


def chain_a_weights(seed=7, wmul=(1.0, 1.0, 1.0)):
    """plain fp32 weights of chain A; wmul scales Wp / W0 / W1 (their biases with them)."""
    gen = _gen(seed)
    W = {}
    for name, bias, m in (("Wp", "bp", wmul[0]), ("W0", "b0", wmul[1]), ("W1", "b1", wmul[2])):
        W[name], W[bias] = mk_w(gen, 256, 256, m, 0.1 * m)
    W["W2"], W["b2"] = mk_w(gen, 3, 256, 1.0, 1.0)
    return W


A_KEYS = ("Wp", "bp", "W0", "b0", "W1", "b1", "W2", "b2")


def chain_b_weights(seed=11, variant=None):
    """variant "chunks": hidden chunk 0 entirely zero and chunk 1 large for every row (the per-chunk row scale)."""
    gen = _gen(seed)
    W = {}
    for name, bias, n, k in (("Wu", "bu", 256, 256), ("W1", "b1", 1024, 256), ("W2", "b2", 256, 1024), ("Wn", "bn", 256, 256)):
        W[name], W[bias] = mk_w(gen, n, k)
    W["Wc"], W["bc"] = mk_w(gen, 2, 256, 1.0, 1.0)
    for g, b in (("g2", "be2"), ("g3", "be3")):
        W[g], W[b] = 1 + 0.1 * torch.randn(256, generator=gen), 0.1 * torch.randn(256, generator=gen)
    if variant == "chunks":
        W["b1"][:256] = -1e3
        W["b1"][256:512] = 50.0
    return W


B_KEYS = ("Wu", "bu", "g2", "be2", "W1", "b1", "W2", "b2", "g3", "be3", "Wc", "bc")


# ---------------------------------------------------------------------------------------------------------------- operand rows
def operand_rows(kind, rows, seed):
    """(rows, 256) fp32 rows at the edges of the operand split."""
    gen = _gen(seed)
    x = torch.randn(rows, 256, generator=gen)
    if kind == "randn":
        return x
    if kind == "rows_12_decades":                    # 1e-6 .. 1e6 row by row
        return x * 10.0 ** torch.linspace(-6, 6, rows)[:, None]
    if kind == "rows_1e-30_1e30":
        return x * 10.0 ** torch.linspace(-30, 30, rows)[:, None]
    if kind == "entries_6_decades":                  # heavy-tailed rows: no averaging over k
        return x * 10.0 ** (6 * torch.rand(rows, 256, generator=gen) - 3)
    if kind == "zero_rows":
        x[::3] = 0
        return x
    if kind == "max_under_2^14":                     # the row maximum's mantissa just under 2: the scaled maximum just under 2^14
        e = torch.randint(-20, 20, (rows,), generator=gen)
        x = x.clamp(-1.9, 1.9)
        x[torch.arange(rows), torch.randint(0, 256, (rows,), generator=gen)] = torch.nextafter(torch.tensor(2.0), torch.tensor(0.0))
        return torch.ldexp(x, e[:, None])
    raise KeyError(kind)


OPERAND_KINDS = ("randn", "rows_12_decades", "entries_6_decades", "zero_rows", "max_under_2^14")


# --------------------------------------------------------------------------------------------------------------------- chain B
_NEXT = [None, ("q", 32), (None, 64), ("q", 192), ("q", 256), (None, 192)]
_VS = (1, 2, 3, 4, 5, 8, 31)


def _b_cases():
    """(B, NQ, J, V): B * NQ one below, at and one above two tiles' persons for both tile sizes (32 // J and 64 // J persons)."""
    out, k = [], 0
    for J in (1, 2, 14, 15, 16, 17, 21, 31, 32):
        nqs = sorted({m + d for m in (2 * (32 // J), 2 * (64 // J)) for d in (-1, 0, 1)})
        for nq in nqs:
            B = 2 if nq % 2 == 0 and k % 2 == 0 else 1
            out.append((B, nq // B, J, _VS[k % len(_VS)]))
            k += 1
    return out


B_CASES = _b_cases()


def b_edge_cases(cus):
    """name -> (inputs, weight variant, has_ffn) of the chain B cases outside the table: both sides of the tile-size switch
    (J = 15: 64-row tiles start at ceil(B NQ / 4) > 3 CUs / 4), LayerNorm edge rows, operand edges."""
    out = {}
    for above in (0, 1):
        nq = 4 * ((cus * 3) // 4 + above)
        out["switch_%d" % above] = (chain_b_inputs(2, nq // 2, 15, 2, seed=77 + above, nxt=("q", 192)), None, True)
    for has_ffn in (0, 1):
        out["ln_edges_ffn%d" % has_ffn] = (chain_b_inputs(2, 9, 15, 3, seed=5, nxt=("q", 192), ln_edges=True), None, bool(has_ffn))
    out["operands"] = (chain_b_inputs(1, 9, 15, 3, seed=8, nxt=("q", 256), edges="operands"), None, True)
    out["chunks"] = (chain_b_inputs(1, 9, 15, 3, seed=8, nxt=("q", 256)), "chunks", True)
    return out


B_EDGE_NAMES = ("switch_0", "switch_1", "ln_edges_ffn0", "ln_edges_ffn1", "operands", "chunks")


def b_options(k):
    """the options that cycle over the cases: has_ffn, forced_valid, any_valid's initial value, (qpos, n_next)."""
    return dict(has_ffn=k % 3 != 2, forced=k % 5 == 3, any0=int(k % 7 == 1), nxt=_NEXT[k % len(_NEXT)])


def chain_b_inputs(B, NQ, J, V, seed, nxt=None, forced=False, ln_edges=False, edges=None):
    """attn (V, rows, 256), tgt, qpos / n_next, forced_valid of one case (CPU tensors).  ln_edges: the four LayerNorm row kinds of
    tests/test_chains_fp64.py::_chain_b_case.  edges "operands": view rows over 12 decades, tgt rows at 1e-20 and 1e4."""
    gen = _gen(seed)
    rows, nq = B * NQ * J, B * NQ
    attn = torch.randn(V, rows, 256, generator=gen)
    tgt = torch.randn(rows, 256, generator=gen)
    bu = chain_b_weights()["bu"]
    if ln_edges:
        n = min(rows, 4 * J)
        attn[:, :n] = 0
        tgt[: n // 4] = 1e3 + tgt[: n // 4]
        tgt[n // 4: n // 2] = 0.25 - bu + 1e-3 * tgt[n // 4: n // 2]            # variance ~ 1e-6 (< eps)
        tgt[n // 2: 3 * n // 4] = -1.5 - bu + 3e-3 * tgt[n // 2: 3 * n // 4]    # ~ 1e-5 (= eps)
        tgt[3 * n // 4: n] = 0.5 - bu                                             # ~ 0
    if edges == "operands":
        attn = attn * 10.0 ** torch.linspace(-6, 6, V * rows).view(rows, V).t()[:, :, None]
        tgt[0::5] *= 1e-20
        tgt[1::5] *= 1e4
    qpos, n_next = (None, 0) if nxt is None else ((None if nxt[0] is None else torch.randn(rows, 256, generator=gen)), nxt[1])
    fv = (torch.rand(nq, generator=gen) < 0.5).to(torch.uint8) if forced else None
    return dict(attn=attn, tgt=tgt, qpos=qpos, n_next=n_next, forced=fv, B=B, NQ=NQ, J=J, V=V)


def chain_b_ref(c, W, has_ffn=True, thr=None):
    """fp64 statement and bounds of a case (on the case's device).  thr None: the threshold is put into the widest gap between
    the persons' fp64 prob_1 next to the median, so that persons fall on both sides and none is near it."""
    dev = c["attn"].device
    Wd = {k: v.to(dev) for k, v in W.items()}
    n = c["n_next"]

    def run(t):
        return R.chain_b_f32h(c["attn"], c["tgt"], *[Wd[k] for k in B_KEYS], t, c["J"], has_ffn=has_ffn, forced=c["forced"],
                              qpos=c["qpos"], Wn=Wd["Wn"][:n] if n else None, bn=Wd["bn"][:n] if n else None, n_next=n)
    ref = run(0.5 if thr is None else thr)
    if thr is None:
        p1 = ref["prob"][:, 1].sort().values
        if p1.numel() == 1:
            thr = float(p1[0]) - 0.01
        else:
            cand = range(max(0, p1.numel() // 2 - 2), min(p1.numel() - 1, p1.numel() // 2 + 1))
            i = max(cand, key=lambda j: float(p1[j + 1] - p1[j]))
            thr = float((p1[i] + p1[i + 1]) / 2)
        thr = float(torch.tensor(thr, dtype=torch.float32))         # the kernel takes a float
        if c["forced"] is None:
            ref["valid"] = ref["prob"][:, 1] > thr
    ref["thr"] = thr
    # the persons whose fp64 prob_1 lies within its bound of the threshold: must be none
    ref["ambiguous"] = (ref["prob"][:, 1] - thr).abs() <= ref["prob_err"][:, 1]
    return ref


# ------------------------------------------------------------------------------------------------------------------ emulation
def emu_lin(x, W, b=None, parts=2, w_scale=None):
    """x W^T + b the way the kernels form it, in fp32 torch on whatever device x is on: row scales from the row maxima, two-part
    (parts = 1: h only) fp16 operands, three products, un-scaled by an exact power of two.  The summation order is torch's."""
    x, W = x.float(), W.float()
    sx = R.row_scale(x.abs().amax(-1, keepdim=True))
    sw = R.weight_scale(W) if w_scale is None else w_scale
    xh, xl = (t.float() for t in R.split_h2(x, sx))
    wh, wl = (t.float() for t in R.split_h2(W, sw))
    acc = xh @ wh.t()
    if parts == 2:
        acc = (xl @ wh.t() + xh @ wl.t()) + acc
    y = torch.ldexp(acc, -(sx + sw))
    return y if b is None else y + b.float()


def emu_chain_a(samp, inside, Wp, bp, W0, b0, W1, b1, W2, b2, parts=2):
    attn = emu_lin(samp, Wp, bp, parts) * (inside.view(-1, 1) != 0).float()
    h1 = torch.relu(emu_lin(torch.relu(emu_lin(attn, W0, b0, parts)), W1, b1, parts))
    return attn, h1 @ W2.float().t() + b2.float()


def emu_chain_b(attn, tgt, Wu, bu, g2, be2, W1, b1, W2, b2, g3, be3, Wc, bc, J, has_ffn=True, qpos=None, Wn=None, bn=None, parts=2):
    V = attn.shape[0]
    ln32 = lambda x, g, b: torch.nn.functional.layer_norm(x, (256,), g.float(), b.float(), 1e-5)
    t1 = ln32(tgt.float() + emu_lin(attn.float().sum(0) / float(V), Wu, bu, parts), g2, be2)
    t = t1
    if has_ffn:
        s1, s2 = R.weight_scale(W1), R.weight_scale(W2)
        ysum = torch.zeros_like(t1)
        for c in range(0, 1024, 256):
            hid = torch.relu(emu_lin(t1, W1[c:c + 256], b1[c:c + 256], parts, w_scale=s1))
            ysum = ysum + emu_lin(hid, W2[:, c:c + 256], None, parts, w_scale=s2)
        t = ln32((ysum + b2.float()) + t1, g3, be3)
    out = dict(tgt=t, prob=torch.sigmoid(t @ Wc.float().t() + bc.float()).view(-1, J, 2).mean(1))
    if Wn is not None:
        out["xw"] = emu_lin(t if qpos is None else t + qpos.float(), Wn, bn, parts)
    return out
