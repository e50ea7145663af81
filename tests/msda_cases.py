"""TEST INFRASTRUCTURE ONLY.  Inputs of the sampling op that reach the branches of the deterministic backward (csrc/msda_bwd.hip) at small
sizes, and the figures of the chain that say so.  The numbers come from the kernel's constants: BW_T = 8 (tile edge), 256 entries per pass
of bw_reduce, 4096 bins per chunk of bw_scan, BW_PARTS = 128, 32 bins per workgroup of bw_prefix, 16-byte loads in bw_absmax.
tests/test_msda_ref_oracle.py asserts the properties on the CPU; tests/test_msda_fp64.py runs the cases on the device.

A case is a dict of CPU tensors: value (N, S, M, D), shapes (L, 2), starts (L,), loc (N, Lq, M, L, P, 2), weight (N, Lq, M, L, P),
go (N, Lq, M * D) -- all fp32 -- and for nonfinite_go also go_clean and bad_rows."""
import functools

import numpy as np
import torch

from tests import msda_ref as R

BW_T, BW_PASS, BW_SCAN_CHUNK, BW_PARTS = 8, 256, 4096, 128
BAD_LOCS = (float("nan"), float("inf"), float("-inf"), 1e30, -1e30, 3.4e38, -3.4e38, 2.0 ** 31 + 0.5, -(2.0 ** 31 + 0.5))


def _levels(shapes):
    st = torch.tensor(shapes, dtype=torch.long)
    starts = torch.cat([st.new_zeros(1), (st[:, 0] * st[:, 1]).cumsum(0)[:-1]])
    return st, starts, int((st[:, 0] * st[:, 1]).sum())


def _generic(shapes, N, M, D, Lq, P, seed, lo=-0.15, hi=1.15, wmax=None):
    """seeded normal value / grad_output, uniform locations in [lo, hi]^2, weights normalised over a head's L * P samples, or uniform in
    [-wmax, wmax] (un-normalised, mixed signs)."""
    rs = np.random.RandomState(seed)
    st, starts, S = _levels(shapes)
    L = len(shapes)
    value = rs.standard_normal((N, S, M, D)).astype(np.float32)
    loc = (lo + (hi - lo) * rs.rand(N, Lq, M, L, P, 2)).astype(np.float32)
    if wmax is None:
        wgt = rs.rand(N, Lq, M, L, P).astype(np.float32)
        wgt = wgt / wgt.reshape(N, Lq, M, -1).sum(-1)[..., None, None]
    else:
        wgt = (wmax * (2.0 * rs.rand(N, Lq, M, L, P) - 1.0)).astype(np.float32)
    go = rs.standard_normal((N, Lq, M * D)).astype(np.float32)
    return dict(value=torch.from_numpy(value), shapes=st, starts=starts, loc=torch.from_numpy(loc), weight=torch.from_numpy(wgt),
                go=torch.from_numpy(go))


def one_bin():
    """903 samples in the one bin of an 8 x 8 map: four passes of bw_reduce, the last one partial (135 entries: two full wavefronts, one
    with 7 entries = a single step, one idle), M = 1."""
    return _generic([(8, 8)], 1, 1, 32, 301, 3, 201, lo=0.0, hi=1.0)


def odd_heads(variant):
    """per_img = 90 floats of attn_weight: image 1 starts 8 bytes off a 16-byte boundary (lead = 2), images 0 and 2 end with a 2-float
    tail.  The largest |attn_weight| -- 8 x the others, so a missed maximum saturates the int32 contributions -- sits in the first two
    elements of image 1 ("a") or in the last two of image 2 ("b"); both samples are inside their maps.  bpi = 24."""
    c = _generic([(9, 17), (1, 9)], 3, 3, 32, 5, 3, 202, lo=0.05, hi=0.95, wmax=1.0)
    w = c["weight"].view(3, -1)
    loc = c["loc"].view(3, -1, 2)
    if variant == "a":
        w[1, 0], w[1, 1] = 8.0, -7.5
        loc[1, 0], loc[1, 1] = torch.tensor([0.31, 0.62]), torch.tensor([0.77, 0.18])
    else:
        w[2, -1], w[2, -2] = -8.0, 7.5
        loc[2, -1], loc[2, -2] = torch.tensor([0.31, 0.62]), torch.tensor([0.77, 0.18])
    return c


def many_bins(second=(48, 60)):
    """T_total = 228 tiles (215, odd, with the second level (35, 52): both of its dimensions end in a partial tile), N * bpi = 5472 (5160)
    bins: bw_scan takes a second chunk of 4096 with a carry, bw_prefix a ragged last workgroup; 2048 samples per image and level leave a third of
    the bins empty (the interior zero fill)."""
    return _generic([(96, 120), second], 3, 8, 32, 64, 4, 203 if second == (48, 60) else 204)


def ragged():
    """six levels with dimensions 1, below 8, exactly 8, 8 k + 1, and L above 4."""
    return _generic([(7, 13), (1, 9), (5, 1), (8, 8), (9, 9), (16, 17)], 2, 2, 32, 40, 2, 205, lo=-0.3, hi=1.3)


def _both(l, n):
    """fp32 coordinate of the fp32 location l on a map dimension n in the fused and in the two-rounding form."""
    l = np.float32(l)
    return np.float32(np.float64(l) * n - 0.5), np.float32(np.float32(l * np.float32(n)) - np.float32(0.5))


def _reach(t, n, side):
    """a location whose coordinate is the same in both forms and equals t (side 0), or is the nearest such value above (+1) / below (-1) t."""
    l0 = np.float32((t + 0.5) / n)
    best = None
    for k in range(-64, 65):
        l = l0
        for _ in range(abs(k)):
            l = np.nextafter(l, np.float32(np.inf if k > 0 else -np.inf), dtype=np.float32)
        a, b = _both(l, n)
        if a != b:
            continue
        if side == 0 and a == np.float32(t):
            return float(l), float(a)
        if side != 0 and (a - t) * side > 0 and (best is None or abs(a - t) < abs(best[1] - t)):
            best = (float(l), float(a))
    if best is None:
        raise ValueError("no location reaches %r on a dimension of %d" % (t, n))
    return best


def lattice_axis(n):
    """locations and coordinates along a map dimension n: the exclusion edges -1 and n, the first floats inside them, -0.5, 0, the
    integers at the tile border (7, 8), 7.5, n - 1 and the first float above it ("first float": the nearest coordinate within 64 ulps of the
    location on which both coordinate forms agree).  On a dimension that is no power of two the fused form
    cannot give most of these exactly: the nearest coordinates on both sides stand in."""
    want = [(-1.0, 0), (-1.0, 1), (-0.5, 0), (0.0, 0), (7.0, 0), (7.5, 0), (8.0, 0), (n - 1.0, 0), (n - 1.0, 1), (float(n), -1), (float(n), 0)]
    got = {}
    for t, side in want:
        try:
            found = [_reach(t, n, side)]
        except ValueError:       # (t + 0.5) / n is no fp32 number (n = 9): the fused form never gives t; take its neighbours on both sides
            found = [_reach(t, n, 1), _reach(t, n, -1)]
        for l, c in found:
            got[c] = l
    cs = sorted(got)
    return [got[c] for c in cs], cs


def lattice(D=32):
    """levels (8, 16) and (16, 9), M = P = N = 1: one query per point of the product of the two axes' sets (lattice_axis), the same query
    index on both levels.  Every sample has the same coordinate in both forms; nothing is left out of any comparison."""
    shapes = [(8, 16), (16, 9)]
    axes = [(lattice_axis(h)[0], lattice_axis(w)[0]) for h, w in shapes]
    Lq = max(len(a) * len(b) for a, b in axes)
    c = _generic(shapes, 1, 1, D, Lq, 1, 206, wmax=1.0)
    for l, (ys, xs) in enumerate(axes):
        for q in range(Lq):
            c["loc"][0, q, 0, l, 0, 1] = ys[(q // len(xs)) % len(ys)]
            c["loc"][0, q, 0, l, 0, 0] = xs[q % len(xs)]
    return c


def coincident(kind):
    """4096 samples of one head on one spot of a 16 x 16 map, weights and gradients of mixed signs: a texel centre inside a tile (row 3,
    column 5: lh = lw = 0), or the point (7.25, 7.625), whose four corners are the last interior pixel of one tile and three pixels shared
    with its neighbours (the pixel (8, 8) belongs to four tiles)."""
    c = _generic([(16, 16)], 1, 1, 32, 1024, 4, 207, wmax=1.0)
    y, x = (3.0, 5.0) if kind == "centre" else (7.25, 7.625)
    c["loc"][..., 0] = (x + 0.5) / 16
    c["loc"][..., 1] = (y + 0.5) / 16
    return c


def range_case(zero_image=None):
    """the shape of the golden case small_f32 with N = 3: gradient scales 1, 1e6 and 1e-30 per image, un-normalised weights up to 40;
    zero_image: that image's grad_output is all zero (scale 0: its grad_value is exactly zero)."""
    c = _generic([(12, 20), (6, 10), (3, 5)], 3, 8, 32, 37, 8, 208, wmax=40.0)
    c["go"] *= torch.tensor([1.0, 1e6, 1e-30]).view(3, 1, 1)
    if zero_image is not None:
        c["go"][zero_image] = 0.0
    return c


def nonfinite_loc():
    """NaN, +-Inf, +-1e30, +-3.4e38 and +-(2^31 + 0.5) on one coordinate in eight: such samples read and write nothing."""
    c = _generic([(12, 20), (6, 10), (3, 5)], 2, 8, 32, 37, 8, 209)
    rs = np.random.RandomState(210)
    flat = c["loc"].view(-1)
    pos = torch.from_numpy(rs.permutation(flat.numel())[:flat.numel() // 8])
    flat[pos] = torch.tensor(BAD_LOCS, dtype=torch.float32)[torch.from_numpy(rs.randint(0, len(BAD_LOCS), pos.numel()))]
    return c


NONFINITE_GO = ((0, 3, 1, 5, float("inf")), (0, 7, 0, 0, float("nan")), (1, 2, 1, 31, float("-inf")), (1, 9, 0, 3, float("inf")),
                (1, 9, 0, 4, float("nan")))


def nonfinite_go():
    """NaN, +Inf and -Inf entries (image, query, head, channel) in grad_output; sample (0, 3, 1, level 0, point 0) sits on the centre of texel
    (2, 3) (lh = lw = 0: three of its corner weights are zero), the other samples of the affected rows are generic.  go_clean: the same
    with zeros at those entries; bad_rows (N, Lq, M): the rows that carry one."""
    c = _generic([(8, 16), (16, 8), (4, 4)], 2, 2, 32, 20, 2, 211, lo=0.02, hi=0.98)
    c["loc"][0, 3, 1, 0, 0] = torch.tensor([3.5 / 16, 2.5 / 8])
    go = c["go"].view(2, 20, 2, 32)
    c["go_clean"] = go.clone()
    c["bad_rows"] = torch.zeros(2, 20, 2, dtype=torch.bool)
    for n, q, m, ch, x in NONFINITE_GO:
        go[n, q, m, ch] = x
        c["go_clean"][n, q, m, ch] = 0.0
        c["bad_rows"][n, q, m] = True
    c["go_clean"] = c["go_clean"].view(2, 20, 64)
    return c


def generic_d(D):
    """the generic generator at another head width (the fp32-atomic kernel: D = 16 and 64 reduce with shuffles, D = 12 with atomics)."""
    return _generic([(9, 17), (1, 9), (12, 20)], 2, 3, D, 37, 3, 212 + D, lo=-0.2, hi=1.2)


CASES = {
    "one_bin": one_bin,
    "odd_heads_a": functools.partial(odd_heads, "a"),
    "odd_heads_b": functools.partial(odd_heads, "b"),
    "many_bins": many_bins,
    "many_bins_b": functools.partial(many_bins, (35, 52)),
    "ragged": ragged,
    "lattice": lattice,
    "coincident_centre": functools.partial(coincident, "centre"),
    "coincident_corner": functools.partial(coincident, "corner"),
    "range": range_case,
    "range_zero": functools.partial(range_case, 0),
    "nonfinite_loc": nonfinite_loc,
    "nonfinite_go": nonfinite_go,
}
DET_CASES = list(CASES)                                       # D = 32: the deterministic form takes them
ATOMIC_ONLY_CASES = []                                        # D = 16 / 64 / 12: mvg_msda_backward_det_workspace returns 0
for _D in (16, 64, 12):
    CASES["generic_d%d" % _D] = functools.partial(generic_d, _D)
    CASES["lattice_d%d" % _D] = functools.partial(lattice, _D)
    ATOMIC_ONLY_CASES += ["generic_d%d" % _D, "lattice_d%d" % _D]


@functools.lru_cache(maxsize=None)
def case(name):
    """the case's tensors (cached: treat them as read-only)."""
    return CASES[name]()


def _lead_tail(per_img, N):
    """floats before the first and after the last whole 16-byte load of every image's slice (bw_absmax), for a 16-byte-aligned tensor."""
    out = []
    for n in range(N):
        lead = min(per_img, (4 - ((n * per_img) & 3)) & 3)
        out.append((lead, (per_img - lead) & 3))
    return out


def properties(c):
    """the figures of the chain for a case: bins per image, the largest bin, N * bpi, bpi % 32, the lead / tail of every image's slice of
    attn_weight and grad_output, the numbers of out-of-map and of ambiguous samples among `samples`."""
    N, S, M, D = c["value"].shape
    _, Lq, _, L, P, _ = c["loc"].shape
    b, T_total = R.bins(c["loc"], c["shapes"], M, BW_T)
    bpi = T_total * M
    key = (torch.arange(N).view(N, 1, 1, 1, 1) * bpi + b)[b >= 0]
    counts = torch.bincount(key, minlength=N * bpi)
    amb = R.ambiguous(c["loc"], c["shapes"])
    return dict(T_total=T_total, bpi=bpi, nbins=N * bpi, bpi_mod32=bpi % 32, largest_bin=int(counts.max()), empty_bins=int((counts == 0).sum()),
                wgt_lead_tail=_lead_tail(Lq * M * L * P, N), go_lead_tail=_lead_tail(Lq * M * D, N),
                out_of_map=int((b < 0).sum()), ambiguous=int(amb.sum()), samples=b.numel())


KINDS = ("out", "grad_value", "grad_loc", "grad_attn")


def reference_of(value, shapes, starts, loc, weight, go, form="fma"):
    """(ref, k): tests/msda_ref.msda in fp64 with the error scales, and per output kind k = 4 x the largest |ref32 - ref64| / (2^-24 A),
    ref32 being the same statement evaluated in fp32 after the coordinates: the yardstick of the error bars (it measures the reference)."""
    ref = R.msda(value, shapes, starts, loc, weight, go, R.F64, form)
    r32 = R.msda(value, shapes, starts, loc, weight, go, R.F32, form)
    k = {}
    for kind in KINDS:
        A = ref[kind + "_A"]
        ratio = (r32[kind].double() - ref[kind]).abs() / (2.0 ** -24 * A)
        k[kind] = 4.0 * float(ratio[A > 0].max()) if bool((A > 0).any()) else 0.0
    ref["ambiguous"] = R.ambiguous(loc, shapes) if form != "f64" else torch.zeros_like(ref["inside"])
    return ref, k


@functools.lru_cache(maxsize=None)
def reference(name, mode="f32"):
    """reference_of a case (cached: read-only) -- mode "f32": the fp32 inputs and the device's fused coordinates; "bf16": the same on the
    value rounded to bf16; "f64": fp64 coordinates (the fp64 kernels on the widened inputs) with the k of mode "f32" -- the yardstick needs
    the exact fp32 fractions lh, lw of the fp32 coordinates (1 - lh is then exact too); the fraction of an fp64 coordinate rounded to fp32 is
    neither, and a k measured that way (2e4 on a corner weight of 1e-8) says nothing about the operation.  The non-finite grad_output
    entries of nonfinite_go are zeros here."""
    c = case(name)
    go = c.get("go_clean", c["go"])
    if mode == "f64":
        ref = R.msda(c["value"], c["shapes"], c["starts"], c["loc"], c["weight"], go, R.F64, "f64")
        ref["ambiguous"] = torch.zeros_like(ref["inside"])
        return ref, reference(name, "f32")[1]
    value = c["value"].bfloat16().float() if mode == "bf16" else c["value"]
    return reference_of(value, c["shapes"], c["starts"], c["loc"], c["weight"], go)


def bound_per_image(go, weight):
    """max |grad_output[n]| * max |attn_weight[n]| over the finite entries: the scale of image n's fixed-point contributions."""
    N = go.shape[0]
    g = torch.where(torch.isfinite(go), go, torch.zeros_like(go)).abs().reshape(N, -1).amax(1).double()
    w = torch.where(torch.isfinite(weight), weight, torch.zeros_like(weight)).abs().reshape(N, -1).amax(1).double()
    return g * w


def bar(ref, k, kind, eps=2.0 ** -24, fixed_point_bound=None):
    """elementwise error bar of an output: k * eps * A + 2 ulp of the value (eps = 2^-24: fp32 outputs, 2^-53: fp64 outputs); the
    deterministic grad_value adds the rounding its kernel documents, cnt * 2^-31 * bound_n."""
    b = k[kind] * eps * ref[kind + "_A"] + 4.0 * eps * ref[kind].abs()
    if fixed_point_bound is not None:
        assert kind == "grad_value"
        b = b + (ref["grad_value_cnt"].double() * 2.0 ** -31 * fixed_point_bound.view(-1, 1, 1)).unsqueeze(-1)
    return b
