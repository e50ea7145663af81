"""TEST INFRASTRUCTURE ONLY.  Small inputs of the fused sampling operation that reach the edge branches of msda_gsamp_kernel,
msda_gfused_f32_hp_kernel and msda_fused_kernel (csrc/msda.hip, csrc/gsamp_dev.h), in the kernels' own layout, and the figures that say so.
tests/test_gsamp_ref_cpu.py asserts the properties on the CPU; tests/test_gsamp_fp64.py runs the cases on the device.

A case is a dict of CPU tensors: value (n_img, S, 256) fp32 row-major (head planes: planes()), G (n_img * S, 192) and xw (B * Lq, 192) fp32
with their columns in ops.gsamp_column_order(), ref_lvl (n_img, Lq, L, 2) fp32, shapes (L, 2), starts (L,), B, pair_mask (u8) or None,
order: None, an int32 permutation, or the string "bin" (ops.bin_pairs' order of the case: it needs the device; a permutation does not
change the rows, so the reference is taken without it).

Edge cases are ONE-HOT: with G = 0 the offsets and logits of a pair are its xw row, whose 8 column groups every level row shares, so the
hot (group g, point p) -- its logit 14 above logits of unit scale -- is the dominant sample of the L heads m = (g + 8 j) // L on the
levels (g + 8 j) % L, j < L, and those heads' output is essentially that one bilinear tap: a structural error is of the size of the
values, not 1 / 24 of it.  On the power-of-two pyramid the tap's coordinate is exact (r = c / n, offset = t + 0.5 - c: every
operation of (r + off / n) n - 0.5 is exact); on the ragged pyramids the reference point carries the location found by
msda_cases._reach and the hot offset is 0."""
import functools

import numpy as np
import torch

from tests import gsamp_ref as GR
from tests import msda_cases as MC

POW2 = [(8, 16), (4, 8), (2, 4)]
RAGGED = [(6, 10), (3, 5), (1, 3)]
THIN = [(5, 1), (7, 9)]
FOUR = [(8, 16), (4, 8), (2, 4), (3, 5)]
HOT = 14.0
TINY = 2.0 ** -16


def _base(shapes, n_img, Lq, B, seed, g_off=1.5, g_lg=1.5, x_off=1.0, x_lg=1.0, lo=-0.05, hi=1.05):
    rs = np.random.RandomState(seed)
    st, starts, S = MC._levels(shapes)
    L = len(shapes)
    value = rs.standard_normal((n_img, S, 256)).astype(np.float32)
    Gn = np.concatenate([g_off * rs.standard_normal((n_img * S, 128)), g_lg * rs.standard_normal((n_img * S, 64))], 1).astype(np.float32)
    xn = np.concatenate([x_off * rs.standard_normal((B * Lq, 128)), x_lg * rs.standard_normal((B * Lq, 64))], 1).astype(np.float32)
    r = (lo + (hi - lo) * rs.rand(n_img, Lq, L, 2)).astype(np.float32)
    return dict(value=torch.from_numpy(value), Gn=torch.from_numpy(Gn), xn=torch.from_numpy(xn), ref_lvl=torch.from_numpy(r), shapes=st,
                starts=starts, B=B, pair_mask=None, order=None)


def _finish(c):
    """natural columns -> ops.gsamp_column_order()."""
    c["G"] = c.pop("Gn")[:, GR.COLUMN_ORDER].contiguous()
    c["xw"] = c.pop("xn")[:, GR.COLUMN_ORDER].contiguous()
    return c


def _set_hot(xn, row, g, p, ox, oy):
    xn[row, 16 * g + 2 * p], xn[row, 16 * g + 2 * p + 1], xn[row, 128 + 8 * g + p] = ox, oy, HOT


def hot_samples(L, g):
    """(head, level) of the samples that column group g feeds."""
    return [divmod(g + 8 * j, L) for j in range(L)]


# per-axis slots of the exact lattice: (which integer c the reference point sits on, offset) -> coordinate c - 0.5 + offset
SLOTS = (("lo", -0.5), ("lo", -0.5 + TINY), ("lo", 0.0), ("lo", 0.5), ("mid", 0.5), ("mid", 1.0), ("hi1", 0.5), ("hi1", 0.5 + TINY),
         ("hi", 0.5 - TINY), ("hi", 0.5))


def _slot_c(kind, n):
    return {"lo": 0, "mid": n // 2, "hi1": n - 1, "hi": n}[kind]


def slot_target(slot, n):
    return _slot_c(slot[0], n) - 0.5 + slot[1]


def lattice():
    """POW2, G = 0, one pair per point of SLOTS x SLOTS: on every level the hot tap sits, per axis, at -1, just above -1, -0.5, 0, the
    interior integer n // 2, n // 2 + 0.5, n - 1, just above n - 1, just below n and n -- exactly (TINY = 2^-16)."""
    ns = len(SLOTS)
    c = _base(POW2, 1, ns * ns, 1, 301, x_off=2.0)
    c["Gn"].zero_()
    for i in range(ns * ns):
        sx, sy = SLOTS[i % ns], SLOTS[i // ns]
        for l, (H, W) in enumerate(POW2):
            c["ref_lvl"][0, i, l, 0] = _slot_c(sx[0], W) / W
            c["ref_lvl"][0, i, l, 1] = _slot_c(sy[0], H) / H
        _set_hot(c["xn"], i, i % 8, (i // 8) % 8, sx[1], sy[1])
    return _finish(c)


def reach_axis(n):
    """locations along a dimension n whose coordinate (both forms of msda_cases._both agree) is, or is nearest to, -1, just above -1, -0.5,
    0, n // 2, n // 2 + 0.5, n - 1, just above n - 1, just below n, n."""
    out = []
    for t, side in ((-1.0, 0), (-1.0, 1), (-0.5, 0), (0.0, 0), (n // 2, 0), (n // 2 + 0.5, 0), (n - 1.0, 0), (n - 1.0, 1), (float(n), -1), (float(n), 0)):
        try:
            out.append(MC._reach(t, n, side))
        except ValueError:                       # the fused form never gives t on this dimension: its nearest neighbour above
            out.append(MC._reach(t, n, 1))
    return out


def reached_lattice(shapes, seed):
    """G = 0, the hot offset is 0 and the reference point of level l carries the location: one pair per point of the product of the
    two axes' reach_axis sets, on every level (L = 2: column group g feeds level g % 2 in both of its heads, so every point comes twice,
    once with an even and once with an odd group)."""
    L = len(shapes)
    reps = 2 if L == 2 else 1
    c = _base(shapes, 1, 100 * reps, 1, seed, x_off=2.0)
    c["Gn"].zero_()
    axes = [(reach_axis(W), reach_axis(H)) for H, W in shapes]
    for i in range(100 * reps):
        pt, rep = i % 100, i // 100
        for l, (xs, ys) in enumerate(axes):
            c["ref_lvl"][0, i, l, 0] = xs[pt % 10][0]
            c["ref_lvl"][0, i, l, 1] = ys[pt // 10][0]
        _set_hot(c["xn"], i, (pt % 4) * 2 + rep if L == 2 else pt % 8, (pt // 8) % 8, 0.0, 0.0)
    return _finish(c)


FOOT_T = ("-1", "-0.5", "0", "n-1", "n-0.5", "below", "above", "inner")


def _foot_r(kind, n):
    t = {"-1": -1.0, "-0.5": -0.5, "0": 0.0, "n-1": n - 1.0, "n-0.5": n - 0.5}.get(kind)
    if t is not None:
        return (t + 0.5) / n                      # footprint coordinate ix = r n - 0.5 (before the clamp)
    return {"below": -0.3, "above": 1.3, "inner": 0.37}[kind]


def footprint(shapes, seed):
    """G nonzero.  64 pairs; on level l pair i has its reference point, per axis, at the footprint coordinates -1, -0.5, 0, n - 1, n - 0.5,
    beyond the clamp on either side (2 r - 1 = -1.6, 1.6: the clamped coordinate -0.05 n - 0.5 is inside the padded cell for n < 10 and
    outside for n >= 10) or inside -- a different point of the 8 x 8 product on every level, so a level row whose footprint is clamped feeds
    (through the view) samples on levels whose reference point is inside the map."""
    c = _base(shapes, 1, 64, 1, seed, g_off=1.5, g_lg=2.0)
    for i in range(64):
        for l, (H, W) in enumerate(shapes):
            c["ref_lvl"][0, i, l, 0] = _foot_r(FOOT_T[(i + 3 * l) % 8], W)
            c["ref_lvl"][0, i, l, 1] = _foot_r(FOOT_T[(i // 8 + 5 * l) % 8], H)
    return _finish(c)


def levels(L):
    """random inputs at L levels: per-level reference points, G and xw columns random per group -- the reinterpretation, the second
    footprint of a head (L = 3: heads 2 and 5) and the partial last phase-A round matter."""
    shapes = {1: [(7, 9)], 2: THIN, 3: RAGGED, 4: FOUR}[L]
    return _finish(_base(shapes, 2, 37, 1, 310 + L))


def batch():
    """V = 2, B = 3: n_img = 6, image n takes the xw rows of batch item n % 3 (distinct per item)."""
    return _finish(_base(RAGGED, 6, 11, 3, 320))


def ragged_count(count, kind):
    """`count` pairs (1, 33, 257: no multiple of the 32 / 64 / 128 / 256 slots of a workgroup, nor of an XCD chunk) with about half of
    them masked; order None, ops.bin_pairs' ("bin") or a seeded permutation ("perm")."""
    c = _base(POW2, 1, count, 1, 330 + count)
    rs = np.random.RandomState(340 + count)
    mask = (rs.rand(count) < 0.5).astype(np.uint8)
    mask[0] = 1
    if count > 1:
        mask[-1] = 0
    c["pair_mask"] = torch.from_numpy(mask)
    c["order"] = {"none": None, "bin": "bin", "perm": torch.from_numpy(rs.permutation(count).astype(np.int32))}[kind]
    return _finish(c)


SOFTMAX_KINDS = ("equal", "shift", "spread", "dominant_outside", "all_outside")


def softmax():
    """G = 0, query q is of kind SOFTMAX_KINDS[q % 5]: all logits equal; a common shift of 3000; a spread of 200; the dominant sample
    (HOT) 10^4 pixels outside the map -- it reads nothing and still owns the denominator --; every sample 10^30 pixels outside: the row
    is exactly 0."""
    c = _base(POW2, 1, 40, 1, 350, lo=0.2, hi=0.8)
    c["Gn"].zero_()
    rs = np.random.RandomState(351)
    for q in range(40):
        kind = SOFTMAX_KINDS[q % 5]
        if kind == "equal":
            c["xn"][q, 128:] = 0.25
        elif kind == "shift":
            c["xn"][q, 128:] += 3000.0
        elif kind == "spread":
            lg = (200.0 * rs.rand(8, 8) - 100.0).astype(np.float32)
            lg[:, q % 8], lg[:, (q + 3) % 8] = -100.0, 100.0          # every column group, so every head, spans the 200
            c["xn"][q, 128:] = torch.from_numpy(lg.reshape(64))
        elif kind == "dominant_outside":
            _set_hot(c["xn"], q, (q // 5) % 8, q % 8, 1e4, 0.0)
        else:
            c["xn"][q, :128] = torch.from_numpy(np.where(rs.rand(128) < 0.5, -1e30, 1e30).astype(np.float32))
    return _finish(c)


CASES = {
    "lattice": lattice,
    "lattice_ragged": functools.partial(reached_lattice, RAGGED, 302),
    "thin": functools.partial(reached_lattice, THIN, 303),
    "footprint": functools.partial(footprint, POW2, 304),
    "footprint_ragged": functools.partial(footprint, RAGGED, 305),
    "footprint_thin": functools.partial(footprint, THIN, 306),
    "levels_1": functools.partial(levels, 1),
    "levels_2": functools.partial(levels, 2),
    "levels_3": functools.partial(levels, 3),
    "levels_4": functools.partial(levels, 4),
    "batch": batch,
    "softmax": softmax,
}
for _n in (1, 33, 257):
    for _k in ("none", "bin", "perm"):
        CASES["ragged_count_%d_%s" % (_n, _k)] = functools.partial(ragged_count, _n, _k)
ONE_HOT = ("lattice", "lattice_ragged", "thin")


@functools.lru_cache(maxsize=None)
def case(name):
    """the case's tensors (cached: treat them as read-only)."""
    return CASES[name]()


def planes(value):
    """row-major (n_img, S, 256) -> head planes (n_img, 8, S, 32)."""
    n_img, S, _ = value.shape
    return value.view(n_img, S, 8, 32).permute(0, 2, 1, 3).contiguous()


def operands(name, mode="f32"):
    """(value, G) of the case as the kernels of `mode` store them: fp32, or rounded to bf16 ("bf16"; returned as fp32 tensors)."""
    c = case(name)
    if mode == "bf16":
        return c["value"].bfloat16().float(), c["G"].bfloat16().float()
    return c["value"], c["G"]


def evaluate(name, mode="f32", dtype=GR.F64, wrong=None):
    c = case(name)
    value, G = operands(name, mode)
    order = None if isinstance(c["order"], str) else c["order"]
    return GR.gsamp(value, G, c["xw"], c["ref_lvl"], c["shapes"], c["starts"], c["B"], c["pair_mask"], order, dtype, wrong)


@functools.lru_cache(maxsize=None)
def reference(name, mode="f32"):
    """(ref, k) of a case (cached: read-only): tests/gsamp_ref.gsamp in fp64 on the operands of `mode`, and k = 4 x the largest
    |ref32 - ref64| / (2^-24 out_A), ref32 the same statement in fp32 on the CPU."""
    ref = evaluate(name, mode)
    return ref, GR.yardstick(ref, evaluate(name, mode, GR.F32))


@functools.lru_cache(maxsize=None)
def reference_fused(name, mode="f32"):
    """(oa, ref, k) of msda_fused on the case: oa (pairs * L, 192) fp32 formed on the CPU from the same G, xw and reference points (the
    fp32 G: oa is an fp32 operand of both kernels), the reference on that oa and the value of `mode`."""
    c = case(name)
    oa = GR.oa_of(c["G"], c["xw"], c["ref_lvl"], c["shapes"], c["starts"], c["B"])
    value = operands(name, mode)[0]
    ref = GR.fused(value, oa, c["ref_lvl"], c["shapes"], c["starts"])
    return oa, ref, GR.yardstick(ref, GR.fused(value, oa, c["ref_lvl"], c["shapes"], c["starts"], GR.F32))


def kernel_coordinates(c, ref):
    """the pixel coordinates of every sample as the kernels' fp32 arithmetic forms them from the reference's offsets (exact where G = 0):
    lx = r + off * (1 / W) in fp32, then lx * W - 0.5 fused and in two roundings.  Returns h_fma, w_fma, h_plain, w_plain (fp32 numpy,
    (n_img, Lq, M, L, P))."""
    off = ref["offsets"].float().numpy()
    r = c["ref_lvl"].numpy()[:, :, None, :, None, :]
    WH = np.stack([c["shapes"][:, 1].numpy(), c["shapes"][:, 0].numpy()], -1).astype(np.float32)[None, None, None, :, None, :]
    inv = (np.float32(1.0) / WH).astype(np.float32)
    loc = (r + (off * inv).astype(np.float32)).astype(np.float32)
    fma = (loc.astype(np.float64) * WH - 0.5).astype(np.float32)
    plain = ((loc * WH).astype(np.float32) - np.float32(0.5)).astype(np.float32)
    return fma[..., 1], fma[..., 0], plain[..., 1], plain[..., 0]


def hot_mask(c, ref):
    """(n_img, Lq, M, L, P) bool: the dominant sample of every one-hot head."""
    return (ref["weights"] > 0.99).numpy()
