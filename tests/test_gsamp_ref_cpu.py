"""tests/gsamp_ref.py and tests/gsamp_cases.py on the CPU: the fp64 statement of the fused sampling operation equals the oracle, every case
reaches what it is named for, the cases tell each deliberately wrong variant of the statement from the right one, and the fp32
yardstick gives a finite k per case.  No device."""
import numpy as np
import pytest
import torch

from oracle import decoder_ref as O
from tests import gsamp_cases as GC
from tests import gsamp_ref as GR

F64 = torch.float64
PYRAMIDS = {1: [(7, 9)], 2: GC.THIN, 3: GC.RAGGED, 4: GC.FOUR}


def test_column_order_is_the_library_s():
    from mvgformer_amd import ops
    assert torch.equal(GR.COLUMN_ORDER, ops.gsamp_column_order())


# ------------------------------------------------------------------------------------------------------ the reference against the oracle
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_reference_equals_the_oracle(L, B):
    """seeded weights and features, V = 2 views: gsamp_ref on G = feat @ Woa^T, xw = x @ Woa^T + b gives the oracle's `sampled` to 1e-12 of
    scale in fp64 (the G-commutation), and the oa form of the reference gives the G form."""
    shapes = PYRAMIDS[L]
    V, Lq, C = 2, 13, 256
    g = torch.Generator().manual_seed(400 + 10 * L + B)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    st = torch.tensor(shapes, dtype=torch.long)
    starts = torch.cat([st.new_zeros(1), (st[:, 0] * st[:, 1]).cumsum(0)[:-1]])
    src = [rnd(V * B, C, H, W) for H, W in shapes]
    query = rnd(B, Lq, C)
    ref_lvl = -0.2 + 1.4 * torch.rand(V * B, Lq, L, 2, generator=g, dtype=F64)
    prm = {"p.rayconv.weight": rnd(C, C) / 16, "p.rayconv.bias": rnd(C), "p.sampling_offsets.weight": rnd(128, C) / 8,
           "p.sampling_offsets.bias": rnd(128), "p.attention_weights.weight": rnd(64, C) / 8, "p.attention_weights.bias": rnd(64),
           "p.output_proj.weight": rnd(C, C) / 16, "p.output_proj.bias": rnd(C)}
    want = torch.cat([O.proj_attn_forward(prm, "p.", query, ref_lvl[v * B:(v + 1) * B], [s[v * B:(v + 1) * B] for s in src], st, starts,
                                          return_intermediates=True)[1]["sampled"] for v in range(V)], 0)          # (V B, Lq, 256), view-major
    flat = torch.cat([s.flatten(2) for s in src], -1).transpose(1, 2)                                              # (V B, S, C)
    value = flat @ prm["p.rayconv.weight"].t() + prm["p.rayconv.bias"]
    Woa = torch.cat([prm["p.sampling_offsets.weight"], prm["p.attention_weights.weight"]], 0)
    boa = torch.cat([prm["p.sampling_offsets.bias"], prm["p.attention_weights.bias"]], 0)
    G = (flat.reshape(-1, C) @ Woa.t())[:, GR.COLUMN_ORDER].contiguous()
    xw = (query.reshape(-1, C) @ Woa.t() + boa)[:, GR.COLUMN_ORDER].contiguous()
    scale = float(want.abs().max())
    for val in (value, GC.planes(value)):                                    # row-major and head planes
        got = GR.gsamp(val, G, xw, ref_lvl, st, starts, B)
        err = float((got["out"].view_as(want) - want).abs().max())
        print("L %d B %d: |gsamp_ref - oracle| max %.3e of scale %.3e" % (L, B, err, scale))
        assert err <= 1e-12 * scale
    oa = GR.phase_a(G, xw, ref_lvl, st, starts, B)[0].reshape(-1, 192)
    via_oa = GR.fused(value, oa, ref_lvl, st, starts)
    assert float((via_oa["out"] - got["out"]).abs().max()) <= 1e-12 * scale
    assert bool(torch.isfinite(got["out_A"]).all()) and bool((got["out_A"] >= got["out_abs"]).all())


# -------------------------------------------------------------------------------------------- every case reaches what it is named for
def _hot_coordinates(name):
    c = GC.case(name)
    ref, _ = GC.reference(name)
    hf, wf, hp, wp = GC.kernel_coordinates(c, ref)
    hot = GC.hot_mask(c, ref)
    assert np.array_equal(hf[hot], hp[hot]) and np.array_equal(wf[hot], wp[hot])      # fused and two-rounding coordinates agree on the taps
    return c, ref, hot, hf, wf


def test_lattice_taps_sit_exactly_on_the_lattice():
    """100 pairs x 3 hot heads: on every level every point of SLOTS x SLOTS is the coordinate of exactly one hot tap, exactly."""
    c, ref, hot, hf, wf = _hot_coordinates("lattice")
    assert int(hot.sum()) == 300 and bool((hot.sum((3, 4)) <= 1).all())
    for l, (H, W) in enumerate(GC.POW2):
        got = sorted(zip(hf[:, :, :, l][hot[:, :, :, l]].tolist(), wf[:, :, :, l][hot[:, :, :, l]].tolist()))
        want = sorted((np.float32(GC.slot_target(sy, H)), np.float32(GC.slot_target(sx, W))) for sy in GC.SLOTS for sx in GC.SLOTS)
        assert got == [(float(a), float(b)) for a, b in want], l
    # the same coordinates in the fp64 statement: the reference and the kernels sample the same points
    assert np.array_equal(ref["h"].numpy()[hot], hf[hot].astype(np.float64)) and np.array_equal(ref["w"].numpy()[hot], wf[hot].astype(np.float64))


@pytest.mark.parametrize("name,shapes", [("lattice_ragged", GC.RAGGED), ("thin", GC.THIN)])
def test_reached_lattices_cover_the_edges_of_every_level(name, shapes):
    """per level and axis, hot taps at -1 or the first coordinate inside it, at n or the last coordinate inside it, on both sides of
    n - 1, and -- on a dimension of 1 -- taps whose two corners are pixel 0 and the padding on either side."""
    c, ref, hot, hf, wf = _hot_coordinates(name)
    L = len(shapes)
    assert int(hot.sum()) == c["ref_lvl"].shape[1] * L and all(int(hot[:, :, :, l].sum()) >= 100 for l in range(L))
    for l, (H, W) in enumerate(shapes):
        for co, n in ((hf[:, :, :, l][hot[:, :, :, l]], H), (wf[:, :, :, l][hot[:, :, :, l]], W)):
            count = lambda lo, hi: int(((co >= lo) & (co <= hi)).sum())
            assert count(-1.0, -1.0) + count(-1.0, -1.0 + 1e-4) >= 10, (l, n)                 # the exclusion edge and just inside it
            assert count(n - 1e-4, n) >= 10 and count(n - 1.0, n - 1.0 + 1e-4) >= 10, (l, n)
            assert count(-0.5 - 1e-4, -0.5 + 1e-4) >= 10 and count(-1e-4, 1e-4) >= 10, (l, n)
            if n == 1:
                assert int(((co > -1) & (co < 0)).sum()) >= 10 and int(((co > 0) & (co < 1)).sum()) >= 10


@pytest.mark.parametrize("name,shapes", [("footprint", GC.POW2), ("footprint_ragged", GC.RAGGED), ("footprint_thin", GC.THIN)])
def test_footprint_cases_reach_the_clamp_and_the_padding(name, shapes):
    """per level and axis: reference points beyond the clamp on both sides (the clamped coordinate inside the padded cell exactly on the
    dimensions below 10), footprints with a padded corner on either side, and a different reference point on every level."""
    c = GC.case(name)
    ix, iy, _, _, clamped = GR.footprint_coordinates(c["ref_lvl"], c["shapes"])
    for l, (H, W) in enumerate(shapes):
        for co, cl, n in ((ix[0, :, l], clamped[0, :, l, 0], W), (iy[0, :, l], clamped[0, :, l, 1], H)):
            lo, hi = co[cl & (co < 0)], co[cl & (co > 0)]
            assert lo.numel() >= 8 and hi.numel() >= 8, (l, n)
            assert bool((lo > -1).all()) == (n < 10) and bool((hi < n).all()) == (n < 10), (l, n)
            x0 = torch.floor(co)
            assert int((x0 == -1).sum()) >= 8 and int((x0 == n - 1).sum()) >= 8, (l, n)      # left / right corner in the padding
            assert int(((co - x0).abs() < 1e-6).sum()) >= 8, (l, n)                          # on a pixel centre: the other corner's weight is 0
    if len(shapes) > 1:
        r = c["ref_lvl"][0]
        assert bool(((r[:, 0] - r[:, 1]).abs().amax(-1) > 0).all())


def test_thin_footprint_straddles_both_padded_sides():
    """W = 1 (level 0 of THIN): footprints with x0 = -1 (padding left, pixel 0 right) and with x0 = 0 (pixel 0 left, padding right)."""
    c = GC.case("footprint_thin")
    ix = GR.footprint_coordinates(c["ref_lvl"], c["shapes"])[0][0, :, 0]
    x0 = torch.floor(ix)
    assert int(((x0 == -1) & (ix > -1)).sum()) >= 8 and int(((x0 == 0) & (ix > 0)).sum()) >= 8


def test_level_cases_have_two_level_heads_and_partial_rounds():
    """the heads whose L flat groups span two level rows (l_hi != l_lo: heads 2 and 5 at L = 3), and the chunks of the last phase-A round:
    3 L % 4 lanes of a quad in msda_gsamp_kernel, 6 L % 8 lanes of a head's 8 in msda_gfused_f32_hp_kernel."""
    two = {L: [m for m in range(8) if (m * L) >> 3 != (m * L + L - 1) >> 3] for L in (1, 2, 3, 4)}
    assert two == {1: [], 2: [], 3: [2, 5], 4: []}
    assert {L: (3 * L) % 4 for L in (1, 2, 3, 4)} == {1: 3, 2: 2, 3: 1, 4: 0}
    assert {L: (6 * L) % 8 for L in (1, 2, 3, 4)} == {1: 6, 2: 4, 3: 2, 4: 0}
    for L in (1, 2, 3, 4):
        c = GC.case("levels_%d" % L)
        assert c["ref_lvl"].shape[2] == L and c["shapes"].shape[0] == L
        if L > 1:
            assert bool(((c["ref_lvl"][:, :, 0] - c["ref_lvl"][:, :, 1]).abs().amax(-1) > 1e-3).all())
        Gn = GR.natural(c["G"])
        assert len({float(Gn[0, 16 * g]) for g in range(8)}) == 8 and len({float(Gn[0, 128 + 8 * g]) for g in range(8)}) == 8


def test_batch_and_count_cases():
    c = GC.case("batch")
    assert c["B"] == 3 and c["ref_lvl"].shape[0] == 6 and c["xw"].shape[0] == 3 * c["ref_lvl"].shape[1]
    xw = c["xw"].view(3, -1, 192)
    assert not torch.equal(xw[0], xw[1]) and not torch.equal(xw[1], xw[2])
    for n in (1, 33, 257):
        for kind in ("none", "bin", "perm"):
            c = GC.case("ragged_count_%d_%s" % (n, kind))
            assert c["ref_lvl"].shape[1] == n and all(n % s for s in (32, 64, 128, 256)) and c["pair_mask"].numel() == n
            if n > 1:
                assert 0.3 * n < int(c["pair_mask"].sum()) < 0.7 * n
            ref, _ = GC.reference("ragged_count_%d_%s" % (n, kind))
            assert bool((ref["out"][c["pair_mask"] == 0] == 0).all()) and bool((ref["out"][c["pair_mask"] != 0].abs().amax(-1) > 0).all())
        p = GC.case("ragged_count_%d_perm" % n)["order"]
        assert p.dtype == torch.int32 and sorted(p.tolist()) == list(range(n))


def test_softmax_case():
    c = GC.case("softmax")
    ref, _ = GC.reference("softmax")
    lg, a, inside = ref["logits"][0], ref["weights"][0], ref["inside"][0]
    for q in range(40):
        kind = GC.SOFTMAX_KINDS[q % 5]
        if kind == "equal":
            assert float((a[q] - 1.0 / 24).abs().max()) < 1e-15
        elif kind == "shift":
            assert float(lg[q].min()) > 2990
        elif kind == "spread":
            assert bool((lg[q].amax(-1) - lg[q].amin(-1) == 200).all())
        elif kind == "dominant_outside":
            dom = a[q] > 0.99
            assert int(dom.sum()) == 3 and not bool(inside[q][dom].any())
            heads = dom.flatten(1).any(1)
            assert float(ref["out"][q].view(8, 32)[heads].abs().max()) < 1e-3 * float(ref["out"].abs().max())
        else:
            assert not bool(inside[q].any()) and bool((ref["out"][q] == 0).all()) and bool((ref["out_A"][q] == 0).all())


# ------------------------------------------------------------------------------------- the cases tell a wrong kernel from a right one
CATCHES = {"sample_clamp": "lattice", "foot_clamp": "footprint", "no_half_pixel": "lattice", "no_grid_clamp": "footprint",
           "natural_view": "levels_3", "ref_level0": "levels_3", "first_footprint": "levels_3", "xw_n_div_b": "batch",
           "softmax_per_level": "levels_3", "order_ignored": "ragged_count_257_perm", "mask_by_slot": "ragged_count_257_perm"}


def test_every_wrong_variant_is_listed():
    assert set(CATCHES) == set(GR.WRONG)


@pytest.mark.parametrize("wrong", sorted(GR.WRONG))
def test_wrong_variant_breaks_its_case(wrong):
    """the deliberately wrong statement exceeds the bf16 bar, and 4 x the fp32 bar, on the named case (bars of the right statement)."""
    name = CATCHES[wrong]
    worst = {}
    for mode, kind, factor in (("f32", "f32", 4.0), ("bf16", "gsamp_bf16", 1.0)):
        ref, k = GC.reference(name, mode)
        bad = GC.evaluate(name, mode, wrong=wrong)
        ratio = (bad["out"] - ref["out"]).abs() / (factor * GR.bar(ref, k, kind)).clamp_min(1e-300)
        worst[kind] = float(ratio.max())
        print("%s on %s: %d of %d elements beyond %g x the %s bar, worst %.3g x" % (wrong, name, int((ratio > 1).sum()), ratio.numel(), factor,
                                                                                   kind, worst[kind]))
    assert worst["f32"] > 1 and worst["gsamp_bf16"] > 1, worst


EDGE_PAIRS = [(n, w) for n in ("lattice_ragged", "thin") for w in ("sample_clamp", "no_half_pixel")] \
    + [(n, w) for n in ("footprint_ragged", "footprint_thin") for w in ("foot_clamp", "no_grid_clamp")]


@pytest.mark.parametrize("name,wrong", EDGE_PAIRS, ids=["%s-%s" % nw for nw in EDGE_PAIRS])
def test_edge_variants_on_the_ragged_pyramids(name, wrong):
    """the sampling variants break the reached lattices, the footprint variants the ragged footprint cases."""
    ref, k = GC.reference(name, "bf16")
    bad = GC.evaluate(name, "bf16", wrong=wrong)
    assert bool(((bad["out"] - ref["out"]).abs() > GR.bar(ref, k, "gsamp_bf16")).any())


# ------------------------------------------------------------------------------------------------------------- k of every case
@pytest.mark.parametrize("name", list(GC.CASES))
def test_yardstick_is_finite_and_inside_its_own_bar(name):
    """k of the G form and of the oa form, fp32 and bf16 operands: finite, printed; the fp32 evaluation of the statement is inside the
    fp32 bar built from its own k, and every error scale is finite."""
    c = GC.case(name)
    for mode in ("f32", "bf16"):
        ref, k = GC.reference(name, mode)
        r32 = GC.evaluate(name, mode, GR.F32)
        assert np.isfinite(k) and bool(torch.isfinite(ref["out_A"]).all()) and bool(torch.isfinite(ref["out"]).all())
        assert bool(((r32["out"].double() - ref["out"]).abs() <= GR.bar(ref, k, "f32")).all())
        _, reff, kf = GC.reference_fused(name, mode)
        assert np.isfinite(kf) and bool(torch.isfinite(reff["out_A"]).all())
        print("%s %s: k %.2f (G form)  %.2f (oa form)" % (name, mode, k, kf))
