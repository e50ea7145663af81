"""Pin tests/msda_ref.py (the fp64 statement that tests/test_msda_fp64.py holds the sampling kernels to) against the oracle's autograd,
the C restatement oracle/msda_ref.c and the golden vectors of the reference, and assert without a device that the cases of
tests/msda_cases.py reach the branches they are named for.  CPU only."""
import os

import numpy as np
import pytest
import torch

from oracle import decoder_ref as O
from tests import msda_cases as MC
from tests import msda_ref as R
from tests.golden.cases import msda_case, msda_grad_output

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN = ["small_f32", "ragged_f32", "edge_f32"]


def _rel(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _golden_inputs(name):
    c = msda_case(name)
    N, Lq = c["loc"].shape[:2]
    go = msda_grad_output(name, (N, Lq, c["value"].shape[2] * c["value"].shape[3]))
    return c, go


@pytest.mark.parametrize("name", GOLDEN)
def test_ref_equals_oracle_autograd_and_golden_gradients(name):
    """fp64 coordinates (form "f64": what autograd through the oracle and the reference's own fp64 autograd differentiate): forward and the
    three gradients to 1e-12 of each tensor's scale.  Against the oracle every sample is included, edge_f32's hand-placed rows 0..6 on texel
    borders too (floor gives the one-sided derivative that autograd through the oracle takes); the golden grad_loc comes from the
    reference's grid_sample twin, which takes the OTHER one-sided derivative at an exact border: those seven rows are left out of that one
    comparison, as everywhere else in the suite."""
    c, go = _golden_inputs(name)
    r = R.msda(c["value"], c["shapes"], c["starts"], c["loc"].double(), c["weight"], go, R.F64, "f64")
    v = c["value"].double().requires_grad_(True)
    lo = c["loc"].double().requires_grad_(True)
    w = c["weight"].double().requires_grad_(True)
    y = O.msda_forward(v, c["shapes"], c["starts"], lo, w)
    (y * go.double()).sum().backward()
    g, gm = np.load(os.path.join(GOLD, "grad.npz")), np.load(os.path.join(GOLD, "msda.npz"))
    pre = "msda/%s/" % name
    sl = slice(7, None) if name == "edge_f32" else slice(None)
    for nm, got, want in (("out vs oracle", r["out"], y.detach()), ("out vs msda.npz", r["out"], gm[name + "/out_f64"]),
                          ("grad_value vs autograd", r["grad_value"], v.grad), ("grad_value vs grad.npz", r["grad_value"], g[pre + "grad_value_f64"]),
                          ("grad_loc vs autograd", r["grad_loc"], lo.grad), ("grad_loc vs grad.npz", r["grad_loc"][:, sl], g[pre + "grad_loc_f64"][:, sl]),
                          ("grad_attn vs autograd", r["grad_attn"], w.grad), ("grad_attn vs grad.npz", r["grad_attn"], g[pre + "grad_attn_f64"])):
        e = _rel(got, want)
        print("%s %s: %.2e" % (name, nm, e))
        assert e < 1e-12, (nm, e)


@pytest.mark.parametrize("name", GOLDEN)
def test_ref_equals_the_c_restatement(name):
    """two-rounding fp32 coordinates (form "plain": what a CPU build of oracle/msda_ref.c computes): its double-accumulated backward to
    1e-12 of each tensor's scale on every sample, its fp32 forward within 8 x 2^-24 A + 1 ulp of the fp64 value; and the golden fp32
    forward of the reference's CPU twin within the same bar on the samples that are not ambiguous (the case has none)."""
    from oracle import msda_c
    c, go = _golden_inputs(name)
    r = R.msda(c["value"], c["shapes"], c["starts"], c["loc"], c["weight"], go, R.F64, "plain")
    gv, gl, ga = msda_c.msda_backward(c["value"], c["shapes"], c["starts"], c["loc"], c["weight"], go)
    for nm, got, want in (("grad_value", r["grad_value"], gv), ("grad_loc", r["grad_loc"], gl), ("grad_attn", r["grad_attn"], ga)):
        e = _rel(got, want)
        print("%s %s vs msda_c: %.2e" % (name, nm, e))
        assert e < 1e-12, (nm, e)
    bar = 8.0 * 2.0 ** -24 * r["out_A"] + 2.0 ** -23 * r["out"].abs()
    y = msda_c.msda_forward(c["value"], c["shapes"], c["starts"], c["loc"], c["weight"]).double()
    assert bool(((y - r["out"]).abs() <= bar).all())
    assert int(R.ambiguous(c["loc"], c["shapes"]).sum()) == 0
    y = torch.from_numpy(np.load(os.path.join(GOLD, "msda.npz"))[name + "/out"]).double()
    assert bool(((y - r["out"]).abs() <= bar).all())


def test_fused_and_plain_coordinates_differ_and_ambiguity_sees_it():
    """ly * H - 0.5 as one fused multiply-add and as two roundings: a location a hair below a texel border lands on different cells, and
    `ambiguous` marks that sample and no other."""
    found = None
    for H in range(3, 40):                                   # the fused form resolves the difference finer than the rounded product
        for border in (0.0, 2.0):
            ly = np.float32((border + 0.5) / H)
            for _ in range(8):
                a, b = MC._both(ly, H)
                if np.floor(a) != np.floor(b) and found is None:
                    found = (H, float(ly))
                ly = np.nextafter(ly, np.float32(0), dtype=np.float32)
    assert found is not None
    shapes = torch.tensor([[found[0], 20]])
    found = found[1]
    loc = torch.tensor([[0.4, found], [0.4, 0.3]]).view(1, 2, 1, 1, 1, 2)
    assert R.ambiguous(loc, shapes).flatten().tolist() == [True, False]


# every figure of msda_cases.properties for every case (the seeds are fixed: the counts are exact).  T_total tiles of all levels, bpi bins
# per image, nbins = N * bpi, the largest bin and the number of empty ones, (lead, tail) floats of every image's slice of attn_weight /
# grad_output around its whole 16-byte loads, samples outside their map and ambiguous ones among `samples`.
EXPECT = {
    "one_bin":           dict(T_total=1, bpi=1, nbins=1, bpi_mod32=1, largest_bin=903, empty_bins=0, wgt_lead_tail=[(0, 3)], go_lead_tail=[(0, 0)], out_of_map=0, ambiguous=0, samples=903),
    "odd_heads_a":       dict(T_total=8, bpi=24, nbins=72, bpi_mod32=24, largest_bin=15, empty_bins=43, wgt_lead_tail=[(0, 2), (2, 0), (0, 2)], go_lead_tail=[(0, 0), (0, 0), (0, 0)], out_of_map=0, ambiguous=0, samples=270),
    "odd_heads_b":       dict(T_total=8, bpi=24, nbins=72, bpi_mod32=24, largest_bin=15, empty_bins=43, wgt_lead_tail=[(0, 2), (2, 0), (0, 2)], go_lead_tail=[(0, 0), (0, 0), (0, 0)], out_of_map=0, ambiguous=0, samples=270),
    "many_bins":         dict(T_total=228, bpi=1824, nbins=5472, bpi_mod32=0, largest_bin=10, empty_bins=1881, wgt_lead_tail=[(0, 0), (0, 0), (0, 0)], go_lead_tail=[(0, 0), (0, 0), (0, 0)], out_of_map=4872, ambiguous=0, samples=12288),
    "many_bins_b":       dict(T_total=215, bpi=1720, nbins=5160, bpi_mod32=24, largest_bin=14, empty_bins=1877, wgt_lead_tail=[(0, 0), (0, 0), (0, 0)], go_lead_tail=[(0, 0), (0, 0), (0, 0)], out_of_map=4792, ambiguous=0, samples=12288),
    "ragged":            dict(T_total=16, bpi=32, nbins=64, bpi_mod32=0, largest_bin=67, empty_bins=4, wgt_lead_tail=[(0, 0), (0, 0)], go_lead_tail=[(0, 0), (0, 0)], out_of_map=812, ambiguous=0, samples=1920),
    "lattice":           dict(T_total=6, bpi=6, nbins=6, bpi_mod32=6, largest_bin=40, empty_bins=0, wgt_lead_tail=[(0, 2)], go_lead_tail=[(0, 0)], out_of_map=89, ambiguous=0, samples=242),
    "coincident_centre": dict(T_total=4, bpi=4, nbins=4, bpi_mod32=4, largest_bin=4096, empty_bins=3, wgt_lead_tail=[(0, 0)], go_lead_tail=[(0, 0)], out_of_map=0, ambiguous=0, samples=4096),
    "coincident_corner": dict(T_total=4, bpi=4, nbins=4, bpi_mod32=4, largest_bin=4096, empty_bins=3, wgt_lead_tail=[(0, 0)], go_lead_tail=[(0, 0)], out_of_map=0, ambiguous=0, samples=4096),
    "range":             dict(T_total=9, bpi=72, nbins=216, bpi_mod32=8, largest_bin=281, empty_bins=0, wgt_lead_tail=[(0, 0), (0, 0), (0, 0)], go_lead_tail=[(0, 0), (0, 0), (0, 0)], out_of_map=4551, ambiguous=0, samples=21312),
    "range_zero":        dict(T_total=9, bpi=72, nbins=216, bpi_mod32=8, largest_bin=281, empty_bins=0, wgt_lead_tail=[(0, 0), (0, 0), (0, 0)], go_lead_tail=[(0, 0), (0, 0), (0, 0)], out_of_map=4551, ambiguous=0, samples=21312),
    "nonfinite_loc":     dict(T_total=9, bpi=72, nbins=144, bpi_mod32=8, largest_bin=218, empty_bins=0, wgt_lead_tail=[(0, 0), (0, 0)], go_lead_tail=[(0, 0), (0, 0)], out_of_map=5626, ambiguous=0, samples=14208),
    "nonfinite_go":      dict(T_total=5, bpi=10, nbins=20, bpi_mod32=10, largest_bin=40, empty_bins=0, wgt_lead_tail=[(0, 0), (0, 0)], go_lead_tail=[(0, 0), (0, 0)], out_of_map=0, ambiguous=0, samples=480),
    "generic_d16":       dict(T_total=14, bpi=42, nbins=84, bpi_mod32=10, largest_bin=85, empty_bins=4, wgt_lead_tail=[(0, 3), (1, 2)], go_lead_tail=[(0, 0), (0, 0)], out_of_map=683, ambiguous=0, samples=1998),
    "lattice_d16":       dict(T_total=6, bpi=6, nbins=6, bpi_mod32=6, largest_bin=40, empty_bins=0, wgt_lead_tail=[(0, 2)], go_lead_tail=[(0, 0)], out_of_map=89, ambiguous=0, samples=242),
    "generic_d64":       dict(T_total=14, bpi=42, nbins=84, bpi_mod32=10, largest_bin=85, empty_bins=3, wgt_lead_tail=[(0, 3), (1, 2)], go_lead_tail=[(0, 0), (0, 0)], out_of_map=690, ambiguous=0, samples=1998),
    "lattice_d64":       dict(T_total=6, bpi=6, nbins=6, bpi_mod32=6, largest_bin=40, empty_bins=0, wgt_lead_tail=[(0, 2)], go_lead_tail=[(0, 0)], out_of_map=89, ambiguous=0, samples=242),
    "generic_d12":       dict(T_total=14, bpi=42, nbins=84, bpi_mod32=10, largest_bin=86, empty_bins=4, wgt_lead_tail=[(0, 3), (1, 2)], go_lead_tail=[(0, 0), (0, 0)], out_of_map=662, ambiguous=0, samples=1998),
    "lattice_d12":       dict(T_total=6, bpi=6, nbins=6, bpi_mod32=6, largest_bin=40, empty_bins=0, wgt_lead_tail=[(0, 2)], go_lead_tail=[(0, 0)], out_of_map=89, ambiguous=0, samples=242),
}


@pytest.mark.parametrize("name", list(MC.CASES))
def test_case_properties(name):
    """every figure that decides which branch of the chain a case reaches, for every case, against EXPECT; at most 1 ambiguous sample in
    10 000 (every seed here has none; zero is a condition for the lattice); and what each case is named for."""
    c = MC.case(name)
    p = MC.properties(c)
    print(name, p)
    assert set(EXPECT) == set(MC.CASES) and set(p) == set(EXPECT[name])
    for key, want in EXPECT[name].items():
        assert p[key] == want, (key, p[key], want)
    N = c["value"].shape[0]
    assert p["nbins"] == N * p["bpi"] and p["bpi"] == p["T_total"] * c["value"].shape[2] and p["bpi_mod32"] == p["bpi"] % 32
    assert p["ambiguous"] <= 1e-4 * p["samples"]
    assert all(bool(torch.isfinite(c[k]).all()) for k in ("value", "weight")) and c["value"].dtype == torch.float32
    if name == "one_bin":              # four passes of 256; the last: 135 = 64 + 64 + 7 entries -> an odd number of 8-sample steps
        assert p["largest_bin"] > 3 * MC.BW_PASS and (p["largest_bin"] % MC.BW_PASS) % 64 == 7
    if name.startswith("many_bins"):   # a second chunk of bw_scan; a third of the bins are empty
        assert p["nbins"] > MC.BW_SCAN_CHUNK and p["empty_bins"] > p["nbins"] // 4
        assert (name == "many_bins_b") == (p["T_total"] % 2 == 1)
    if name.startswith("odd_heads"):   # the largest |weight| is in the head of image 1 / the tail of image 2, 8 x the rest
        w = c["weight"].view(3, -1).abs()
        img, sl = (1, slice(0, 2)) if name.endswith("a") else (2, slice(-2, None))
        rest = w[img].clone()
        rest[sl] = 0
        assert float(w[img, sl].max()) == 8.0 and float(rest.max()) <= 1.0
        assert bool(R.msda(c["value"], c["shapes"], c["starts"], c["loc"], c["weight"])["inside"].view(3, -1)[img, sl].all())
    if name == "ragged":
        dims = set(c["shapes"].flatten().tolist())
        assert {1, 5, 7, 8, 9, 17} <= dims and c["shapes"].shape[0] > 4
    if name.startswith("range"):
        s = c["go"].abs().amax((1, 2))
        assert float(c["weight"].abs().max()) > 39.0 and (float(s[0]) == 0.0 if name == "range_zero" else 1e5 < float(s[1] / s[0]) < 1e7)
        assert 1e-31 < float(s[2]) < 1e-29
    if name == "nonfinite_loc":
        bad = ~torch.isfinite(c["loc"]) | (c["loc"].abs() > 1e9)
        assert 0.1 < float(bad.double().mean()) < 0.15 and p["out_of_map"] > 0.2 * p["samples"]
        for x in MC.BAD_LOCS:
            t = torch.tensor(x, dtype=torch.float32)
            assert bool((torch.isnan(c["loc"]) if x != x else (c["loc"] == t)).any())
    if name == "nonfinite_go":
        r = R.msda(c["value"], c["shapes"], c["starts"], c["loc"], c["weight"])
        lh_lw = R.anchors(*R.coordinates(c["loc"], c["shapes"]), c["shapes"])[3:]
        assert bool(r["inside"][0, 3, 1, 0, 0]) and float(lh_lw[0][0, 3, 1, 0, 0]) == 0.0 and float(lh_lw[1][0, 3, 1, 0, 0]) == 0.0
        assert int(c["bad_rows"].sum()) == 4 and int((~torch.isfinite(c["go"])).sum()) == len(MC.NONFINITE_GO)
        assert bool(torch.isfinite(c["go_clean"]).all())
        generic = r["inside"][c["bad_rows"]] & ((lh_lw[0][c["bad_rows"]] > 0) & (lh_lw[1][c["bad_rows"]] > 0))
        assert int(generic.sum()) >= 4


@pytest.mark.parametrize("D", [32, 12])
def test_lattice_reaches_every_edge_with_one_coordinate_in_both_forms(D):
    """every lattice sample: the fused and the two-rounding coordinate are the same float (so no sample is ambiguous and none is left out).
    On the power-of-two dimensions (8, 16) the sets contain -1, -0.5, 0, 7, 7.5, 8, H - 1 and H exactly; the "first floats inside" -1 and H and
    above H - 1 are the nearest coordinates, within 1e-5, on which both forms agree (not always the adjacent float).  On W = 9 the fused form
    cannot give most targets ((t + 0.5) / 9 is no fp32 number): there a coordinate within 1e-5 on EACH side of the target stands in, and that
    is what is asserted."""
    c = MC.case("lattice" if D == 32 else "lattice_d%d" % D)
    hf, wf = R.coordinates(c["loc"], c["shapes"], "fma")
    hp, wp = R.coordinates(c["loc"], c["shapes"], "plain")
    assert torch.equal(hf, hp) and torch.equal(wf, wp)
    assert int(R.ambiguous(c["loc"], c["shapes"]).sum()) == 0
    for l, (H, W) in enumerate(c["shapes"].tolist()):
        for coord, n in ((hf[0, :, 0, l, 0], H), (wf[0, :, 0, l, 0], W)):
            s = sorted(set(coord.tolist()))
            for t in (-1.0, -0.5, 0.0, 7.0, 7.5, 8.0, n - 1.0, float(n)):
                if n & (n - 1) == 0:
                    assert t in s, (l, n, t, s)
                else:           # W = 9: (t + 0.5) / 9 is no fp32 number; the neighbours on both sides
                    assert t in s or (any(t - 1e-5 < x < t for x in s) and any(t < x < t + 1e-5 for x in s)), (l, n, t, s)
            assert any(-1.0 < x < -0.99999 for x in s) and any(n - 1e-5 < x < n for x in s) and any(n - 1.0 < x < n - 1.0 + 1e-5 for x in s)
        # all four combinations of the excluded / included edges occur as (h, w) pairs
        pairs = set(zip(hf[0, :, 0, l, 0].tolist(), wf[0, :, 0, l, 0].tolist()))
        if W & (W - 1) == 0:
            assert {(-1.0, 0.0), (0.0, -1.0), (float(H), 0.0), (0.0, float(W)), (H - 1.0, W - 1.0), (7.0, 8.0), (8.0, 7.0)} <= pairs


# largest k per output kind over the 19 cases as recorded in DESIGN.md 9g (forward: many_bins_b; grad_value: range; grad_loc: lattice_d16;
# grad_attn: generic_d12)
K_RECORDED = dict(out=13.2, grad_value=24.3, grad_loc=11.0, grad_attn=10.4)


def test_yardstick_k_of_every_case():
    """k = 4 x max |ref32 - ref64| / (2^-24 A) per output kind, every case: positive, and at most 2 x the largest figure DESIGN.md records for
    the kind -- k measures the reference, so a jump means that tests/msda_ref.py (or its fp32 evaluation) changed, and the bars with it."""
    worst = dict.fromkeys(MC.KINDS, 0.0)
    for name in MC.CASES:
        _, k = MC.reference(name)
        print("k %-18s %s" % (name, "  ".join("%s %.2f" % kv for kv in k.items())))
        for kind in MC.KINDS:
            assert 0.0 < k[kind] <= 2.0 * K_RECORDED[kind], (name, kind, k[kind])
            worst[kind] = max(worst[kind], k[kind])
    print("largest k:", worst)
    for kind in MC.KINDS:
        assert worst[kind] >= 0.9 * K_RECORDED[kind], (kind, worst[kind])        # the record is the measurement, not a loose ceiling
