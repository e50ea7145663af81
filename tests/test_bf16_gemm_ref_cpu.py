"""The fp64 statement and bound of the bf16 GEMMs (tests/bf16_gemm_ref.py) and the case lists of tests/bf16_gemm_cases.py without a
GPU: the lists reach every k-loop variant of mvg_pyramid_group_ws and every tile shape of mvg_linear (from restatements of the two
launchers), the reference accepts a CPU emulation of the kernels' arithmetic and rejects each of eight defects on the case inputs,
and on every bf16-output case at most 2 % of the elements are straddlers (the elements where the device test cannot insist on bit
equality)."""
import pytest
import torch

from tests import bf16_gemm_cases as Cs
from tests import bf16_gemm_ref as B

CAP = 0.02


def _bad(got, exp, bound):
    """number of elements outside their bound (a NaN counts)."""
    return int((~((got.double() - exp).abs() <= bound)).sum())


def _share(bound):
    return float((bound > 0).double().mean())


# ---------------------------------------------------------------------------------------------------------------- the case lists
def test_pyramid_split_restatement_gives_the_table():
    for (M, jobs, slots), want in Cs.PYR_TABLE.items():
        counts = B.group_tile_counts(M, jobs, slots)
        assert len(counts) == jobs
        assert set().union(*counts) == want, (M, jobs, slots, counts)
        assert any(n_img * S == M and (j, s) == (jobs, slots) for n_img, S, j, s in Cs.PYR_CASES), (M, jobs, slots)
    assert B.group_split(32 * 8 * 64, 8, 64) == (512, [8] * 8) and B.group_split(100000, 3, 0)[1] == [21] * 3


def test_pyramid_cases_cover_every_k_loop_variant():
    """each job kind (head planes, row-major) has workgroups with 0, 1, 2, 3 and >= 4 tiles -- no tile at all, the first tile without
    previous stores, the second with vmcnt(4), the third and later ones with vmcnt(8), and the tail stores -- and ragged last tiles
    of 1 and of 31 rows; images of 1, 5 and 31 pixels (SMALL_S), of 32 and 33, of M / 2, and prime M."""
    seen = {True: set(), False: set()}
    ragged = {True: set(), False: set()}
    for n_img, S, jobs, slots in Cs.PYR_CASES:
        M = n_img * S
        for j, counts in enumerate(B.group_tile_counts(M, jobs, slots)):
            seen[Cs.job_is_planes(j)] |= counts
            ragged[Cs.job_is_planes(j)].add(M % 32)
    for kind in (True, False):
        assert {0, 1, 2, 3} <= seen[kind] and max(seen[kind]) >= 4, seen
        assert {1, 31} <= ragged[kind], ragged
    sizes = {S for _, S, _, _ in Cs.PYR_CASES}
    assert {1, 5, 31, 32, 33} <= sizes and any(n == 2 for n, _, _, _ in Cs.PYR_CASES)
    prime = lambda n: n > 1 and all(n % p for p in range(2, int(n ** 0.5) + 1))
    assert sum(prime(n * S) for n, S, _, _ in Cs.PYR_CASES) >= 3
    assert max(n * S for n, S, _, _ in Cs.PYR_CASES) == 3711 and all(1 <= j <= 8 for _, _, j, _ in Cs.PYR_CASES)


def test_linear_cases_cover_every_tile_shape_and_option():
    """every tile shape with a ragged and a whole last row tile and (128 x 192 has none: N % 192 = 0) a ragged last column tile,
    128 x 128 at M > 64 (knob 0) and 64 x 128 at M <= 64 (knob 2); every option on and off on every tile shape; every M, N, K."""
    assert len(Cs.LIN_CASES) <= 60
    tiles = {(128, 128), (64, 128), (128, 192)}
    seen = {}
    for c in Cs.LIN_CASES:
        t = B.linear_tile(c["M"], c["N"], c["tiles"])
        s = seen.setdefault(t, dict(ragged_m=set(), ragged_n=set(), opts=set(), big_m=False, small_m=False, multi=False))
        s["ragged_m"].add(c["M"] % t[0] != 0)
        s["ragged_n"].add(c["N"] % t[1] != 0)
        s["opts"] |= {(o, c[o]) for o in Cs.LIN_OPTIONS}
        s["big_m"] |= c["M"] > 64
        s["small_m"] |= c["M"] <= 64
        s["multi"] |= c["M"] > t[0] and c["N"] > t[1]
    assert set(seen) == tiles
    for t, s in seen.items():
        assert s["ragged_m"] == {True, False}, (t, s)
        assert s["ragged_n"] == ({False} if t == (128, 192) else {True, False}), (t, s)
        assert s["opts"] == {(o, v) for o in Cs.LIN_OPTIONS for v in (True, False)}, (t, sorted(s["opts"]))
        assert s["big_m"] and s["small_m"] and s["multi"], (t, s)
    for key, vals in (("M", Cs.LIN_M), ("N", Cs.LIN_N), ("K", Cs.LIN_K)):
        assert {c[key] for c in Cs.LIN_CASES} == set(vals)
    assert B.linear_tile(7680, 256) == (64, 128) and B.linear_tile(200000, 256) == (128, 128) and B.linear_tile(64, 256) == (128, 128)


# ------------------------------------------------------------------------------------------------- the reference and its bound
def test_bound_is_zero_away_from_rounding_boundaries():
    """round_err(rms=False) as the bound of a bf16 output: 0 inside a rounding interval, one step where the interval reaches a
    boundary; behind the ReLU an element whose interval is <= 0 is exact; a masked row is exact."""
    x = torch.tensor([[1.0, 0.0], [1.0, 0.0], [-1.0, 0.0], [1.0, 0.0]]).to(Cs.BF)
    W = torch.tensor([[1.0, 0.0]]).to(Cs.BF)
    b = torch.tensor([0.001953125])                     # 1 + 2^-9: a quarter of the way to the next bf16 value, 2^-7 above
    exp, bound = B.expected(x, W, b, relu=True, mask=torch.tensor([1, 1, 1, 0], dtype=torch.uint8))
    assert exp.view(-1).tolist() == [1.0, 1.0, 0.0, 0.0] and bound.view(-1).tolist() == [0.0, 0.0, 0.0, 0.0]
    exp, bound = B.expected(x[:1], W, torch.tensor([0.00390625]))      # 1 + 2^-8: the tie itself
    assert float(bound) == 2.0 ** -7


def _pyr_expected(feat, j, n_img, S):
    W, b, planes = Cs.pyr_job(j)
    return B.expected(feat, W, b)


@pytest.mark.parametrize("c", Cs.PYR_CASES, ids=Cs.pyr_id)
def test_pyramid_defects_are_rejected(c):
    """on every case and job: the clean emulation inside the bound everywhere, every defect outside it somewhere; at most 2 % straddlers."""
    n_img, S, jobs, slots = c
    M = n_img * S
    feat = Cs.pyr_case_feat(c)
    for j in range(jobs):
        W, b, planes = Cs.pyr_job(j)
        exp, bound = B.expected(feat, W, b)
        clean = Cs.emulate(feat, W, b)
        share = _share(bound)
        print("%s job %d (%s): straddlers %.3f %%, clean outside 0" % (Cs.pyr_id(c), j, "planes" if planes else "G", 100 * share))
        assert _bad(clean, exp, bound) == 0
        assert share <= CAP
        defects = ["truncate"] + (["bias_after_round", "bias_group_shift"] if planes else [])
        for d in defects:
            n = _bad(Cs.emulate(feat, W, b, defect=d), exp, bound)
            assert n > 0, (d, j)
        for d in Cs.ROW_DEFECTS:
            if d == "heads_swapped" and not planes:
                continue
            got = Cs.defect_rows(clean, d, n_img, S)
            if got is None:
                assert (d == "ragged_shift" and (M % 32 == 0 or M < 2)) or (d == "stale_tile" and M <= 32), (d, c)
                continue
            assert _bad(got, exp, bound) > 0, (d, j)
    if jobs > 1:                                        # the planes layout itself: a round trip, and one known element
        y = Cs.emulate(feat, *Cs.pyr_job(0)[:2])
        vh = B.to_planes(y, n_img, S)
        assert torch.equal(B.from_planes(vh), y)
        assert vh[n_img - 1, 5, S - 1, 7] == y[M - 1, 5 * 32 + 7]


def test_pyramid_row_defects_occur_in_the_list():
    """the two row defects that need room for them are exercised: a ragged tile of 1 and of 31 rows, a stale tile."""
    done = {"ragged_1": 0, "ragged_31": 0, "stale": 0}
    for n_img, S, jobs, slots in Cs.PYR_CASES:
        M = n_img * S
        z = torch.zeros(M, 256)
        if Cs.defect_rows(z, "ragged_shift", n_img, S) is not None:
            done["ragged_%d" % (M % 32)] = done.get("ragged_%d" % (M % 32), 0) + 1
        done["stale"] += Cs.defect_rows(z, "stale_tile", n_img, S) is not None
    assert done["ragged_1"] >= 3 and done["ragged_31"] >= 3 and done["stale"] >= 10, done


@pytest.mark.parametrize("k", range(len(Cs.LIN_CASES)), ids=[Cs.lin_id(c) for c in Cs.LIN_CASES])
def test_linear_defects_are_rejected(k):
    """on every shape and dtype combination, with the case's options: the clean emulation inside the bound, the defects that apply
    outside it; at most 2 % straddlers on the bf16 outputs."""
    c = Cs.LIN_CASES[k]
    inp = Cs.lin_inputs(c, k)
    for a_dt, o_dt in Cs.DTYPES:
        x = Cs.lin_operand(inp, a_dt)
        ob = o_dt == "bf16"
        kw = dict(out_bf16=ob, relu=c["relu"], mask=inp["mask"])
        exp, bound = B.expected(x, inp["w"], inp["b"], **kw)
        assert _bad(Cs.emulate(x, inp["w"], inp["b"], **kw), exp, bound) == 0, (a_dt, o_dt)
        if ob:
            share = _share(bound)
            print("%s %s->%s: straddlers %.3f %%" % (Cs.lin_id(c), a_dt, o_dt, 100 * share))
            assert share <= CAP, (a_dt, o_dt, share)
        defects = []
        if ob:
            defects.append("truncate")
        if inp["b"] is not None:
            defects += ["bias_group_shift"] + (["bias_after_round"] if ob else []) + (["relu_before_bias"] if c["relu"] else [])
            if inp["mask"] is not None and bool((inp["mask"] == 0).any()):
                defects.append("mask_before_bias")
        for d in defects:
            assert _bad(Cs.emulate(x, inp["w"], inp["b"], defect=d, **kw), exp, bound) > 0, (d, a_dt, o_dt)
    if c["a2"]:                                         # the sum is formed in fp32 and rounded once
        assert torch.equal(Cs.lin_operand(inp, "f32"), (inp["a"] + inp["a2"]).to(Cs.BF))
        assert not torch.equal(Cs.lin_operand(inp, "f32"), Cs.lin_operand(inp, "bf16"))


def test_every_defect_is_exercised_on_the_linear_cases():
    n = {d: 0 for d in Cs.ELEMENT_DEFECTS}
    for k, c in enumerate(Cs.LIN_CASES):
        inp = Cs.lin_inputs(c, k)
        n["truncate"] += 1
        if c["bias"]:
            n["bias_group_shift"] += 1
            n["bias_after_round"] += 1
            n["relu_before_bias"] += c["relu"]
            n["mask_before_bias"] += c["mask"] and bool((inp["mask"] == 0).any())
    assert all(v >= 5 for v in n.values()), n


@pytest.mark.parametrize("relu", [False, True])
def test_mask_and_relu_order_with_a_negative_bias(relu):
    """bias < 0 everywhere.  ReLU in front of the bias leaves negative results: rejected.  The mask in front of the bias leaves
    act(bias) in the masked rows: rejected without ReLU; with ReLU relu(bias) = 0 and the defect cannot show, which is why the
    case list carries biases of both signs (and where it is rejected with ReLU too)."""
    c = dict(M=65, N=136, K=128, a2=False, bias=True, mask=True)
    inp = Cs.lin_inputs(c, 77)
    x = Cs.lin_operand(inp, "bf16")
    neg = -inp["b"].abs() - 0.5
    for ob in (True, False):
        kw = dict(out_bf16=ob, relu=relu, mask=inp["mask"])
        exp, bound = B.expected(x, inp["w"], neg, **kw)
        assert _bad(Cs.emulate(x, inp["w"], neg, **kw), exp, bound) == 0
        if relu:
            assert _bad(Cs.emulate(x, inp["w"], neg, defect="relu_before_bias", **kw), exp, bound) > 0
            assert _bad(Cs.emulate(x, inp["w"], neg, defect="mask_before_bias", **kw), exp, bound) == 0
            exp2, bound2 = B.expected(x, inp["w"], inp["b"], **kw)
            assert _bad(Cs.emulate(x, inp["w"], inp["b"], defect="mask_before_bias", **kw), exp2, bound2) > 0
        else:
            assert _bad(Cs.emulate(x, inp["w"], neg, defect="mask_before_bias", **kw), exp, bound) > 0
        masked = inp["mask"] == 0
        assert bool((exp[masked] == 0).all()) and bool((bound[masked] == 0).all())


def test_tie_case_sits_on_ties():
    """the fp64 results of the tie case are k + 1/2 where bf16 steps by 1; nearest-even differs from truncation AND from rounding
    half away from zero on a good share of them, and the emulation (exact arithmetic) is bit-equal to bf(y)."""
    feat, Wv, bv, Wg = Cs.tie_case()
    for W, b in ((Wv, bv), (Wg, None)):
        y = B.lin(feat, W, b)
        tie = (y >= 128) & (y < 256) & (y - torch.floor(y) == 0.5)
        up = tie & (torch.floor(y) % 2 == 1)
        print("ties %.1f %%, of which rounded up %.1f %%" % (100 * float(tie.double().mean()), 100 * float(up.sum()) / float(tie.sum())))
        assert float(tie.double().mean()) > 0.5 and 0.3 < float(up.sum()) / float(tie.sum()) < 0.7
        assert bool((B.lin(feat.abs(), W.abs(), None if b is None else b.abs()) < 2.0 ** 20).all())     # every partial sum exact in fp32
        assert torch.equal(Cs.emulate(feat, W, b).double(), B.bf(y))
        assert torch.equal(B.bf(y)[tie], torch.where(up, torch.floor(y) + 1, torch.floor(y))[tie])
