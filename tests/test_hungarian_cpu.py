"""CPU checks of the one-to-one ground-truth matcher: the numpy restatement (tests/hungarian_ref.py) against the reference's recorded
pairs (tests/golden/hungarian.npz), against scipy on the restated costs, against brute force, its dual certificate and its tie
rule; and the host side of the new surface (ops.hungarian_match, criterion.HungarianMatcher, factory.build_matcher_from_cfg)."""
import itertools
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import criterion_ref as R
from tests import hungarian_cases as HC
from tests import hungarian_ref as H

HERE = os.path.dirname(os.path.abspath(__file__))
_restated = {}


def restated(name):
    """the restatement's result for a case of the table, computed once"""
    if name not in _restated:
        inp = HC.make_inputs(name)
        _restated[name] = (inp, H.hungarian_match(inp["poses"], inp["joints_3d"], inp["num_person"], HC.SPACE_SIZE, HC.SPACE_CENTER,
                                                  logits=inp["logits"], **HC.match_kwargs(name)))
    return _restated[name]


def golden():
    return np.load(os.path.join(HERE, "golden", "hungarian.npz"))


def test_the_fixture_holds_every_golden_case_and_was_made_from_these_inputs():
    z = golden()
    names = {k.split("/")[0] for k in z.files}
    assert names == set(HC.GOLDEN)
    for name in HC.GOLDEN:
        assert int(z[name + "/checksum"]) == int(HC.checksum(HC.make_inputs(name))), name


@pytest.mark.parametrize("name", HC.GOLDEN)
def test_restatement_equals_the_references_pairs(name):
    z = golden()
    inp, r = restated(name)
    Lm, B = r["pair_count"].shape
    for l in range(Lm):
        for b in range(B):
            G = int(r["pair_count"][l, b])
            assert G == min(int(inp["num_person"][b]), HC.CASES[name]["Gmax"])
            assert r["pair_query"][l, b, :G].tolist() == z["%s/%d/%d/query" % (name, l, b)].tolist(), (name, l, b)
            assert r["pair_gt"][l, b, :G].tolist() == z["%s/%d/%d/gt" % (name, l, b)].tolist(), (name, l, b)
            assert np.all(r["pair_query"][l, b, G:] == -1) and np.all(r["pair_gt"][l, b, G:] == -1)


def test_restated_pose_cost_is_the_criterion_refs_cost_up_to_fp32_summation_order():
    inp = HC.make_inputs("nq257")
    mine = H.pose_costs(inp["poses"][0], inp["joints_3d"], HC.SPACE_SIZE, HC.SPACE_CENTER)                 # (B, Gmax, NQ)
    theirs = R.costs(torch.from_numpy(inp["poses"][0]), torch.from_numpy(inp["joints_3d"]), torch.tensor(HC.SPACE_SIZE),
                     torch.tensor(HC.SPACE_CENTER)).numpy().transpose(0, 2, 1)
    assert mine.dtype == np.float32 and mine.shape == theirs.shape
    # 45 fp32 additions of positive terms: relative error of either order <= 45 * 2^-24
    assert np.abs(mine - theirs).max() <= 2 * 45 * 2.0 ** -24 * np.abs(theirs).max()


def test_restated_round_trip_is_the_criterion_refs_up_to_the_fused_product():
    rs = np.random.RandomState(5)
    x = ((rs.rand(4000, 3) - 0.5) * np.array(HC.SPACE_SIZE) + np.array(HC.SPACE_CENTER)).astype(np.float32)
    mine = H.norm_round_trip_f32(x, HC.SPACE_SIZE, HC.SPACE_CENTER)
    theirs = R.norm_round_trip(torch.from_numpy(x), torch.tensor(HC.SPACE_SIZE), torch.tensor(HC.SPACE_CENTER)).numpy()
    assert mine.dtype == np.float32
    # one rounding of n * size (<= 2^-24 * 8000) less than the unfused form, then the same two additions
    assert np.abs(mine.astype(np.float64) - theirs).max() <= 2.0 ** -24 * 8000.0 * 2
    assert np.mean(mine == theirs) > 0.5
    # the fused multiply-add against exact rational arithmetic
    from fractions import Fraction
    a, b, c = (rs.standard_normal(300).astype(np.float32) * s for s in (1.0, 8000.0, 500.0))
    got = H.fma_f32(a, b, c)
    for i in range(300):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        near = np.float32(float(exact))
        cands = [near, np.nextafter(near, np.float32(np.inf)), np.nextafter(near, np.float32(-np.inf))]
        best = min(abs(Fraction(float(v)) - exact) for v in cands)
        assert abs(Fraction(float(got[i])) - exact) == best, i


@pytest.mark.parametrize("seed", range(12))
def test_restatement_equals_scipy_on_seeded_random_problems(seed):
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    rs = np.random.RandomState(seed)
    G = int(rs.randint(1, 40))
    NQ = G + int(rs.randint(0, 200))
    C = rs.rand(G, NQ) * 100.0 if seed % 2 else rs.standard_normal((G, NQ)) * 10.0
    col, u, v = H.solve(C)
    rows, cols = lsa(C)
    assert rows.tolist() == list(range(G)) and cols.tolist() == col.tolist()
    order = np.argsort(col)
    H.check_certificate(C, G, col[order], order, u, v, seed)


@pytest.mark.parametrize("seed", range(20))
def test_restatement_equals_brute_force(seed):
    rs = np.random.RandomState(100 + seed)
    G = int(rs.randint(1, 5))
    NQ = int(rs.randint(G, 7))
    C = rs.rand(G, NQ)
    col, _, _ = H.solve(C)
    best = min(itertools.permutations(range(NQ), G), key=lambda cols: sum(C[g, q] for g, q in enumerate(cols)))
    assert tuple(col.tolist()) == best


@pytest.mark.parametrize("name", sorted(HC.CASES))
def test_dual_certificate_of_the_restatement(name):
    _, r = restated(name)
    Lm, B = r["pair_count"].shape
    for l in range(Lm):
        for b in range(B):
            H.check_certificate(r["C"][l, b], int(r["pair_count"][l, b]), r["pair_query"][l, b], r["pair_gt"][l, b], r["u"][l, b],
                                r["v"][l, b], (name, l, b))


def test_counts_clamp_and_empty_elements():
    _, r = restated("counts")
    assert r["pair_count"][0].tolist() == [0, 6, 3] and r["matched"][0].sum(1).tolist() == [0, 6, 3]
    _, r = restated("clamp")
    assert r["pair_count"][0].tolist() == [6, 6]


@pytest.mark.parametrize("name", sorted(HC.TIE_CASES))
def test_tie_rule_on_integer_coordinates(name):
    t = HC.TIE_CASES[name]
    inp = HC.tie_inputs(name)
    r = H.hungarian_match(inp["poses"], inp["joints_3d"], inp["num_person"], *HC.TIE_SPACE, method="hungarian-dis")
    G = len(t["persons"])
    assert list(zip(r["pair_query"][0, :G].tolist(), r["pair_gt"][0, :G].tolist())) == t["pairs"]
    C = r["C"][0]
    assert np.array_equal(C * 100.0, np.round(C * 100.0))                    # the costs are the exact hundredths written down
    H.check_certificate(C, G, r["pair_query"][0], r["pair_gt"][0], r["u"][0], r["v"][0], name)


def test_wrappers_raise_on_cpu_tensors():
    from mvgformer_amd import ops
    from mvgformer_amd.criterion import HungarianMatcher
    inp = HC.make_inputs("nq70")
    t = {k: torch.from_numpy(v) for k, v in inp.items()}
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.hungarian_match(t["poses"][0], t["joints_3d"], t["num_person"], HC.SPACE_SIZE, HC.SPACE_CENTER, logits=t["logits"][0])
    with pytest.raises(ValueError, match="KNN"):
        ops.hungarian_match(t["poses"][0], t["joints_3d"], t["num_person"], HC.SPACE_SIZE, HC.SPACE_CENTER, method="KNN")
    m = HungarianMatcher()
    m.grid_size, m.grid_center = torch.tensor(HC.SPACE_SIZE), torch.tensor(HC.SPACE_CENTER)
    meta = [dict(joints_3d=t["joints_3d"], num_person=t["num_person"])]
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        m.match(t["poses"][0], meta, logits=t["logits"][0])
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        m({"pred_logits": t["logits"][0], "pred_poses": {"outputs_coord": t["poses"][0]}}, meta)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        m.match(t["poses"][0], meta, method="KNN", value=5)                  # the reference's class in full: KNN delegates


def test_matcher_defaults_and_factory():
    import mvgformer_amd
    from mvgformer_amd.criterion import HungarianMatcher, KNNMatcher
    from mvgformer_amd.factory import build_criterion_from_cfg, build_matcher_from_cfg, build_training_head
    assert mvgformer_amd.HungarianMatcher is HungarianMatcher and mvgformer_amd.build_matcher_from_cfg is build_matcher_from_cfg
    m = HungarianMatcher()
    assert m.method == "hungarian" and m.method_value is None and m.uses_logits
    assert (m.cost_class, m.cost_pose, m.cost_giou) == (1, 1, 1)
    assert not getattr(KNNMatcher("abs", "norm"), "uses_logits", False)
    m = HungarianMatcher("abs", "norm", 2.0, 5.0, 1.0, "hungarian-dis", 7)   # the reference's positional order
    assert (m.cost_class, m.cost_pose, m.method, m.method_value) == (2.0, 5.0, "hungarian-dis", 7)
    with pytest.raises(NotImplementedError, match="match_coord_est"):
        HungarianMatcher("norm", "norm")
    with pytest.raises(NotImplementedError, match="match_coord_gt"):
        HungarianMatcher("abs", "abs")
    with pytest.raises(ValueError, match="nearest"):
        HungarianMatcher(method="nearest")
    bare = NS(DECODER=NS(), NETWORK=NS(IMAGE_SIZE=[960, 512]),
              MULTI_PERSON=NS(SPACE_SIZE=list(HC.SPACE_SIZE), SPACE_CENTER=list(HC.SPACE_CENTER)))
    m = build_matcher_from_cfg(bare)
    assert isinstance(m, HungarianMatcher) and m.method == "hungarian" and (m.cost_class, m.cost_pose) == (2.0, 5.0)
    assert build_matcher_from_cfg(NS(DECODER=NS(match_method="KNN", match_method_value=3))).method_value == 3
    hcfg = NS(DECODER=NS(match_method="hungarian", pred_conf_threshold=0.5), NETWORK=bare.NETWORK, MULTI_PERSON=bare.MULTI_PERSON)
    crit, wd, decay = build_criterion_from_cfg(hcfg, matcher=m)
    assert crit.matcher is m and m.grid_size.tolist() == list(HC.SPACE_SIZE) and decay == "none"
    with pytest.raises(NotImplementedError, match="hungarian"):              # without a matcher: as before
        build_criterion_from_cfg(hcfg)
    from mvgformer_amd.factory import _DECODER_DEFAULTS
    full = NS(DECODER=NS(**{**_DECODER_DEFAULTS, "num_decoder_layers": 1, "num_instance": 16, "match_method": "hungarian",
                            "pred_conf_threshold": 0.5}),
              NETWORK=bare.NETWORK, MULTI_PERSON=bare.MULTI_PERSON, DATASET=NS(CAMERA_NUM=3))
    head, _ = build_training_head(full, matcher=m)
    assert head.criterion.matcher is m
    with pytest.raises(NotImplementedError, match="hungarian"):
        build_training_head(full)


def test_per_layer_matching_needs_a_hungarian_matcher():
    from mvgformer_amd.criterion import KNNMatcher, SetCriterion, criterion_all_layers
    cfg = NS(DECODER=NS(pred_conf_threshold=0.5), NETWORK=NS(IMAGE_SIZE=[960, 512]),
             MULTI_PERSON=NS(SPACE_SIZE=list(HC.SPACE_SIZE), SPACE_CENTER=list(HC.SPACE_CENTER)))
    crit = SetCriterion(2, KNNMatcher("abs", "norm", method="KNN", method_value=5), {}, ["joints", "labels", "cardinality"], cfg)
    z = torch.zeros(1, 1, 4, 2)
    with pytest.raises(ValueError, match="HungarianMatcher"):
        criterion_all_layers(crit, z, torch.zeros(1, 1, 4, 3), torch.zeros(1, 1, 1, 4, 2), [{}], None)


def test_abi_table_and_workspace():
    from mvgformer_amd import _lib, ops
    assert "mvg_hungarian_match" in _lib.SIGNATURES and "mvg_hungarian_match_workspace" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["mvg_hungarian_match"]) == 25
    assert ops.HUNGARIAN_METHODS == {"hungarian": 2, "hungarian-dis": 3} and ops.MATCH_METHODS == {"KNN": 0, "multiple": 1}
    lib = _lib.load()
    assert lib.mvg_hungarian_match_workspace(1, 1024, 10) == 0
    assert lib.mvg_hungarian_match_workspace(1, 4096, 64) == 4096 * 64 * 4
    assert lib.mvg_hungarian_match_workspace(8, 4096, 64) == 8 * 4096 * 64 * 4
    assert lib.mvg_hungarian_match_workspace(0, 1024, 10) == 0
