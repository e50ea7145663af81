"""CPU checks of the training criterion: the fp64 restatement tests/criterion_ref.py is pinned to what the reference itself
computed (tests/golden/criterion.npz, fp64 columns), the layer weights of decay_method, the ABI table and the wrappers' argument
checks.  No kernel is launched."""
import os

import numpy as np
import pytest
import torch

from tests import criterion_ref as R
from tests.golden import criterion_cases as cc

FIX = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "criterion.npz"))


def restate(name, dtype=torch.float64, device="cpu", affine="fixture"):
    """(pairs, table (L, 7), grads) of the restatement on a fixture case"""
    inp = cc.make_inputs(name)
    if name in cc.CASES:
        assert int(cc.checksum(inp)) == int(FIX[name + "/checksum"]), "inputs of %s differ from the ones the fixture was made from" % name
    t, cam, aff = R.tensors_of(inp, dtype, device, FIX[name + "/affine"] if (affine == "fixture" and name in cc.CASES) else None)
    c = cc.EMPTY_CASE if name == "empty" else cc.CASES[name]
    size = torch.tensor(cc.SPACE_SIZE, dtype=dtype, device=device)
    cen = torch.tensor(cc.SPACE_CENTER, dtype=dtype, device=device)
    pairs = R.match(t["init_poses"], t["joints_3d"], t["num_person"], size, cen, c["method"], c["value"])
    lg, ps, p2 = (t[k].clone().requires_grad_(True) for k in ("logits", "poses", "poses_2d"))
    rows, total = [], 0
    for l in range(c["L"]):
        o = R.criterion_layer(lg[l], ps[l], p2[l], pairs, t["joints_3d"], t["joints_3d_vis"], t["joints_vis"], t["num_person"], cam,
                              aff, size, cen, cc.PRED_CONF_THRESHOLD)
        rows.append(torch.stack([torch.as_tensor(o[k], dtype=dtype, device=device).detach().reshape(()) for k in R.KEYS]))
        total = total + o["loss_ce"] + o["loss_pose_perjoint"] + o["loss_pose_perprojection_2d"]
    grads = torch.autograd.grad(total, [lg, ps, p2], allow_unused=True)
    grads = [torch.zeros_like(x) if g is None else g for g, x in zip(grads, (lg, ps, p2))]
    return pairs, torch.stack(rows), grads


@pytest.mark.parametrize("name", list(cc.CASES))
def test_restatement_equals_the_reference_fp64(name):
    pairs, table, grads = restate(name)
    for b, (q, g) in enumerate(pairs):
        fq, fg = FIX["%s/pairs/%d/query" % (name, b)], FIX["%s/pairs/%d/gt" % (name, b)]
        for person in range(int(cc.CASES[name]["num_person"][b])):
            assert set(q[g == person].tolist()) == set(fq[fg == person].tolist()), (name, b, person)
        assert q.tolist() == fq.tolist() and g.tolist() == fg.tolist()       # no ties in the fixture: the order is defined too
    want = FIX[name + "/table/f64"]
    err = np.abs(table.numpy() - want) / np.maximum(np.abs(want), 1e-30)
    assert err.max() <= 1e-10, (name, err)
    for key, g in zip(("grad_logits", "grad_poses", "grad_poses_2d"), grads):
        w = FIX["%s/%s/f64" % (name, key)]
        assert np.abs(g.numpy() - w).max() <= 1e-10 * max(np.abs(w).max(), 1e-30), (name, key)


def test_fixture_covers_what_it_must():
    assert FIX["b2/shared_queries"] > 0 and FIX["b1/shared_queries"] > 0      # a query among the K nearest of two persons
    assert np.all(FIX["guard/table/f64"][:, 6] == 0) and np.all(FIX["guard/grad_poses_2d/f64"] == 0)
    assert np.abs(FIX["vis/grad_poses_2d/f64"]).max() > 0
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "criterion.npz")) < 1 << 20


def test_weights_order_quirk_is_visible_in_the_vis_case():
    """with non-uniform joints_vis, weighting every row by ITS OWN visibility gives another 2D loss than the reference's"""
    inp = cc.make_inputs("vis")
    t, cam, aff = R.tensors_of(inp, torch.float64, affine=FIX["vis/affine"])
    size, cen = torch.tensor(cc.SPACE_SIZE, dtype=torch.float64), torch.tensor(cc.SPACE_CENTER, dtype=torch.float64)
    pairs = R.match(t["init_poses"], t["joints_3d"], t["num_person"], size, cen, "KNN", 5)
    V = t["joints_vis"].shape[0]
    bi = torch.cat([torch.full_like(q, b) for b, (q, _) in enumerate(pairs)])
    gi = torch.cat([g for _, g in pairs])
    own = torch.stack([t["joints_vis"][v][bi, gi][:, :, 0] for v in range(V)], 1).reshape(-1, cc.J)       # pair-major
    ref = torch.cat([t["joints_vis"][v][bi, gi][:, :, 0] for v in range(V)], 0)                           # view-major
    assert not torch.equal(own, ref)


def test_decay_method_weights():
    assert R.layer_weights("none", 4).tolist() == [1, 1, 1, 1]
    assert torch.allclose(R.layer_weights("linear", 4), torch.tensor([0.25, 0.5, 0.75, 1.0]))
    assert R.layer_weights("exp", 4).tolist() == [0.125, 0.25, 0.5, 1.0]
    assert R.layer_weights("last", 4).tolist() == [0, 0, 0, 1]
    from mvgformer_amd.criterion import layer_weights
    for m in ("none", "linear", "exp", "last"):
        assert torch.allclose(layer_weights(m, 6), R.layer_weights(m, 6))
    with pytest.raises(ValueError):
        layer_weights("cosine", 4)


def test_abi_lists_the_criterion_entry_points():
    from mvgformer_amd import _lib
    for name in ("mvg_knn_match", "mvg_knn_match_workspace", "mvg_criterion", "mvg_criterion_workspace"):
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.mvg_knn_match_workspace(1, 1024, 10) == 0                     # 40 KB of costs: LDS
    assert lib.mvg_knn_match_workspace(2, 1024, 64) == 2 * 1024 * 64 * 4
    assert lib.mvg_criterion_workspace(4, 1, 10, 5, 15) == (10 * 5 * 15 * 2 + 4 * 8) * 8


def test_wrappers_raise_on_cpu_tensors_and_on_hungarian():
    from mvgformer_amd import ops
    from mvgformer_amd.criterion import KNNMatcher
    inp = cc.make_inputs("b1")
    t, _, _ = R.tensors_of(inp, torch.float32)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.knn_match(t["init_poses"], t["joints_3d"], t["num_person"], cc.SPACE_SIZE, cc.SPACE_CENTER, "KNN", 5)
    with pytest.raises(NotImplementedError, match="hungarian"):
        ops.knn_match(t["init_poses"], t["joints_3d"], t["num_person"], cc.SPACE_SIZE, cc.SPACE_CENTER, "hungarian", None)
    with pytest.raises(NotImplementedError, match="hungarian-dis"):
        KNNMatcher("abs", "norm", method="hungarian-dis")
    z = torch.zeros(1)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.criterion(t["logits"], t["poses"], t["poses_2d"], z.int(), z.int(), z.int(), t["joints_3d"], t["joints_3d_vis"],
                      t["joints_vis"], t["num_person"], z, cc.SPACE_SIZE, cc.SPACE_CENTER, 0.5)


def test_factory_builds_matcher_criterion_and_weights_from_every_shipped_yaml():
    import json
    from types import SimpleNamespace as NS
    from mvgformer_amd.criterion import KNNMatcher, SetCriterion
    from mvgformer_amd.factory import build_criterion_from_cfg, build_training_head
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(os.path.dirname(here), "mvgformer_amd", "data", "yaml_extract.json")) as f:
        extract = json.load(f)
    for rel, v in extract.items():
        cfg = NS(DECODER=NS(**v["DECODER"]), NETWORK=NS(IMAGE_SIZE=v["IMAGE_SIZE"]), DATASET=NS(CAMERA_NUM=v["CAMERA_NUM"]),
                 MULTI_PERSON=NS(SPACE_SIZE=v["SPACE_SIZE"], SPACE_CENTER=v["SPACE_CENTER"]))
        crit, wd, decay = build_criterion_from_cfg(cfg)
        d = v["DECODER"]
        assert isinstance(crit, SetCriterion) and isinstance(crit.matcher, KNNMatcher), rel
        assert crit.matcher.method == d["match_method"] == "KNN" and crit.matcher.method_value == d["match_method_value"]
        assert wd == {"loss_ce": d["loss_weight_loss_ce"], "loss_pose_perjoint": d["loss_pose_perjoint"],
                      "loss_pose_perprojection_2d": d["loss_pose_perprojection_2d"], "loss_init": d["loss_weight_init"]}
        assert decay == d.get("decay_method", "none") and crit.pred_conf_threshold == d["pred_conf_threshold"]
        assert crit.grid_size.tolist() == v["SPACE_SIZE"]
    with pytest.raises(NotImplementedError, match="hungarian"):
        build_criterion_from_cfg(NS(DECODER=NS(match_method="hungarian"), NETWORK=cfg.NETWORK, MULTI_PERSON=cfg.MULTI_PERSON))
    from mvgformer_amd.factory import _DECODER_DEFAULTS
    full = NS(DECODER=NS(**{**_DECODER_DEFAULTS, **v["DECODER"]}), NETWORK=cfg.NETWORK, MULTI_PERSON=cfg.MULTI_PERSON, DATASET=cfg.DATASET)
    head, wd = build_training_head(full)
    assert head.criterion is not None and head.decay_method == "none" and set(wd) == {"loss_ce", "loss_pose_perjoint", "loss_pose_perprojection_2d", "loss_init"}
    head.criterion = None
    with pytest.raises(RuntimeError, match="no criterion"):
        head.forward_train([torch.zeros(5, 256, 4, 4)], [{}] * 5)
