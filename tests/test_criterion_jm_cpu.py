"""CPU checks of the joint map of the training criterion (Shelf / Campus joint format): the fp64 restatement
tests/criterion_ref.py, applied to predictions gathered with the map and with its gradients carried back through the gather, is
pinned to what the reference itself computed (tests/golden/criterion_jm.npz, fp64 columns; the bars of test_criterion_cpu.py);
the ABI of the two new entry points; the wrappers' checks of the map; the factory on the two shelf_campus YAMLs.  No kernel is
launched."""
import os
import re

import numpy as np
import pytest
import torch

from tests import criterion_ref as R
from tests.golden import criterion_jm_cases as jc

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = np.load(os.path.join(HERE, "golden", "criterion_jm.npz"))
SHELF_YAML = "configs/shelf_campus/shelf_knn5-lr4-q1024.yaml"
CAMPUS_YAML = "configs/shelf_campus/campus_knn5-lr4-q1024.yaml"


def restate(name, dtype=torch.float64, device="cpu"):
    """(pairs, table (L, 7), grads in the UNconverted 15-joint shape) of the restatement on a joint-map fixture case"""
    c = jc.CASES[name]
    jm, NQ = list(c["joint_map"]), c["NQ"]
    inp = jc.make_inputs(name)
    assert int(jc.checksum(inp)) == int(FIX[name + "/checksum"]), "inputs of %s differ from the ones the fixture was made from" % name
    t, cam, aff = R.tensors_of(inp, dtype, device, FIX[name + "/affine"])
    size = torch.tensor(jc.SPACE_SIZE, dtype=dtype, device=device)
    cen = torch.tensor(jc.SPACE_CENTER, dtype=dtype, device=device)
    pairs = R.match(jc.gather(t["init_poses"], jm, NQ), t["joints_3d"], t["num_person"], size, cen, c["method"], c["value"])
    lg, ps, p2 = (t[k].clone().requires_grad_(True) for k in ("logits", "poses", "poses_2d"))
    psc, p2c = jc.gather(ps, jm, NQ), jc.gather(p2, jm, NQ)                  # autograd scatters the gradients back
    rows, total = [], 0
    for l in range(c["L"]):
        o = R.criterion_layer(lg[l], psc[l], p2c[l], pairs, t["joints_3d"], t["joints_3d_vis"], t["joints_vis"], t["num_person"], cam,
                              aff, size, cen, jc.PRED_CONF_THRESHOLD)
        rows.append(torch.stack([torch.as_tensor(o[k], dtype=dtype, device=device).detach().reshape(()) for k in R.KEYS]))
        total = total + o["loss_ce"] + o["loss_pose_perjoint"] + o["loss_pose_perprojection_2d"]
    grads = torch.autograd.grad(total, [lg, ps, p2], allow_unused=True)
    grads = [torch.zeros_like(x) if g is None else g for g, x in zip(grads, (lg, ps, p2))]
    return pairs, torch.stack(rows), grads


@pytest.mark.parametrize("name", list(jc.CASES))
def test_restatement_on_gathered_predictions_equals_the_reference_fp64(name):
    pairs, table, grads = restate(name)
    for b, (q, g) in enumerate(pairs):
        fq, fg = FIX["%s/pairs/%d/query" % (name, b)], FIX["%s/pairs/%d/gt" % (name, b)]
        assert q.tolist() == fq.tolist() and g.tolist() == fg.tolist()
    want = FIX[name + "/table/f64"]
    err = np.abs(table.numpy() - want) / np.maximum(np.abs(want), 1e-30)
    assert err.max() <= 1e-10, (name, err)
    for key, g in zip(("grad_logits", "grad_poses", "grad_poses_2d"), grads):
        w = FIX["%s/%s/f64" % (name, key)]
        assert g.shape == w.shape
        assert np.abs(g.numpy() - w).max() <= 1e-10 * max(np.abs(w).max(), 1e-30), (name, key)


def test_fixture_covers_what_it_must():
    assert jc.CASES["shelf"]["joint_map"] == (14, 13, 12, 6, 7, 8, 11, 10, 9, 3, 4, 5, 0, 1)
    assert sorted(jc.CASES["perm15"]["joint_map"]) == list(range(15)) and list(jc.CASES["perm15"]["joint_map"]) != list(range(15))
    assert jc.CASES["one"]["joint_map"] != (0,) and len(jc.CASES["one"]["joint_map"]) == 1
    assert jc.CASES["multiple"]["method"] == "multiple" and sum(len(FIX["multiple/pairs/%d/query" % b]) for b in range(2)) > 0
    from mvgformer_amd import _lib
    lib = _lib.load()
    assert lib.mvg_knn_match_workspace(1, 1024, 10) == 0 and lib.mvg_knn_match_workspace(1, 1024, 11) > 0
    assert FIX["shelf/shared_queries"] > 0
    for name, c in jc.CASES.items():
        # the stored gradients are those of the UNconverted tensors: 15 joints, zeros where the map names no joint
        for key, ch in (("grad_poses", 3), ("grad_poses_2d", 2)):
            g = FIX["%s/%s/f64" % (name, key)]
            assert g.shape[-2:] == (c["NQ"] * jc.JP, ch)
            g = g.reshape(g.shape[:-2] + (c["NQ"], jc.JP, ch))
            unnamed = [j for j in range(jc.JP) if j not in c["joint_map"]]
            assert not np.any(g[..., unnamed, :]), (name, key)
            if name != "guard" or key == "grad_poses":
                assert np.abs(g[..., list(c["joint_map"]), :]).max() > 0, (name, key)
    assert np.all(FIX["guard/table/f64"][:, 6] == 0) and np.all(FIX["guard/grad_poses_2d/f64"] == 0)
    assert os.path.getsize(os.path.join(HERE, "golden", "criterion_jm.npz")) < 1 << 20


def test_header_declares_the_joint_map_entry_points_and_the_ctypes_table_matches():
    import ctypes as C
    from mvgformer_amd import _lib
    with open(os.path.join(os.path.dirname(HERE), "include", "mvg_decoder.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    ctype_of = {"int": C.c_int, "float": C.c_float, "size_t": C.c_size_t}
    for name in ("mvg_knn_match_jm", "mvg_criterion_jm"):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, "%s is not declared in include/mvg_decoder.h" % name
        args = [a.strip() for a in m.group(1).split(",")]
        want = [_lib.TensorPtr if "*" in a else ctype_of[a.split()[0]] for a in args]      # the table's type of a device pointer
        assert _lib.SIGNATURES[name] == want, name
        assert any(re.fullmatch(r"const int\s*\*\s*joint_map", a) for a in args) and "int Jp" in args and "int Jc" in args
        assert hasattr(_lib.load(), name)
    # the map-less declarations are what they were
    assert re.search(r"int Gmax, int J, int Pmax,\s*void\* workspace", src) and re.search(r"int NQ,\s*int J, int V, int Gmax, int Pmax", src)


def _cpu_case():
    inp = jc.make_inputs("shelf")
    t, _, _ = R.tensors_of(inp, torch.float32)
    return t


@pytest.fixture
def no_library(monkeypatch):
    """any attempt to reach the library fails the test: the map has to be rejected before"""
    from mvgformer_amd import _lib

    def load():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "load", load)


@pytest.mark.parametrize("bad,exc", [([14, 13, 12, 6, 7, 8, 11, 10, 9, 3, 4, 5, 0, 0], ValueError),       # repeated entry
                                     ([14, 13, 12, 6, 7, 8, 11, 10, 9, 3, 4, 5, 0, 15], ValueError),      # entry == Jp
                                     ([14, 13, 12, 6, 7, 8, 11, 10, 9, 3, 4, 5, -1, 1], ValueError),
                                     ([14, 13, 12, 6, 7, 8, 11, 10, 9, 3, 4, 5, 0], RuntimeError),        # 13 entries, 14 gt joints
                                     (list(range(15)), RuntimeError)])
def test_wrappers_reject_a_bad_joint_map_before_any_library_call(bad, exc, no_library):
    from mvgformer_amd import ops
    t = _cpu_case()
    with pytest.raises(exc, match="joint_map"):
        ops.knn_match(t["init_poses"], t["joints_3d"], t["num_person"], jc.SPACE_SIZE, jc.SPACE_CENTER, "KNN", 5, joint_map=bad,
                      num_joints=jc.JP)
    z = torch.zeros((2, 20), dtype=torch.int32)
    with pytest.raises(exc, match="joint_map"):
        ops.criterion(t["logits"], t["poses"], t["poses_2d"], z, z, z[:, 0], t["joints_3d"], t["joints_3d_vis"], t["joints_vis"],
                      t["num_person"], torch.zeros((6, 48)), jc.SPACE_SIZE, jc.SPACE_CENTER, 0.5, joint_map=bad)


def test_wrappers_with_a_good_map_still_refuse_cpu_tensors_and_a_map_without_the_joint_count():
    from mvgformer_amd import ops
    t = _cpu_case()
    jm = list(jc.SHELF_MAP)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.knn_match(t["init_poses"], t["joints_3d"], t["num_person"], jc.SPACE_SIZE, jc.SPACE_CENTER, "KNN", 5, joint_map=jm,
                      num_joints=jc.JP)
    with pytest.raises(ValueError, match="joints per query"):
        ops.knn_match(t["init_poses"], t["joints_3d"], t["num_person"], jc.SPACE_SIZE, jc.SPACE_CENTER, "KNN", 5, joint_map=jm)


@pytest.mark.parametrize("rel", [SHELF_YAML, CAMPUS_YAML])
def test_factory_builds_the_training_head_of_the_shelf_campus_yamls(rel):
    from mvgformer_amd import validate
    from mvgformer_amd.factory import build_training_head
    cfg = validate.load_config("extract:" + rel)
    assert cfg.DECODER.optimizer == "adamw"
    head, weight_dict = build_training_head(cfg)
    assert head.convert_joint_format_indices == list(jc.SHELF_MAP) and head.num_joints == 15
    assert weight_dict["loss_ce"] == 0.0 and head.criterion.weight_dict["loss_ce"] == 0.0
    assert weight_dict["loss_pose_perjoint"] > 0 and head.criterion.matcher.method == "KNN"


def test_forward_train_no_longer_refuses_the_joint_format():
    """the refusal was the second statement of forward_train; with the map it gets as far as the device work"""
    from mvgformer_amd import validate
    from mvgformer_amd.factory import build_training_head
    head, _ = build_training_head(validate.load_config("extract:" + SHELF_YAML))
    with pytest.raises(Exception) as e:
        head.forward_train([torch.zeros(5, 256, 4, 4)], [{}] * 5)
    assert not isinstance(e.value, NotImplementedError), e.value


def test_validate_actor_ground_truth_and_pcp_row():
    from mvgformer_amd import evaluate as E
    from mvgformer_amd import validate
    rs = np.random.RandomState(3)
    gts = [rs.standard_normal((3, 14, 3)) * 300 + np.array([0, 0, 1000.0]) for _ in range(2)]
    vis = [np.ones((3, 14, 3)), np.ones((3, 14, 3))]
    vis[1][2] = 0                                                   # actor 2 is not annotated in frame 1
    actors = validate.actor_ground_truth(gts, vis)
    assert len(actors) == 3 and actors[2][1] is None and np.array_equal(actors[1][1], gts[1][1])
    kept = []
    for f in range(2):
        p = np.zeros((3, 14, 5))
        p[:, :, :3] = gts[f] + rs.standard_normal((3, 14, 3)) * (5.0 if f == 0 else 400.0)
        p[:, :, 4] = 0.9
        kept.append(torch.from_numpy(p))
    row = validate.pcp_report(kept, gts, vis)
    actor, avg, bones, recall = E.evaluate_pcp(kept, actors)
    assert row["actor"] == [round(100 * float(a), 2) for a in actor] and row["average"] == round(100 * float(avg), 2)
    assert row["recall500"] == round(100 * float(recall), 2) and set(row["bones"]) == set(E.PCP_BONE_GROUPS)
    assert row["bones"]["Head"] == [round(100 * float(x), 2) for x in bones["Head"]]
    assert 0 < row["average"] < 100
    empty = [k[:0] for k in kept]
    assert "error" in validate.pcp_report(empty, gts, vis)
