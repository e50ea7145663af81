"""Structural triangulation without a GPU: the numpy restatement of the kernel (tests/st_ref.py) against the reference's outputs
(tests/golden/st.npz, made by tests/golden/make_golden_st.py), its properties, the status codes, the ABI and the CPU refusals."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests import st_ref
from tests.golden.st_cases import bone_residual

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# Largest |restatement (fp64, before its rounding to fp32) - reference| over ALL 36 + 18 (scene, method, weights) cases x 4 persons of
# the fixture, in mm, and the bars = 4 x that maximum (the maximum of a noise distribution over some dozens of persons moves from
# set to set):
MEASURED_FP32_REF = 8.204e-3          # against Pose3D_inference_torch (fp32), 15-joint Panoptic tree; its own distance from the truth
BAR_FP32_REF = 4 * MEASURED_FP32_REF  # on noise-free input is up to 8.2e-3 mm
MEASURED_FP64_REF = 2.797e-11         # against Pose3D_inference (fp64 numpy), 17-joint Human3.6M tree
BAR_FP64_REF = 4 * MEASURED_FP64_REF

METHODS = (("LS", "LS", 1), ("ST1", "ST", 1), ("ST3", "ST", 3))


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(os.path.join(HERE, "golden", "st.npz")) as z:
        return {k: z[k] for k in z.files}


def golden_cases():
    """every (scene key, tree, method tag, method, n_steps, weights tag) of the fixture"""
    for name in ("pan", "h36m"):
        for V in (3, 4, 5):
            for noise in (0, 2):
                for tag, method, steps in METHODS:
                    for w in (("w", "u") if name == "pan" else ("w",)):
                        yield "%s_v%d_n%d" % (name, V, noise), name, tag, method, steps, w


def scene_inputs(key):
    g = golden()
    ud, conf, Pm, bl = (g["%s_%s" % (key, k)] for k in ("ud", "conf", "Pm", "bone_len"))
    return ud, conf, np.broadcast_to(Pm, (ud.shape[0],) + Pm.shape), bl


@functools.lru_cache(maxsize=None)
def restated(key, name, method, steps, w):
    ud, conf, Pm, bl = scene_inputs(key)
    return st_ref.solve(ud, conf if w == "w" else None, Pm, golden()[name + "_parent"].tolist(), bl, method, steps, full=True)


def test_restatement_equals_the_reference_outputs():
    g = golden()
    worst = {"pan": 0.0, "h36m": 0.0}
    seen = 0
    for key, name, tag, method, steps, w in golden_cases():
        want = g["%s_%s_%s" % (key, tag, w)]
        assert want.dtype == (np.float32 if name == "pan" else np.float64) and want.shape[0] == 4
        X32, status, X64 = restated(key, name, method, steps, w)
        assert (status == 0).all(), (key, tag, w, status)
        assert np.array_equal(X32, X64.astype(np.float32))
        worst[name] = max(worst[name], float(np.abs(X64 - want.astype(np.float64)).max()))
        seen += want.shape[0]
    print("max |restatement - reference| mm: fp32 reference %.4g (bar %.4g), fp64 reference %.4g (bar %.4g), %d persons"
          % (worst["pan"], BAR_FP32_REF, worst["h36m"], BAR_FP64_REF, seen))
    assert seen == (36 + 18) * 4
    assert worst["pan"] <= BAR_FP32_REF and worst["h36m"] <= BAR_FP64_REF


def test_noise_free_input_reproduces_the_generating_pose():
    g = golden()
    for key, name, tag, method, steps, w in golden_cases():
        if name != "pan" or not key.endswith("_n0"):
            continue
        truth = g[key + "_truth"]
        ours = float(np.abs(restated(key, name, method, steps, w)[0].astype(np.float64) - truth).max())
        ref = float(np.abs(g["%s_%s_%s" % (key, tag, w)].astype(np.float64) - truth).max())
        assert ours <= ref, (key, tag, w, ours, ref)


def test_bone_residual_shrinks_with_the_constraint_and_with_the_steps():
    g = golden()
    for name in ("pan", "h36m"):
        parent = g[name + "_parent"].tolist()
        for V in (3, 4, 5):
            key = "%s_v%d_n2" % (name, V)
            bl = g[key + "_bone_len"]
            res = {tag: bone_residual(restated(key, name, method, steps, "w")[2], parent, bl) for tag, method, steps in METHODS}
            print(key, res)
            assert res["ST3"] < res["ST1"] < res["LS"], (key, res)


def test_status_codes_and_addressing():
    g = golden()
    parent = g["pan_parent"].tolist()
    ud, conf, Pm, bl = (a.copy() for a in scene_inputs("pan_v4_n2"))
    clean, _ = st_ref.solve(ud, conf, Pm, parent, bl, "ST", 3)
    conf[1] = 0.0                                       # a person nobody saw
    ud[2, 1, 7, 0] = np.nan                             # one NaN observation
    X, status = st_ref.solve(ud, conf, Pm, parent, bl, "ST", 3)
    assert status.tolist() == [0, 1, 1, 0]
    assert not X[1].any() and not X[2].any()
    assert np.array_equal(X[0], clean[0]) and np.array_equal(X[3], clean[3])
    # the kernel's two addressings of the same persons: B = 1, the four persons are the queries
    V, J = ud.shape[1], len(parent)
    udq = ud.transpose(1, 0, 2, 3).reshape(1, V, 4 * J, 2)
    cfq = conf.transpose(1, 0, 2).reshape(1, V, 4 * J)
    Xd, sd = st_ref.dense(udq, cfq, Pm[:1], parent, bl[None], valid=np.array([[1, 1, 0, 1]], np.uint8), method="ST", n_steps=3)
    assert sd.tolist() == [[0, 1, -1, 0]] and not Xd[0, 2].any() and np.array_equal(Xd[0, 0], clean[0])
    rows = np.array([[3, 0, 1, 2]], np.int32)
    lengths = bl[None][:, rows[0]]                      # per person: the lengths of the query the row names
    Xr, sr = st_ref.by_rows(udq, cfq, Pm[:1], parent, lengths, rows, np.array([[2, 0]], np.int32), method="ST", n_steps=3)
    assert sr.tolist() == [[0, 0, -1, -1]]              # rows at and behind the count
    assert np.array_equal(Xr[0, 0], clean[3]) and np.array_equal(Xr[0, 1], clean[0]) and not Xr[0, 2:].any()


def test_symbol_is_declared_bound_and_exported():
    from mvgformer_amd import _lib, structural
    src = open(os.path.join(ROOT, "include", "mvg_decoder.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+mvg_structural_triangulate\s*\(", src)
    assert "mvg_structural_triangulate" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["mvg_structural_triangulate"]) == src.split("mvg_structural_triangulate(")[1].split(")")[0].count(",") + 1
    assert set(structural.__all__) == {"PANOPTIC15_PARENT", "H36M17_PARENT", "bone_lengths", "StructuralRefiner"}
    assert list(structural.PANOPTIC15_PARENT) == golden()["pan_parent"].tolist()
    assert list(structural.H36M17_PARENT) == golden()["h36m_parent"].tolist()


def test_bone_lengths_follow_the_tree():
    from mvgformer_amd import structural
    g = golden()
    truth = torch.from_numpy(g["h36m_v3_n0_truth"])
    got = structural.bone_lengths(truth, structural.H36M17_PARENT)
    assert got.shape == (4, 16) and got.dtype == torch.float64
    assert np.allclose(got.numpy(), g["h36m_v3_n0_bone_len"], rtol=1e-6)
    with pytest.raises(ValueError, match="poses"):
        structural.bone_lengths(truth, structural.PANOPTIC15_PARENT)


def test_cpu_tensors_and_bad_arguments_are_refused():
    from mvgformer_amd import _lib, ops, structural
    ud, conf, Pm, bl = (torch.from_numpy(np.ascontiguousarray(a)) for a in scene_inputs("pan_v3_n0"))
    udq = ud.permute(1, 0, 2, 3).reshape(1, 3, 60, 2).contiguous()
    parent = structural.PANOPTIC15_PARENT
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.structural_triangulate(udq, None, Pm[:1], parent, bl[0])
    refiner = structural.StructuralRefiner(batch=1, rows=4, bone_lengths=bl[0], device="cpu")
    assert tuple(refiner.poses.shape) == (1, 4, 15, 3) and refiner.status.tolist() == [[-1] * 4]
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        refiner.update(udq, torch.zeros((3, 48)), Pm[:1], torch.zeros((1, 4), dtype=torch.int32), torch.zeros((1, 2), dtype=torch.int32))
    with pytest.raises(_lib.MvgError, match="not a tree"):
        ops.structural_check((-1, 0, 3, 2))
    with pytest.raises(_lib.MvgError, match="not a tree"):
        ops.structural_check((0, 0, 1))
    with pytest.raises(_lib.MvgError, match="joints"):
        ops.structural_check((-1,) + tuple(range(17)))
    for steps in (0, 9):
        with pytest.raises(_lib.MvgError, match="n_steps"):
            ops.structural_check(parent, steps)
    with pytest.raises(_lib.MvgError, match="unknown method"):
        ops.structural_check(parent, 1, "Lagrangian")
    with pytest.raises(ValueError, match="bone lengths"):
        structural.StructuralRefiner(batch=1, rows=4, bone_lengths=bl[0][:5], device="cpu")
