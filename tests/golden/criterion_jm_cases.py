"""Seeded inputs of the joint-map fixtures of the training criterion (tests/golden/criterion_jm.npz): the Shelf / Campus joint
format, where the predictions keep the decoder's JP = 15 Panoptic joints per query and the ground truth has Jc = len(joint_map)
joints per person, converted joint j being prediction joint joint_map[j] (DECODER.convert_joint_format_indices).

The inputs are those of tests/golden/criterion_cases.make_inputs for the case's description; the ground truth (joints_3d and both
visibilities) is then gathered with the map, so a person's converted joints are where its Panoptic joints are.  The predictions --
init_poses, poses, poses_2d -- stay UNconverted, 15 joints per query: the maker gathers them as the reference does, the kernels
take them as they are."""
import numpy as np

from tests.golden import criterion_cases as cc
from tests.golden.criterion_cases import (IMG_WH, PRED_CONF_THRESHOLD, SPACE_CENTER, SPACE_SIZE, checksum,  # noqa: F401
                                          make_meta)

JP = cc.J
SHELF_MAP = (14, 13, 12, 6, 7, 8, 11, 10, 9, 3, 4, 5, 0, 1)        # configs/shelf_campus/*.yaml; joint 2 is not named
PERM15 = (3, 14, 0, 9, 7, 12, 1, 5, 10, 2, 13, 6, 11, 4, 8)        # all 15 joints, no fixed point pattern of the identity

# name -> the description of criterion_cases.CASES + the joint map
CASES = {
    "shelf":    dict(B=2, NQ=128, Gmax=4, num_person=[3, 2], V=3, L=2, method="KNN", value=5, vis=True, scale2d=1.0, seed=41,
                     joint_map=SHELF_MAP),
    "multiple": dict(B=2, NQ=128, Gmax=4, num_person=[3, 2], V=3, L=2, method="multiple", value=100.0, vis=True, scale2d=1.0,
                     seed=41, joint_map=SHELF_MAP),
    "perm15":   dict(B=2, NQ=128, Gmax=4, num_person=[3, 2], V=3, L=2, method="KNN", value=5, vis=True, scale2d=1.0, seed=43,
                     joint_map=PERM15),
    # one joint: costs are sums of 3 terms, a few mm apart between neighbours; the seed is one whose margin is > 1e-2 (the maker
    # asserts it)
    "one":      dict(B=2, NQ=128, Gmax=4, num_person=[3, 2], V=3, L=2, method="KNN", value=5, vis=True, scale2d=1.0, seed=54,
                     joint_map=(7,)),
    "q1024":    dict(B=1, NQ=1024, Gmax=10, num_person=[5], V=2, L=1, method="KNN", value=5, vis=True, scale2d=1.0, seed=45,
                     joint_map=SHELF_MAP),
    # 1024 x 11 costs: past the matcher's LDS table, into its workspace
    "q1024g11": dict(B=1, NQ=1024, Gmax=11, num_person=[6], V=2, L=1, method="KNN", value=5, vis=True, scale2d=1.0, seed=46,
                     joint_map=SHELF_MAP),
    "guard":    dict(B=1, NQ=128, Gmax=3, num_person=[2], V=3, L=2, method="KNN", value=5, vis=False, scale2d=1.0e7, seed=47,
                     joint_map=SHELF_MAP),
}


def make_inputs(name):
    """criterion_cases.make_inputs with the ground truth in the converted joint format; name: a key of CASES or a description"""
    c = name if isinstance(name, dict) else CASES[name]
    out = cc.make_inputs({k: v for k, v in c.items() if k != "joint_map"})
    jm = list(c["joint_map"])
    out["joints_3d"] = np.ascontiguousarray(out["joints_3d"][:, :, jm])
    out["joints_3d_vis"] = np.ascontiguousarray(out["joints_3d_vis"][:, :, jm])
    out["joints_vis"] = np.ascontiguousarray(out["joints_vis"][:, :, :, jm])
    return out


def gather(x, joint_map, nq):
    """(..., NQ*JP, C) predictions -> (..., NQ*Jc, C): the gather of dq_transformer.py:97-101, 582-590 (torch or numpy)"""
    lead, ch = tuple(x.shape[:-2]), x.shape[-1]
    return x.reshape(lead + (nq, JP, ch))[..., list(joint_map), :].reshape(lead + (nq * len(joint_map), ch))


def scatter(g, joint_map, nq):
    """the adjoint of gather for torch tensors: (..., NQ*Jc, C) gradients -> (..., NQ*JP, C), zeros at joints the map does not name"""
    lead, ch = tuple(g.shape[:-2]), g.shape[-1]
    full = g.new_zeros(lead + (nq, JP, ch))
    full[..., list(joint_map), :] = g.reshape(lead + (nq, len(joint_map), ch))
    return full.reshape(lead + (nq * JP, ch))
