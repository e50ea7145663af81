"""Seeded inputs of the training-criterion fixtures (tests/golden/criterion.npz): the maker, the CPU tests and the GPU tests all
build them here, so the fixture only has to store what the reference computed from them (plus a checksum of these inputs).

A case = initial query poses (what the matcher sees), per-layer decoder outputs (logits, 3D poses, 2D points), ground truth
(joints_3d, visibilities, num_person) and per-(view, batch element) cameras.  Persons stand inside the space a few hundred to a few
thousand mm apart; some queries start near a person, the rest anywhere in the space, so the K-th and (K+1)-th matching costs of
every person are far apart (the maker asserts it).

A batch element without persons is not among the fixture cases: the reference's matcher raises on it (matcher.py:141-143 reshapes
an empty slice with -1).  EMPTY_CASE describes that case for the tests that compare the kernels with tests/criterion_ref.py."""
import zlib

import numpy as np
import torch

from mvgformer_amd.synthetic import get_scale, ring_cameras

SPACE_SIZE = (8000.0, 8000.0, 2000.0)
SPACE_CENTER = (0.0, -500.0, 800.0)
ORIG_WH = (1920, 1080)
IMG_WH = (960, 512)
J = 15
PRED_CONF_THRESHOLD = 0.5

# name -> B, NQ, Gmax, num_person, V, L, method, value, non-uniform visibility, 2D scale (1e7: the > 1e5 guard)
CASES = {
    "b1":       dict(B=1, NQ=128, Gmax=4, num_person=[3], V=3, L=2, method="KNN", value=5, vis=False, scale2d=1.0, seed=11),
    "b2":       dict(B=2, NQ=128, Gmax=4, num_person=[3, 2], V=3, L=2, method="KNN", value=5, vis=False, scale2d=1.0, seed=12),
    "k3":       dict(B=2, NQ=128, Gmax=4, num_person=[2, 4], V=3, L=1, method="KNN", value=3, vis=False, scale2d=1.0, seed=14),
    "vis":      dict(B=2, NQ=128, Gmax=4, num_person=[3, 2], V=5, L=2, method="KNN", value=5, vis=True, scale2d=1.0, seed=15),
    "guard":    dict(B=1, NQ=128, Gmax=3, num_person=[2], V=3, L=2, method="KNN", value=5, vis=False, scale2d=1.0e7, seed=16),
    "multiple": dict(B=2, NQ=128, Gmax=4, num_person=[3, 2], V=3, L=1, method="multiple", value=100.0, vis=True, scale2d=1.0, seed=17),
    "q1024":    dict(B=1, NQ=1024, Gmax=10, num_person=[5], V=2, L=1, method="KNN", value=5, vis=True, scale2d=1.0, seed=18),
}
EMPTY_CASE = dict(B=2, NQ=128, Gmax=3, num_person=[0, 2], V=3, L=1, method="KNN", value=5, vis=False, scale2d=1.0, seed=13)


def _skeleton(rs):
    """(J, 3) offsets of a person's joints about its centre, mm."""
    return (rs.standard_normal((J, 3)) * np.array([180.0, 180.0, 450.0])).astype(np.float32)


def make_inputs(name):
    """dict of float32 / int64 numpy arrays (see the module docstring); cameras under cam/<key> with shape (V, B, ...).
    name: a key of CASES, "empty", or a case description of the same form (measurement tools)."""
    c = name if isinstance(name, dict) else (EMPTY_CASE if name == "empty" else CASES[name])
    rs = np.random.RandomState(c["seed"])
    B, NQ, Gmax, V, L = c["B"], c["NQ"], c["Gmax"], c["V"], c["L"]
    size, cen = np.array(SPACE_SIZE), np.array(SPACE_CENTER)
    gt = np.zeros((B, Gmax, J, 3), np.float32)
    for b in range(B):
        first = cen + (rs.rand(3) - 0.5) * size * np.array([0.5, 0.5, 0.2])
        for g in range(Gmax):
            # person 1 stands 450 mm from person 0 (shared nearest queries), the others anywhere in the inner space
            if g == 1:
                gt[b, g] = gt[b, 0] + (np.array([450.0, 0.0, 0.0]) + rs.standard_normal((J, 3)) * 30.0).astype(np.float32)
                continue
            ctr = first if g == 0 else cen + (rs.rand(3) - 0.5) * size * np.array([0.7, 0.7, 0.2])
            gt[b, g] = ctr.astype(np.float32) + _skeleton(rs)
    init = np.zeros((B, NQ, J, 3), np.float32)
    for b in range(B):
        for q in range(NQ):
            if q % 8 == 0:          # an eighth of the queries start near a person: at NQ = 128 fewer per person than K = 5
                g = (q // 8) % Gmax
                init[b, q] = gt[b, g] + (rs.standard_normal(3) * 250.0 + rs.standard_normal((J, 3)) * 60.0).astype(np.float32)
            else:
                init[b, q] = (cen + (rs.rand(3) - 0.5) * size).astype(np.float32) + _skeleton(rs)
    out = dict(init_poses=init.reshape(B, NQ * J, 3), joints_3d=gt, num_person=np.array(c["num_person"], np.int64))
    out["logits"] = (rs.standard_normal((L, B, NQ, 2)) * 2.0).astype(np.float32)
    near = gt[:, np.arange(NQ) % Gmax]                                    # (B, NQ, J, 3): every query near some person
    out["poses"] = (near[None] + rs.standard_normal((L, B, NQ, J, 3)) * 120.0).astype(np.float32).reshape(L, B, NQ * J, 3)
    p2 = rs.rand(L, B, V, NQ * J, 2) * np.array(IMG_WH, np.float64)
    out["poses_2d"] = (p2 * c["scale2d"]).astype(np.float32)
    if c["vis"]:
        out["joints_3d_vis"] = np.repeat((rs.rand(B, Gmax, J, 1) > 0.25).astype(np.float32), 3, -1)
        out["joints_vis"] = np.repeat((rs.rand(V, B, Gmax, J, 1) > 0.4).astype(np.float32), 2, -1)
    else:
        out["joints_3d_vis"] = np.ones((B, Gmax, J, 3), np.float32)
        out["joints_vis"] = np.ones((V, B, Gmax, J, 2), np.float32)
    cams = [ring_cameras(V, ORIG_WH, 1400.0, 5500.0, SPACE_CENTER, (-0.28, 0.09, 0.0), (0.0006, -0.0004), seed=c["seed"] + 31 * b)
            for b in range(B)]
    for key in ("R", "T", "fx", "fy", "cx", "cy", "k", "p"):
        out["cam/" + key] = np.stack([np.stack([np.asarray(cams[b][v][key], np.float32) for b in range(B)]) for v in range(V)])
    w, h = ORIG_WH
    out["center"] = np.stack([np.array([w / 2.0, h / 2.0])] * B)                     # float64, as the loader
    out["scale"] = np.stack([get_scale((w, h), IMG_WH)] * B).astype(np.float32)
    return out


def checksum(inputs):
    crc = 0
    for k in sorted(inputs):
        crc = zlib.crc32(np.ascontiguousarray(inputs[k]).tobytes(), crc)
    return np.int64(crc)


def make_meta(inputs, device="cpu", dtype=torch.float32):
    """list[V] of per-view meta dicts in the reference's schema (JointsDataset.py:197-220) for these inputs."""
    from mvgformer_amd.synthetic import crop_affine
    V, B = inputs["joints_vis"].shape[:2]
    inv = np.eye(3)
    inv[:2] = crop_affine(inputs["center"][0], inputs["scale"][0], IMG_WH, inv=True)
    meta = []
    for v in range(V):
        cam = {k: torch.from_numpy(inputs["cam/" + k][v]).to(device=device, dtype=dtype) for k in ("R", "T", "fx", "fy", "cx", "cy", "k", "p")}
        meta.append(dict(camera=cam, center=torch.from_numpy(inputs["center"]).to(device),
                         scale=torch.from_numpy(inputs["scale"]).to(device),
                         inv_affine_trans=torch.from_numpy(np.stack([inv] * B)).to(device),
                         joints_vis=torch.from_numpy(inputs["joints_vis"][v]).to(device=device, dtype=dtype)))
    meta[0].update(joints_3d=torch.from_numpy(inputs["joints_3d"]).to(device=device, dtype=dtype),
                   joints_3d_vis=torch.from_numpy(inputs["joints_3d_vis"]).to(device=device, dtype=dtype),
                   num_person=torch.from_numpy(inputs["num_person"]).to(device))
    return meta
