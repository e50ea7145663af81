"""Pin the fp64 statement of the triangulation kernel (tests/tri_ref.py) to the oracle's chain (oracle/decoder_ref.py: undistort_points,
projection_matrices, dlt_triangulate on softmax confidences) and check on the CPU what the inputs of tests/test_tri_fp64.py
(tests/tri_cases.py) must satisfy for the GPU tests to mean something.  No device.

Two properties are NOT what one would guess, and are asserted as they are (figures: DESIGN.md section 9s):
  * noise2 (2 px) does not settle at sigma = 0: l0 / l1 is ~1e-3 there, the first round of 4 solves leaves ~1e-9 against the 1e-11 test, and
    the routine takes its shift after round one.  Only `meet` is "first"; noise2, off30 and off300 are "shifted".
  * exp(-100) = 3.8e-44 is an fp32 subnormal, not 0: the ramp to -100 ends in a subnormal weight, the ramp to -120 in an exact 0."""
import collections
import os

import numpy as np
import pytest
import torch

from mvgformer_amd import ops
from mvgformer_amd import synthetic as S
from oracle import decoder_ref as O
from tests import tri_cases as C
from tests import tri_ref as T
from tests.geom_cases import dlt_reference
from tests.golden.cases import LAYER_CASES

F64, F32 = torch.float64, torch.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
rel = lambda a, b: float((a - b).abs().max() / b.abs().max())


def _cam_of_records(rec, V, B):
    c = rec.double().view(V, B, 48).transpose(0, 1)
    return dict(R=c[..., 0:9].reshape(B, V, 3, 3), T=c[..., 9:12].reshape(B, V, 3, 1), fx=c[..., 12], fy=c[..., 13], cx=c[..., 14],
                cy=c[..., 15], k=c[..., 16:19].reshape(B, V, 3, 1), p=c[..., 19:21].reshape(B, V, 2, 1))


def _oracle_chain(r, o, rec, V, B, Lq):
    """the oracle's functions on the same (r, o): (X (B, Lq, 3), rows (B, Lq, 2V, 4), ud, Pm, conf), all fp64."""
    c = rec.double().view(V, B, 48).transpose(0, 1)
    rr = r.double().view(V, B, Lq, 2).transpose(0, 1)
    oo = o.double().view(V, B, Lq, 3).transpose(0, 1)
    img = c[:, :, None, 36:38]
    kp = (rr + oo[..., :2] / img) * img
    Ainv = c[..., 27:33].reshape(B, V, 2, 3)
    uo = torch.matmul(torch.cat([kp, torch.ones_like(kp[..., :1])], -1), Ainv.transpose(2, 3))
    cam = _cam_of_records(rec, V, B)
    ud = O.undistort_points(uo, cam, F64)
    Pm = O.projection_matrices(cam, F64)
    conf = torch.softmax(oo[..., 2], 1)
    X, A = O.dlt_triangulate(Pm, ud, conf)
    return X, A, ud, Pm, conf


def test_statement_matches_the_oracle_on_the_golden_arrays():
    """the arrays of test_triangulation_kernel_vs_reference_golden (tri_kp, tri_conf, tri_undist, tri_points3d of mini5_all), fed as
    r = crop(kp) / img, zero offsets and logit = log(conf)."""
    g = np.load(os.path.join(GOLD, "mini5_all.npz"))
    spec = LAYER_CASES["mini5_all"]
    case = S.build_case(spec["config"], B=spec.get("B", 1), seed=spec["seed"], NQ=spec.get("NQ"), layers=spec.get("layers"),
                        valid_fraction=spec.get("valid_fraction"), with_features=False)
    rec = ops.pack_cameras(case.meta, case.img_size, "cpu")
    n, V, J = g["tri_kp"].shape[:3]
    kp = torch.from_numpy(g["tri_kp"]).double()
    A = O.crop_affine_matrix(case.meta[0]["center"], case.meta[0]["scale"], case.img_size, F64)[0]
    net = kp @ A[:, :2].t() + A[:, 2]
    r = (net / torch.tensor(case.img_size, dtype=F64)).permute(1, 0, 2, 3).reshape(V, n * J, 2)
    conf = torch.from_numpy(g["tri_conf"]).double()
    o = torch.zeros(V, n * J, 3, dtype=F64)
    o[..., 2] = torch.log(conf).permute(1, 0, 2).reshape(V, n * J)
    X, ref2d, proj2d, ex = T.triangulate(r, o, rec, torch.ones(1, n, dtype=torch.uint8), 1, V, 1, n, J)
    Xo, Ao, ud_o, Pm_o, conf_o = _oracle_chain(r, o, rec, V, 1, n * J)
    e = (rel(X, Xo), rel(ex["A"], Ao), rel(ref2d, proj2d))
    print("mini5_all: statement against the oracle's chain: X %.2e rows %.2e" % e[:2])
    assert e[0] < 1e-9 and e[1] < 1e-12 and e[2] == 0.0
    # ... and against what the reference recorded: its fp32 undistorted points, and the fp64 solution of ITS rows
    und = torch.from_numpy(g["tri_undist"]).double().permute(1, 0, 2, 3).reshape(1, V, n * J, 2)
    assert float((ud_o - und).abs().max()) < 1e-2                               # px: fp32 evaluation + the affine round trip
    cam = {k: v[:1].expand(n, *v.shape[1:]) for k, v in O._stack_cam(case.meta, F64).items()}
    X64, _ = O.dlt_triangulate(O.projection_matrices(cam, F64), torch.from_numpy(g["tri_undist"]).double(), conf)
    want32 = torch.from_numpy(g["tri_points3d"]).double()
    nrm = X64.norm(dim=-1).clamp_min(1.0)
    rel_ref = float(((want32 - X64).norm(dim=-1) / nrm).max())
    rel_st = float(((X.view(n, J, 3) - X64).norm(dim=-1) / nrm).max())
    print("mini5_all: reference fp32 SVD against fp64 %.2e, statement against fp64 of the recorded points %.2e" % (rel_ref, rel_st))
    assert rel_st <= max(2.0 * rel_ref, 1e-4)


def test_statement_matches_the_oracle_and_the_dlt_reference_on_a_random_case():
    """B = 2, V = 3, strong distortion, per-element image sizes, all classes: X, the rows, and geom_cases.dlt_reference on those rows."""
    V, B, NQ, J = 3, 2, 5, 15
    case = C.tri_case(V, B, NQ, J)
    X, ref2d, proj2d, ex = T.triangulate(case["r"], case["o"], case["rec"], C.all_valid(B, NQ), 1, V, B, NQ, J)
    Xo, Ao, ud, Pm, conf = _oracle_chain(case["r"], case["o"], case["rec"], V, B, NQ * J)
    e = (rel(X, Xo), rel(ex["A"], Ao))
    print("random case: statement against the oracle's chain: X %.2e rows %.2e" % e)
    assert e[0] < 1e-9 and e[1] < 1e-12
    Xd = dlt_reference(Pm, ud, conf, torch.zeros(B, NQ * J, 3), torch.ones(B, NQ * J, dtype=torch.bool))[0]
    assert rel(X, Xd) < 1e-9
    # the layouts: ref2d is (B, V, Lq, 2) of a view-major r
    img = case["rec"].double().view(V, B, 48)[:, :, 36:38]
    want = case["r"].double().view(V, B, NQ * J, 2) * img[:, :, None]
    assert torch.equal(proj2d, want.transpose(0, 1))
    assert float((ref2d - proj2d - case["o"].double().view(V, B, NQ * J, 3)[..., :2].transpose(0, 1)).abs().max()) < 1e-9


def test_masking_and_the_any_valid_rule():
    """a hand-written 2 x 3 validity table."""
    V, B, NQ, J = 3, 2, 3, 2
    case = C.tri_case(V, B, NQ, J, classes=[["noise2"] * NQ] * B)
    full = T.triangulate(case["r"], case["o"], case["rec"], C.all_valid(B, NQ), 1, V, B, NQ, J)
    for table, anyv, want in (([[0, 1, 0], [1, 0, 0]], 1, [[0, 1, 0], [1, 0, 0]]),
                              ([[0, 1, 0], [1, 0, 0]], 0, [[1, 1, 0], [1, 0, 0]]),
                              ([[0, 0, 0], [0, 0, 0]], 0, [[1, 0, 0], [0, 0, 0]]),
                              ([[0, 0, 0], [0, 0, 0]], 1, [[0, 0, 0], [0, 0, 0]]),
                              ([[1, 0, 0], [0, 0, 1]], 0, [[1, 0, 0], [0, 0, 1]])):
        X, ref2d, proj2d, ex = T.triangulate(case["r"], case["o"], case["rec"], torch.tensor(table, dtype=torch.uint8), anyv, V, B, NQ, J)
        tok = torch.tensor(want, dtype=torch.bool).repeat_interleave(J, 1)
        assert torch.equal(ex["computed"], tok)
        for got, ref, m in ((X, full[0], tok), (ref2d, full[1], tok[:, None].expand(B, V, NQ * J)), (proj2d, full[2], tok[:, None].expand(B, V, NQ * J))):
            assert torch.equal(got[m], ref[m]) and bool((got[~m] == 0).all()) and bool((ref[m] != 0).all())


def test_non_finite_inputs_stay_in_their_problem():
    V, B, NQ, J = 3, 1, 4, 1
    case = C.tri_case(V, B, NQ, J, classes=[["noise2"] * NQ])
    r, o = case["r"].clone(), case["o"].clone()
    o[1, 0, 0], o[2, 1, 2], r[0, 2, 1] = float("nan"), float("nan"), float("inf")        # dx of view 1, a logit, r.y of view 0
    X, ref2d, proj2d, ex = T.triangulate(r, o, case["rec"], C.all_valid(B, NQ), 1, V, B, NQ, J)
    X0 = T.triangulate(case["r"], case["o"], case["rec"], C.all_valid(B, NQ), 1, V, B, NQ, J)[0]
    assert bool(torch.isnan(X[0, :3]).all()) and torch.equal(X[0, 3], X0[0, 3])
    assert torch.equal(~torch.isfinite(ref2d).all(-1)[0], torch.tensor([[0, 0, 1, 0], [1, 0, 0, 0], [0, 0, 0, 0]], dtype=torch.bool))
    assert torch.equal(~torch.isfinite(proj2d).all(-1)[0], torch.tensor([[0, 0, 1, 0], [0, 0, 0, 0], [0, 0, 0, 0]], dtype=torch.bool))


# ------------------------------------------------------------------------ what the inputs of the GPU tests must satisfy
@pytest.fixture(scope="module")
def census():
    """per class (logit_edges by kind): path counts of invit_path, last pivots, yardsticks, over every case of the comparison."""
    paths, pivots, yard, fig = collections.defaultdict(collections.Counter), collections.defaultdict(list), {}, {}
    launches = [(c, None) for c in C.main_cases() + [(1,) + C.RAGGED]] + [((V,) + C.RAGGED, C.meet_only(*C.RAGGED[:2])) for V in C.MEET_ONLY_V]
    for (V, B, NQ, J), classes in launches:
        case = C.tri_case(V, B, NQ, J, classes=classes)
        assert bool(case["inside"].all()), (V, B, NQ, J)                     # no projection is clamped: the rays of `meet` meet
        val = C.all_valid(B, NQ)
        x64, _, _, e64 = T.triangulate(case["r"], case["o"], case["rec"], val, 1, V, B, NQ, J)
        x32, _, _, e32 = T.triangulate(case["r"], case["o"], case["rec"], val, 1, V, B, NQ, J, dtype=F32)
        path, raw = T.invit_path(T.gram32(e32), details=True)
        G33 = T.gram32(e32)[:, 3, 3].numpy()
        g32 = T.gap_figure(x32, e64)
        for name, m in C.groups(case, e64["computed"]).items():
            idx = m.view(-1).nonzero()[:, 0].tolist()
            paths[name].update(path[i] for i in idx)
            pivots[name] += [raw[i] / G33[i] for i in idx]
            key = (name, V)
            yard[key] = max(yard.get(key, 0.0), float((x32 - x64)[m].abs().max()))
            fig[key] = max(fig.get(key, 0.0), float(g32[m].max()))
            if name != "degenerate":
                assert bool(torch.isfinite(x32[m]).all()) and bool(torch.isfinite(x64[m]).all()) and bool(torch.isfinite(g32[m]).all())
    return paths, pivots, yard, fig


def test_cases_reach_every_path_of_the_inverse_iteration(census):
    paths, pivots, _, _ = census
    share = lambda name, cls: paths[name][cls] / max(sum(paths[name].values()), 1)
    for name in sorted(paths):
        print("%-24s %s" % (name, dict(paths[name])))
    assert share("meet", "first") >= 0.9
    assert share("off300", "shifted") >= 0.25
    assert share("degenerate", "declined") == 1.0 and sum(paths["degenerate"].values()) > 0
    # noise2 settles, but after its shift (see the module docstring): no problem of a class with a bar falls to the Jacobi
    for name in paths:
        if name != "degenerate":
            assert paths[name]["declined"] == 0, name
    assert share("noise2", "shifted") >= 0.5 and share("off30", "shifted") >= 0.9
    # last pivots of the first factorisation before the clamp, relative to G33: `meet` holds both signs
    pm = np.array(pivots["meet"])
    print("meet: last pivot / G33 %.1e ... %.1e, %d of %d negative" % (pm.min(), pm.max(), int((pm < 0).sum()), pm.size))
    assert int((pm < 0).sum()) >= 3 and bool((pm > 0).any()) and bool(np.isfinite(pm).all())


def test_yardsticks_are_finite_and_of_the_expected_size(census):
    _, _, yard, fig = census
    for (name, V) in sorted(yard):
        print("%-24s V=%2d  fp32 statement against fp64: %.2e mm, gap figure %.2e" % (name, V, yard[(name, V)], fig[(name, V)]))
        if name == "degenerate":
            continue
        assert np.isfinite(yard[(name, V)]) and 0 < fig[(name, V)] < 1e-4
        if not name.startswith("off"):
            assert 0 < yard[(name, V)] < 1e-2                                  # mm


def test_logit_edges_reach_the_edges_of_the_fp32_softmax():
    V, B, NQ, J = 9, 1, 5, 4
    case = C.tri_case(V, B, NQ, J, classes=[["logit_edges"] * NQ])
    conf = T.triangulate(case["r"], case["o"], case["rec"], C.all_valid(B, NQ), 1, V, B, NQ, J, dtype=F32)[3]["conf"]
    assert conf.dtype == F32 and bool(torch.isfinite(conf).all())
    tiny = float(torch.finfo(F32).tiny)
    for j, k in enumerate(C.EDGE_KINDS):
        assert case["kind"][0][j] == k
        w = conf[0, :, j]
        if k.startswith("all"):
            assert bool((w == w[0]).all()) and abs(float(w[0]) - 1.0 / V) < 1e-7
        elif k == "ramp-100":
            assert 0.0 < float(w[-1]) < tiny and float(w[1]) > 0.1            # a subnormal weight; the leading views share the weight
        else:
            assert float(w[-1]) == 0.0 and float(w[1]) > 0.1                   # an exact zero


def test_gap_figure_is_first_order_and_scale_free():
    """moving the fp64 solution by t along the second singular vector gives a figure of t (to first order), whatever the distance."""
    V, B, NQ, J = 3, 1, 10, 1
    case = C.tri_case(V, B, NQ, J, classes=[["noise2", "off300"] * 5])
    X, _, _, ex = T.triangulate(case["r"], case["o"], case["rec"], C.all_valid(B, NQ), 1, V, B, NQ, J)
    assert float(T.gap_figure(X, ex).max()) < 1e-9
    for t in (1e-6, 1e-4):
        h = ex["Vh"][..., 3, :] + t * ex["Vh"][..., 2, :]
        f = T.gap_figure(h[..., :3] / h[..., 3:4], ex)
        assert float((f / t - 1).abs().max()) < 1e-3, (t, f)
