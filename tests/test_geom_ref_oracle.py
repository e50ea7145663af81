"""Pin the fp64 geometry statements of tests/geom_ref.py to the oracle (oracle/decoder_ref.py), which tests/test_oracle_golden.py
pins to the reference's fixtures, and check on the CPU what the inputs of the GPU tests (tests/geom_cases.py, run by tests/test_geometry_fp64.py) must
satisfy for those tests to mean something.  CPU only: the GPU tests then rest on the oracle, not on another kernel."""
import pytest
import torch

from mvgformer_amd import ops
from mvgformer_amd import synthetic as S
from oracle import decoder_ref as O
from tests import geom_ref as R
from tests import geom_cases as T
from tests.golden.cases import LAYER_CASES

F64 = torch.float64


def _mini5_b2():
    spec = LAYER_CASES["mini5_b2"]
    case = S.build_case(spec["config"], B=spec.get("B", 1), seed=spec["seed"], NQ=spec.get("NQ"), layers=spec.get("layers"),
                        valid_fraction=spec.get("valid_fraction"), with_features=False)
    return case.meta, case.img_size, case.reference_points, case.shapes


def _cfg5_k3():
    c = S.CONFIGS["cfg5"]
    B, V = 2, 4
    cams = S.ring_cameras(V, c["orig_wh"], c["focal"], c["radius"], c["space_center"], (-0.1, 0.05, 0.02), c["p"], seed=2)
    meta = S.make_meta(cams, B, c["orig_wh"], c["img_wh"])
    X = S.init_reference_points(B, 8, c["space_size"], c["space_center"], jitter=25.0, seed=2)
    return meta, list(c["img_wh"]), X, S.pyramid_shapes(c["img_wh"])


@pytest.mark.parametrize("make", [_mini5_b2, _cfg5_k3], ids=["mini5_b2", "cfg5_k3"])
def test_geometry_statements_match_the_oracle(make):
    meta, img_size, X, shapes = make()
    V, B, Lq = len(meta), X.shape[0], X.shape[1]
    rec = ops.pack_cameras(meta, img_size, "cpu")
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    # projection
    r, ref_lvl, inside, u = R.project(X, rec, shapes)
    WH = torch.tensor(shapes).flip(-1).double()
    n_in = 0
    for v in range(V):
        ro, io = O.project_ref_points(X, meta[v]["camera"], meta[v]["center"], meta[v]["scale"], img_size, F64)
        e = rel(r[v * B:(v + 1) * B], ro)
        el = rel(ref_lvl[v * B:(v + 1) * B], ro.unsqueeze(2) * WH / (WH - 1))
        print("project view %d: r %.2e ref_lvl %.2e" % (v, e, el))
        assert e < 1e-12 and el < 1e-12 and torch.equal(inside[v * B:(v + 1) * B], io)
        n_in += int(io.sum())
    assert 0 < n_in < V * B * Lq
    # un-crop + undistortion, projection matrices, DLT
    gen = torch.Generator().manual_seed(1)
    kp = (torch.rand(B, V, Lq, 2, generator=gen, dtype=F64) * 1.2 - 0.1) * torch.tensor(img_size, dtype=F64)
    cam = O._stack_cam(meta, F64)
    Ainv = torch.stack([m["inv_affine_trans"][:, :2, :] for m in meta], 1).float().double()
    uo = torch.matmul(torch.cat([kp, torch.ones_like(kp[..., :1])], -1), Ainv.transpose(2, 3))
    ud_o = O.undistort_points(uo, cam, F64)
    ud = R.uncrop_undistort(kp, rec)
    Pm_o, Pm = O.projection_matrices(cam, F64), R.proj_matrices(rec, V, B)
    conf = torch.softmax(torch.randn(B, V, Lq, generator=gen, dtype=F64), 1)
    X_o, A_o = O.dlt_triangulate(Pm_o, ud_o, conf)
    e = (rel(ud, ud_o), rel(Pm, Pm_o), rel(R.dlt_rows(Pm_o, ud_o, conf), A_o), rel(R.dlt(Pm_o, ud_o, conf), X_o))
    print("undistort %.2e  projection matrices %.2e  DLT rows %.2e  DLT %.2e" % e)
    assert max(e) < 1e-12
    assert float((ud - uo).abs().max()) > 1.0                         # the distortion is there


def test_pyramid_statements_match_the_oracle():
    """pack_pyramid + gather_ref against the oracle's explicit bilinear gather on the NCHW maps."""
    gen = torch.Generator().manual_seed(2)
    shapes, starts, S_ = T.PYR_SHAPES, T.PYR_STARTS, T.PYR_S
    V, B, Lq, C_ = 2, 2, 67, 8
    src = [torch.randn(V * B, C_, H, W, generator=gen, dtype=F64) for H, W in shapes]
    feat = R.pack_pyramid(src, shapes, starts, S_, fill=7.0)
    ref_lvl = T._gather_points(V * B, Lq, gen).double()
    x = torch.randn(B, Lq, C_, generator=gen, dtype=F64)
    got = R.gather_ref(feat, ref_lvl, x, shapes, starts)
    for l in range(3):
        want = O.bilinear_zeros(src[l], torch.clamp(ref_lvl[:, :, l] * 2.0 - 1.0, -1.1, 1.1)) + x.repeat(V, 1, 1)
        assert float((got[:, :, l] - want).abs().max()) < 1e-13
    assert bool((feat[:, 65:70] == 7.0).all()) and bool((feat[:, 91:96] == 7.0).all()) and bool((feat[:, 98:] == 7.0).all())


# ------------------------------------------------------------------------ what the inputs of the GPU tests must satisfy
def test_projection_cloud_leaves_at_most_one_percent_of_the_pairs_at_a_border():
    rec = T.camera_records(3, 2)
    X = T.project_cloud(rec)
    assert tuple(X.shape) == (2, 257, 3)
    z = T.z_cam(X, rec)
    assert bool(((z + 1e-5).abs() >= 1.0).all()) and int((z < 0).sum()) >= 6 * 8
    for L, shapes in T.PROJ_SHAPES.items():
        r64, lv64, in64, u64 = R.project(X, rec, shapes)
        r32, lv32, in32, u32 = R.project(X, rec, shapes, dtype=torch.float32)
        assert all(bool(torch.isfinite(t).all()) for t in (r32, lv32, u32))
        wh = rec[:, None, 33:35].double()
        dist, margin = T.border_distance(u64, wh), T.inside_margin(u64, u32, wh).amax(-1)
        sure = dist > margin
        share = 1.0 - float(sure.double().mean())
        print("L=%d: %.3f %% of the pairs within the fp32 error of a border, largest margin among in-box pairs %.2e px, yardsticks "
              "r %.2e ref_lvl %.2e" % (L, 100 * share, float(margin[dist < 100].max()), float((r32 - r64).abs().max()),
                                       float((lv32 - lv64).abs().max())))
        assert share <= 0.01
        assert torch.equal(in32[sure], in64[sure])                     # the fp32 reference itself agrees away from the borders
        # every border of view 0 has pairs within 1 px on both sides, and both clamps are reached
        for b in range(2):
            u, (w, h) = u64[b], wh[b, 0].tolist()
            for d in (u[:, 0], u[:, 0] - w, u[:, 1], u[:, 1] - h):
                assert bool(((d > 0) & (d < 1)).any()) and bool(((d < 0) & (d > -1)).any())
            assert bool((u.amin(-1) < -1).any()) and bool((u.amax(-1) > float(rec[b, 35])).any())
        assert float(rec[1, 35]) > float(rec[1, 33:35].max())          # the clamp bound is not the image's own size


def test_distortion_terms_are_visible_in_the_jacobian():
    """with k3, or the tangential coefficients, zeroed the fp64 Jacobian of the strong-distortion cameras moves by more than 10 x the
    bar of the GPU test: a kernel that dropped either term could not pass."""
    for rotated in (False, True):
        rec, ref2d = T.camera_records(3, 2, rotated), T.uncrop_points()
        _, jac64 = R.uncrop_undistort_jac(ref2d, rec)
        _, jac32 = R.uncrop_undistort_jac(ref2d, rec, dtype=torch.float32)
        bar = T.bar32(jac64, jac32)
        for name, cols in (("k3", [18]), ("p1 p2", [19, 20])):
            z = rec.clone()
            z[:, cols] = 0.0
            vis = ((R.uncrop_undistort_jac(ref2d, z)[1] - jac64).abs() / bar)
            strong = max(float(vis[0, 0].max()), float(vis[1, 1].max()))          # images 0 and 3
            off = max(float(vis[0, 0][:, [0, 1], [1, 0]].max()), float(vis[1, 1][:, [0, 1], [1, 0]].max()))
            print("rotated %d, %s zeroed: jac moves by %.0f x the bar (off-diagonal entries %.0f x)" % (rotated, name, strong, off))
            assert strong > 10.0 and off > 10.0
        assert abs(float(rec[0, 13] / rec[0, 12]) - 1.08) < 1e-6
        if rotated:
            assert abs(float(rec[0, 28])) > 0.3 * abs(float(rec[0, 27])) and float(rec[0, 28]) == -float(rec[0, 30])


def test_degenerate_tokens_are_what_they_claim():
    Pm, ud, conf = T.degenerate_token()
    A = R.dlt_rows(Pm.double(), ud.double(), conf.double())[0, 0]
    w = torch.linalg.eigvalsh(A.t() @ A)
    print("degenerate token: eigenvalues", w.tolist())
    assert abs(float(w[1] - w[0])) <= 1e-15 * float(w[3]) and float(w[2] - w[1]) > 1.0
    Pm, ud, conf, t = T.boundary_token()
    A = R.dlt_rows(Pm.double(), ud.double(), conf.double())[0, 0]
    from fractions import Fraction
    assert int((A != 0).sum()) == 4 and bool(((A != 0).sum(1) == 1).all())   # one entry per row: the Gram matrix is diagonal
    diag = [0.0] * 4
    for row in A.tolist():                                              # the kernels' order: one fma per row and entry
        diag = [float(Fraction(x) * Fraction(x) + Fraction(d)) for x, d in zip(row, diag)]
    print("boundary token: diagonal", diag, "threshold", t)
    assert diag[0] == 1.0 and diag[1] == t and 0.2 < diag[2] < 0.3 and diag[3] == 0.0 and t == 1e-14 * 1.0


def test_eigen_families_and_their_yardstick():
    G = T.eig_families()
    w, V = torch.linalg.eigh(0.5 * (G + G.transpose(1, 2)))
    fig = T.eig_figures(G, w, V)
    print("torch.linalg.eigh at scale 1: residual %.2e orthogonality %.2e eigenvalues %.2e" % fig)
    assert 0 < max(fig) < 1e-13
    ws = torch.linalg.eigvalsh(0.5 * (G + G.transpose(1, 2)))
    assert int(((ws[:, 1] - ws[:, 0]).abs() < 1e-14).sum()) >= 40        # repeated eigenvalues are there
    assert int((ws[:, 3].abs() / ws[:, 0].abs().clamp_min(1e-300) > 1e11).sum()) >= 40
