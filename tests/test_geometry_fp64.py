"""The camera-geometry kernels of csrc/geom.hip (mvg_project, mvg_uncrop_undistort_jac, mvg_dlt_forward / mvg_dlt_backward,
mvg_sym4_eigh, mvg_pack_pyramid, mvg_gather_ref) against the fp64 statements of tests/geom_ref.py (pinned to the oracle by
tests/test_geom_ref_oracle.py), at the shapes and cameras where their code can go wrong unseen.

Error bars (no absolute figure): the yardstick of an fp32 output is the error of geom_ref evaluated in fp32 on the CPU against
its own fp64 evaluation -- it measures the reference, never the kernel -- and the kernel's bar is 4 x the yardstick's maximum over
the case + 2 ulp of the output.  For what the kernels compute in fp64 (the DLT) the yardstick is the fp64 SVD reference
re-evaluated from inputs perturbed by half an fp32 ulp: the conditioning of the problem.  Every assertion prints max err / bar.
Every output buffer carries a guard region filled with a sentinel, which must come back untouched.

The builders of the inputs (camera_records, project_cloud, uncrop_points, dlt_inputs, degenerate_token, boundary_token) live in
tests/geom_cases.py: tests/test_geom_ref_oracle.py checks their properties (share of border pairs, visibility of the distortion terms, the
coincident eigenvalues) without a device."""
import ctypes as C

import pytest
import torch

from tests import geom_ref as R
from tests.geom_cases import (BF16, EPS32, F32, F64, PROJ_SHAPES, PYR_S, PYR_SHAPES, PYR_STARTS, SENT_F, bar32, bf_next, border_distance,
                              boundary_token, camera_records, degenerate_token, dlt_bars, dlt_inputs, dlt_reference, eig_families,
                              eig_figures, inside_margin, project_cloud, uncrop_points, z_cam, _gather_points, _pyramid_src, _valid)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 1024
SENT_U8 = 0xA5
BADARG = 10001                  # MVG_E_BADARG


# ------------------------------------------------------------------------------------------------------------- GPU helpers
def _lib():
    from mvgformer_amd import _lib as L
    return L


def _guarded(n, dtype, front=0):
    """(buffer, view of n elements at offset `front`): the rest of the buffer is the guard, filled with the sentinel."""
    buf = torch.full((front + n + GUARD,), SENT_U8 if dtype == torch.uint8 else SENT_F, dtype=dtype, device=DEV)
    return buf, buf[front:front + n]


def _guard_ok(buf, n, front=0):
    s = torch.full((1,), SENT_U8 if buf.dtype == torch.uint8 else SENT_F, dtype=buf.dtype, device=buf.device)
    return bool((buf[:front] == s).all()) and bool((buf[front + n:] == s).all())


def _check(name, got, ref, bar):
    err = (got.double().cpu() - ref).abs()
    bar = bar if isinstance(bar, torch.Tensor) else torch.full_like(err, bar)
    ratio = float((err / bar.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print("%s: max err %.3e, max err / bar %.3f" % (name, float(err.max()) if err.numel() else 0.0, ratio))
    assert bool((err <= bar).all()), (name, ratio)
    return ratio


def _i64(rows):
    flat = [int(x) for r in rows for x in (r if isinstance(r, (tuple, list)) else (r,))]
    return (C.c_int64 * len(flat))(*flat)


# ------------------------------------------------------------------------------------------------------------- mvg_project


@pytest.fixture(scope="module")
def proj_case():
    rec = camera_records(3, 2)
    X = project_cloud(rec)
    return rec, X, {L: (R.project(X, rec, sh), R.project(X, rec, sh, dtype=F32)) for L, sh in PROJ_SHAPES.items()}


@pytest.mark.parametrize("L", [1, 4])
def test_project_against_fp64(proj_case, L):
    """V = 3, B = 2, Lq = 257 (1542 pairs: a ragged last 256-thread workgroup), non-square levels; points in the scene, across each
    border of view 0, behind every camera and far off axis (both clamps).  r and ref_lvl within the bar; `inside` equal for every
    pair whose fp64 pixel is farther from every border than the reference's own fp32 error (at most 1 % of the pairs are not)."""
    Lm = _lib()
    rec, X, refs = proj_case
    (r64, lv64, in64, u64), (r32, lv32, in32, u32) = refs[L]
    V, B, Lq = 3, 2, X.shape[1]
    n = V * B * Lq
    rb, r = _guarded(n * 2, F32)
    lb, lv = _guarded(n * L * 2, F32)
    ib, ins = _guarded(n, torch.uint8)
    Xd, recd = X.to(DEV), rec.to(DEV)                    # held until the launch has finished
    Lm.check(Lm.load().mvg_project(Lm.ptr(Xd), Lm.ptr(recd), _i64(PROJ_SHAPES[L]), L, Lm.ptr(r), Lm.ptr(lv), Lm.ptr(ins),
                                   V, B, Lq, Lm.stream_ptr()), "mvg_project")
    torch.cuda.synchronize()
    assert _guard_ok(rb, n * 2) and _guard_ok(lb, n * L * 2) and _guard_ok(ib, n)
    keep = (z_cam(X, rec) + 1e-5).abs() >= 1.0                                  # the reference itself divides by ~0 below 1 mm
    assert bool(keep.all())
    _check("project L=%d r" % L, r.view(V * B, Lq, 2), r64, bar32(r64, r32))
    _check("project L=%d ref_lvl" % L, lv.view(V * B, Lq, L, 2), lv64, bar32(lv64, lv32))
    wh = rec[:, None, 33:35].double()
    sure = border_distance(u64, wh) > inside_margin(u64, u32, wh).amax(-1)
    share = 1.0 - float(sure.double().mean())
    print("project L=%d inside: %d pairs compared, %.3f %% left out, %d inside" % (L, int(sure.sum()), 100 * share, int(in64.sum())))
    assert share <= 0.01
    assert torch.equal(ins.view(V * B, Lq).cpu()[sure].bool(), in64[sure])
    # the clamps are reached from both sides, and the bound is the batch's, not the image's own size
    uc = r64 * rec[:, None, 36:38].double()
    assert float(uc.min()) < 0 and bool((u64[1::2] > rec[1::2, None, 33:35].double().amax(-1, keepdim=True)).any())


# ---------------------------------------------------------------------------------------------- mvg_uncrop_undistort_jac
def _uncrop(ref2d, rec, V, B):
    Lm = _lib()
    Lq = ref2d.shape[2]
    n = B * V * Lq
    ub, ud = _guarded(n * 2, F32)
    jb, jac = _guarded(n * 4, F32)
    pd, recd = ref2d.to(DEV).contiguous(), rec.to(DEV)     # held until the launch has finished
    rc = Lm.load().mvg_uncrop_undistort_jac(Lm.ptr(pd), Lm.ptr(recd), Lm.ptr(ud), Lm.ptr(jac), V, B, Lq,
                                            Lm.stream_ptr())
    torch.cuda.synchronize()
    assert _guard_ok(ub, n * 2) and _guard_ok(jb, n * 4)
    return rc, ud.view(B, V, Lq, 2).clone(), jac.view(B, V, Lq, 2, 2).clone(), (ub, jb)


@pytest.mark.parametrize("rotated", [False, True])
def test_uncrop_undistort_and_jacobian_against_fp64(rotated):
    """B = 2, V = 3, Lq = 129 (774 points, a ragged workgroup), strong k1 / k2 / k3 / p1 / p2, fx != fy, no distortion on one camera,
    with and without a rotated inverse affine: ud against geom_ref, jac against the fp64 autograd Jacobian."""
    V, B = 3, 2
    rec, ref2d = camera_records(V, B, rotated), uncrop_points()
    ud64, jac64 = R.uncrop_undistort_jac(ref2d, rec)
    ud32, jac32 = R.uncrop_undistort_jac(ref2d, rec, dtype=F32)
    rc, ud, jac, _ = _uncrop(ref2d, rec, V, B)
    assert rc == 0
    _check("uncrop rotated=%d ud" % rotated, ud, ud64, bar32(ud64, ud32))
    bj = bar32(jac64, jac32)
    _check("uncrop rotated=%d jac" % rotated, jac, jac64, bj)
    # the camera without distortion (image 4 = view 2, batch element 0): the affine image and the affine's 2 x 2 part
    c = rec[4].double()
    A = c[27:33].view(2, 3)
    _check("uncrop k=p=0 ud", ud[0, 2], ref2d[0, 2].double() @ A[:, :2].t() + A[:, 2], bar32(ud64, ud32)[0, 2])
    _check("uncrop k=p=0 jac", jac[0, 2], A[:, :2].expand(ref2d.shape[2], 2, 2), bj[0, 2])


def test_uncrop_camera_index_follows_the_view_major_records():
    """records of images 0 (view 0, b 0) and 3 (view 1, b 1) swapped, the same points in both slots: the two slots' outputs swap,
    every other slot keeps its bits (image n = v * B + b against the (B, V, Lq) layout of the points)."""
    V, B = 3, 2
    rec, ref2d = camera_records(V, B, True), uncrop_points()
    ref2d[1, 1] = ref2d[0, 0]
    sw = rec.clone()
    sw[0], sw[3] = rec[3], rec[0]
    _, ud, jac, _ = _uncrop(ref2d, rec, V, B)
    _, ud2, jac2, _ = _uncrop(ref2d, sw, V, B)
    assert not torch.equal(ud[0, 0], ud[1, 1])
    for a, b in ((ud, ud2), (jac, jac2)):
        assert torch.equal(b[0, 0], a[1, 1]) and torch.equal(b[1, 1], a[0, 0])
        assert torch.equal(b[0, 1:], a[0, 1:]) and torch.equal(b[1, 0], a[1, 0]) and torch.equal(b[1, 2], a[1, 2])


def test_uncrop_function_backward_is_the_transposed_jacobian():
    """geometry_torch.UncropUndistort: backward(g) = J^T g of the fp64 autograd, with rotated inverse affines and fx != fy (J is
    far from symmetric: J g instead of J^T g fails)."""
    from mvgformer_amd import geometry_torch as G
    V, B = 3, 2
    rec, ref2d = camera_records(V, B, True), uncrop_points()
    g = torch.randn(ref2d.shape, generator=torch.Generator().manual_seed(12), dtype=F64).float()
    grads = {}
    for dt in (F64, F32):
        x = ref2d.detach().to(dt).clone().requires_grad_(True)
        R.uncrop_undistort(x, rec, dt).backward(g.to(dt))
        grads[dt] = x.grad
    _, jac64 = R.uncrop_undistort_jac(ref2d, rec)
    wrong = (jac64 @ g.double()[..., None])[..., 0]
    x = ref2d.detach().clone().to(DEV).requires_grad_(True)
    G.UncropUndistort.apply(x, rec.to(DEV), V, B).backward(g.to(DEV))
    bar = bar32(grads[F64], grads[F32])
    _check("UncropUndistort backward", x.grad, grads[F64], bar)
    assert float(((wrong - grads[F64]).abs() / bar).max()) > 10.0


def test_uncrop_of_no_points_writes_nothing():
    """Lq = 0 with valid pointers: returns 0 and no element of either output buffer changes."""
    Lm = _lib()
    pd, recd = torch.zeros(2, 3, 1, 2, device=DEV), camera_records(3, 2).to(DEV)
    ub, ud = _guarded(12, F32)
    jb, jac = _guarded(24, F32)
    rc = Lm.load().mvg_uncrop_undistort_jac(Lm.ptr(pd), Lm.ptr(recd), Lm.ptr(ud), Lm.ptr(jac), 3, 2, 0, Lm.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and bool((ub == SENT_F).all()) and bool((jb == SENT_F).all())


# ------------------------------------------------------------------------------------------ mvg_dlt_forward / _backward
def _dlt_launch(Pm, ud, conf, valid, gX, V, J):
    """raw launches of both kernels on guarded buffers -> (rc_fwd, rc_bwd, X, g_ud, g_conf) on the CPU."""
    Lm = _lib()
    B, NQ = valid.shape
    Lq = NQ * J
    xb, X = _guarded(B * Lq * 3, F32)
    ub, g_ud = _guarded(B * V * Lq * 2, F32)
    cb, g_conf = _guarded(B * V * Lq, F32)
    d = [t.to(DEV).contiguous() for t in (ud, conf, Pm, valid, gX)]
    lib = Lm.load()
    rf = lib.mvg_dlt_forward(Lm.ptr(d[0]), Lm.ptr(d[1]), Lm.ptr(d[2]), Lm.ptr(d[3]), Lm.ptr(X), V, B, NQ, J, Lm.stream_ptr())
    rb = lib.mvg_dlt_backward(Lm.ptr(d[0]), Lm.ptr(d[1]), Lm.ptr(d[2]), Lm.ptr(d[3]), Lm.ptr(d[4]), Lm.ptr(g_ud), Lm.ptr(g_conf), V, B,
                              NQ, J, Lm.stream_ptr())
    torch.cuda.synchronize()
    assert _guard_ok(xb, B * Lq * 3) and _guard_ok(ub, B * V * Lq * 2) and _guard_ok(cb, B * V * Lq)
    if rf or rb:
        assert bool((xb == SENT_F).all()) and bool((ub == SENT_F).all()) and bool((cb == SENT_F).all())
    return rf, rb, X.view(B, Lq, 3).cpu(), g_ud.view(B, V, Lq, 2).cpu(), g_conf.view(B, V, Lq).cpu()


@pytest.mark.parametrize("valid_kind", ["mixed", "none", "last"])
@pytest.mark.parametrize("V,J", [(2, 15), (8, 15), (32, 15), (8, 1)])
def test_dlt_against_fp64_svd(V, J, valid_kind):
    """B = 2, NQ = 9, J = 15 (270 tokens: a ragged 64-lane workgroup) and J = 1: X, g_ud, g_conf against the fp64 SVD and its autograd
    on the same fp32 inputs; zeros for the tokens of the other queries."""
    B, NQ = 2, 9
    Pm, ud, conf, gX = dlt_inputs(V, B, NQ, J)
    valid = _valid(valid_kind, B, NQ, torch.Generator().manual_seed(V + J))
    tok = valid.bool().view(B, NQ, 1).expand(B, NQ, J).reshape(B, NQ * J)
    rf, rb, X, g_ud, g_conf = _dlt_launch(Pm, ud, conf, valid, gX, V, J)
    assert rf == 0 and rb == 0
    assert bool((X[~tok] == 0).all()) and bool((g_ud.transpose(1, 2)[~tok] == 0).all()) and bool((g_conf.transpose(1, 2)[~tok] == 0).all())
    ref = dlt_reference(Pm, ud, conf, gX, tok)
    bars = dlt_bars(Pm, ud, conf, gX, tok, ref)
    for nm, got, want, bar in zip(("X", "g_ud", "g_conf"), (X, g_ud, g_conf), ref, bars):
        _check("dlt V=%d J=%d %s %s" % (V, J, valid_kind, nm), got, want, bar)


def test_dlt_rejects_more_than_32_views():
    B, NQ, J, V = 1, 1, 1, 33
    z = torch.zeros
    rf, rb, _, _, _ = _dlt_launch(z(B, V, 3, 4), z(B, V, 1, 2), z(B, V, 1), torch.ones(B, NQ, dtype=torch.uint8), z(B, 1, 3), V, J)
    assert rf == BADARG and rb == BADARG


def test_dlt_single_view_is_rank_deficient_but_contained():
    """V = 1: two rows for four unknowns.  Nothing is promised about the values (finite or NaN); the launch succeeds and stays inside
    its buffers.  (What it returns is recorded in DESIGN.md section 9e.)"""
    Pm, ud, conf, gX = dlt_inputs(1, 2, 9, 15)
    valid = torch.ones(2, 9, dtype=torch.uint8)
    rf, rb, X, g_ud, g_conf = _dlt_launch(Pm, ud, conf, valid, gX, 1, 15)
    assert rf == 0 and rb == 0
    for nm, t in (("X", X), ("g_ud", g_ud), ("g_conf", g_conf)):
        assert not bool(torch.isinf(t).any()), nm
        print("dlt V=1 %s: %d finite of %d, largest finite %.3e" % (nm, int(torch.isfinite(t).sum()), t.numel(),
                                                                   float(t[torch.isfinite(t)].abs().max()) if torch.isfinite(t).any() else 0.0))


def test_dlt_views_of_zero_confidence():
    """two views with conf = 0 exactly: their g_ud is exactly 0, their g_conf what the reference gives (the Gram matrix depends on
    conf^2, so the SVD's autograd gives 0 to rounding there as well)."""
    B, NQ, J, V = 2, 9, 15, 8
    Pm, ud, conf, gX = dlt_inputs(V, B, NQ, J)
    conf[:, 2] = 0.0
    conf[:, 7] = 0.0
    valid = torch.ones(B, NQ, dtype=torch.uint8)
    tok = torch.ones(B, NQ * J, dtype=torch.bool)
    rf, rb, X, g_ud, g_conf = _dlt_launch(Pm, ud, conf, valid, gX, V, J)
    assert rf == 0 and rb == 0 and bool((g_ud[:, [2, 7]] == 0).all())
    ref = dlt_reference(Pm, ud, conf, gX, tok)
    bars = dlt_bars(Pm, ud, conf, gX, tok, ref)
    for nm, got, want, bar in zip(("X", "g_ud", "g_conf"), (X, g_ud, g_conf), ref, bars):
        _check("dlt zero-confidence views %s" % nm, got, want, bar)


@pytest.mark.parametrize("k", [-4, -70, 55])
def test_dlt_is_invariant_to_a_common_scale_of_the_confidences(k):
    """conf * 2^k: X and g_ud do not change and g_conf scales by 2^-k.  k = -4: the Gram matrix scales by an exact power of two, so all
    three hold bit for bit.  k = -70 / +55: the Gram matrix (~1e14 * 2^2k) is outside fp32's exponent range and far inside fp64's;
    the results stay within the bars of the unscaled fp64 reference."""
    B, NQ, J, V = 2, 9, 15, 8
    Pm, ud, conf, gX = dlt_inputs(V, B, NQ, J)
    valid = torch.ones(B, NQ, dtype=torch.uint8)
    tok = torch.ones(B, NQ * J, dtype=torch.bool)
    _, _, X0, u0, c0 = _dlt_launch(Pm, ud, conf, valid, gX, V, J)
    rf, rb, X, g_ud, g_conf = _dlt_launch(Pm, ud, conf * 2.0 ** k, valid, gX, V, J)
    assert rf == 0 and rb == 0
    if k == -4:
        assert torch.equal(X, X0) and torch.equal(g_ud, u0) and torch.equal(g_conf, c0 * 2.0 ** -k)
        return
    ref = dlt_reference(Pm, ud, conf, gX, tok)
    bars = dlt_bars(Pm, ud, conf, gX, tok, ref)
    for nm, got, want, bar in zip(("X", "g_ud", "g_conf"), (X, g_ud, g_conf.double() * 2.0 ** k), ref, bars):
        _check("dlt conf * 2^%d %s" % (k, nm), got, want, bar)


def test_dlt_backward_drops_a_coincident_pair():
    """the two smallest eigenvalues coincide (degenerate_token): 1 / (l0 - l1) is dropped by the 1e-14 * max |l| guard and the
    gradients are finite; at a gap EQUAL to the threshold (boundary_token) the pair is still dropped: exactly zero gradients
    for the rows along that eigenvector, where keeping it would give ~1e7 and more."""
    valid = torch.ones(1, 1, dtype=torch.uint8)
    gX = torch.tensor([[[0.3, -0.7, 0.5]]])
    Pm, ud, conf = degenerate_token()
    rf, rb, X, g_ud, g_conf = _dlt_launch(Pm, ud, conf, valid, gX, 2, 1)
    print("degenerate token: X", X.flatten().tolist(), "g_ud", g_ud.flatten().tolist(), "g_conf", g_conf.flatten().tolist())
    assert rf == 0 and rb == 0
    assert bool(torch.isfinite(X).all()) and bool(torch.isfinite(g_ud).all()) and bool(torch.isfinite(g_conf).all())
    assert float(g_ud.abs().max()) < 1e3 and float(g_conf.abs().max()) < 1e3
    Pm, ud, conf, _ = boundary_token()
    rf, rb, X, g_ud, g_conf = _dlt_launch(Pm, ud, conf, valid, gX, 2, 1)
    print("boundary token: X", X.flatten().tolist(), "g_ud", g_ud.flatten().tolist(), "g_conf", g_conf.flatten().tolist())
    assert rf == 0 and rb == 0 and bool((X == 0).all())
    # the x rows of both views are the two rows along the dropped eigenvector: their gradient is exactly 0 (7e6 and more if kept)
    assert bool((g_ud[..., 0] == 0).all()) and float(g_ud.abs().max()) < 1e3 and float(g_conf.abs().max()) < 1e3


# ----------------------------------------------------------------------------------------------------------- mvg_sym4_eigh
def _eigh(G):
    Lm = _lib()
    n = G.shape[0]
    wb, w = _guarded(n * 4, F64)
    vb, V = _guarded(n * 16, F64)
    Gd = G.to(DEV).contiguous()
    Lm.check(Lm.load().mvg_sym4_eigh(Lm.ptr(Gd), Lm.ptr(w), Lm.ptr(V), n, Lm.stream_ptr()), "mvg_sym4_eigh")
    torch.cuda.synchronize()
    assert _guard_ok(wb, n * 4) and _guard_ok(vb, n * 16)
    return w.view(n, 4).cpu(), V.view(n, 4, 4).cpu()


@pytest.fixture(scope="module")
def eig_case():
    G = eig_families()
    w, V = torch.linalg.eigh(0.5 * (G + G.transpose(1, 2)))
    c = 4.0 * max(eig_figures(G, w, V)) / 1e-15
    return G, c


@pytest.mark.parametrize("n", [1, 255, 257])
def test_sym4_eigh_against_fp64(eig_case, n):
    """seven families of matrices at scales 2^k, k = -200 ... 200: residual, orthogonality and eigenvalues relative to the matrix's
    own norm, within c * 1e-15 (c: 4 x what torch.linalg.eigh on the CPU reaches on the same matrices at scale 1); k = +-20 give
    the eigenvectors of k = 0 bit for bit and exactly scaled eigenvalues."""
    G, c = eig_case
    G = G[:n]
    print("sym4_eigh: c = %.2f" % c)
    base = None
    for k in (0, -200, -140, -20, 20, 140, 200):
        w, V = _eigh(G * 2.0 ** k)
        assert bool(torch.isfinite(w).all()) and bool(torch.isfinite(V).all())
        if k == 0:
            base = (w, V)
        if abs(k) == 20:
            assert torch.equal(V, base[1]) and torch.equal(w, base[0] * 2.0 ** k)
        fig = eig_figures(G, w * 2.0 ** -k, V)
        print("sym4_eigh n=%d k=%4d: residual %.2e orthogonality %.2e eigenvalues %.2e, max / (c 1e-15) %.3f"
              % (n, k, fig[0], fig[1], fig[2], max(fig) / (c * 1e-15)))
        assert max(fig) <= c * 1e-15, (k, fig)


# ----------------------------------------------------------------------------------- mvg_pack_pyramid / mvg_gather_ref

def _pack(src, C_, dtype):
    Lm = _lib()
    N = src[0].shape[0]
    fb, feat = _guarded(N * PYR_S * C_, dtype)
    d = [s.to(DEV).contiguous() for s in src]
    ptrs = (C.c_void_p * len(d))(*[s.data_ptr() for s in d])
    rc = Lm.load().mvg_pack_pyramid(ptrs, Lm.ptr(feat), Lm.dtype_code(dtype), N, C_, _i64(PYR_SHAPES), _i64(PYR_STARTS), len(d), PYR_S,
                                    Lm.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and _guard_ok(fb, N * PYR_S * C_)
    return feat.view(N, PYR_S, C_).clone()


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C_", [4, 6, 64, 70, 256])
def test_pack_pyramid_is_exact(C_, dtype):
    """three images, levels (5, 13), (3, 7), (1, 2) (HW = 65: more than one 64-pixel tile), C with and without the vector stores and
    whole 64-channel tiles: fp32 exact, bf16 = torch's rounding bit for bit; the sentinel survives in the gaps between the levels."""
    src = _pyramid_src(C_)
    feat = _pack(src, C_, dtype)
    want = R.pack_pyramid(src, PYR_SHAPES, PYR_STARTS, PYR_S, dtype=F32, fill=SENT_F).to(dtype)
    bits = torch.int32 if dtype == F32 else torch.int16
    assert torch.equal(feat.cpu().view(bits), want.view(bits))
    assert bool((feat[:, 65:70] == want[0, 65, 0].item()).all())


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C_", [4, 64, 256])
def test_gather_ref_against_fp64(C_, dtype):
    """V = 2, B = 2, Lq = 67, L = 3 on the packed pyramid above (gaps between the levels): against grid_sample in fp64 on the upcast
    features.  fp32: the bar of the reference's own fp32 evaluation; bf16: one of the bf16 neighbours of the exact sum, widened by
    that fp32 error."""
    Lm = _lib()
    V, B, Lq, L = 2, 2, 67, 3
    gen = torch.Generator().manual_seed(31 + C_)
    src = [torch.randn(V * B, C_, H, W, generator=gen) for H, W in PYR_SHAPES]
    feat = R.pack_pyramid(src, PYR_SHAPES, PYR_STARTS, PYR_S, dtype=F32, fill=7.0).to(dtype)     # a read into a gap between levels shows
    ref_lvl = _gather_points(V * B, Lq, gen)
    x = torch.randn(B, Lq, C_, generator=gen)
    n = V * B * Lq * L * C_
    ab, ain = _guarded(n, dtype)
    fd, rd, xd = feat.to(DEV), ref_lvl.to(DEV), x.to(DEV)   # held until the launch has finished
    rc = Lm.load().mvg_gather_ref(Lm.ptr(fd), Lm.dtype_code(dtype), Lm.ptr(rd), Lm.ptr(xd), _i64(PYR_SHAPES),
                                  _i64(PYR_STARTS), Lm.ptr(ain), V, B, Lq, L, PYR_S, C_, Lm.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and _guard_ok(ab, n)
    got = ain.view(V * B, Lq, L, C_).cpu()
    ex = R.gather_ref(feat, ref_lvl, x, PYR_SHAPES, PYR_STARTS)
    e32 = 4.0 * float((R.gather_ref(feat, ref_lvl, x, PYR_SHAPES, PYR_STARTS, dtype=F32).double() - ex).abs().max())
    if dtype == F32:
        _check("gather_ref f32 C=%d" % C_, got, ex, e32 + 2.0 * EPS32 * ex.abs())
        return
    lo, hi = ex - e32, ex + e32
    nlo, nhi = lo.to(BF16).double(), hi.to(BF16).double()
    nlo = torch.where(nlo <= lo, nlo, bf_next(nlo, up=False))
    nhi = torch.where(nhi >= hi, nhi, bf_next(nhi, up=True))
    g = got.double()
    err = torch.maximum(nlo - g, g - nhi)
    print("gather_ref bf16 C=%d: %d of %d outside the bf16 neighbours of the exact sum, %.1f %% the nearest" %
          (C_, int((err > 0).sum()), g.numel(), 100 * float((g == ex.to(BF16).double()).double().mean())))
    assert bool((err <= 0).all())


@pytest.mark.parametrize("C_", [6, 70])
def test_gather_ref_says_that_it_needs_whole_channel_quads(C_):
    """C % 4 != 0: MVG_E_BADARG and nothing written (the kernel loads and stores four channels at a time)."""
    Lm = _lib()
    V, B, Lq, L = 2, 2, 3, 3
    feat = torch.zeros(V * B, PYR_S, C_, device=DEV)
    ab, ain = _guarded(V * B * Lq * L * C_, F32)
    rc = Lm.load().mvg_gather_ref(Lm.ptr(feat), 0, Lm.ptr(torch.zeros(V * B, Lq, L, 2, device=DEV)), Lm.ptr(torch.zeros(B, Lq, C_, device=DEV)),
                                  _i64(PYR_SHAPES), _i64(PYR_STARTS), Lm.ptr(ain), V, B, Lq, L, PYR_S, C_, Lm.stream_ptr())
    torch.cuda.synchronize()
    assert rc == BADARG and bool((ab == SENT_F).all())
