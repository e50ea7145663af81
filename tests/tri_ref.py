"""Plain torch statement of triangulate_kernel (csrc/geom.hip: mvg_triangulate, mvg_triangulate_project), fp64 by default, `dtype=`
selectable, on the CPU; the figure its rays-that-do-not-meet classes are judged by (gap_figure); and a plain fp64 model of the control
flow of null_vector_invit (invit_path), which only shows that the cases of tests/tri_cases.py reach each of its paths.  Built from the
statements of tests/geom_ref.py (uncrop_undistort, proj_matrices, dlt_rows), pinned to oracle/decoder_ref.py by
tests/test_tri_ref_cpu.py; tests/test_tri_fp64.py compares the kernel with it.

Layouts (the kernel's): r (V * B, Lq, 2) and o (V * B, Lq, 3) view major (image n = v * B + b), Lq = NQ * J, o = (dx, dy, logit);
valid (B, NQ); new_ref (B, Lq, 3); ref2d, proj2d (B, V, Lq, 2).

The solve: the right singular vector of the smallest singular value of the fp64 row matrix, as the oracle takes it.  The row matrix
is NOT rescaled per column first: for rays that do not meet, a column scaling D changes the minimiser itself (min |A D y| over unit y
is another point than min |A x| over unit x), and the kernel, the oracle and the reference all solve the unscaled problem.  What a
scaling would buy -- eigenvalues of the Gram matrix that can be told apart although they span twelve decades -- gap_figure gets from
the singular vectors instead (see there)."""
import numpy as np
import torch

from tests import geom_ref as R

F64, F32 = torch.float64, torch.float32


def computed_mask(valid, any_valid, J):
    """(B, NQ * J) bool: a problem is computed if its query is valid, or if no query of the launch is (any_valid == 0) and it belongs
    to query (0, 0)."""
    m = valid.detach().cpu().bool().clone()
    if int(any_valid) == 0:
        m[0, 0] = True
    B, NQ = m.shape
    return m.view(B, NQ, 1).expand(B, NQ, J).reshape(B, NQ * J)


def triangulate(r, o, cam_records, valid, any_valid, V, B, NQ, J, dtype=F64):
    """-> (new_ref (B, Lq, 3), ref2d (B, V, Lq, 2), proj2d (B, V, Lq, 2), extras).  Everything up to and including the DLT rows in
    `dtype`, the solve in fp64 always.  Zeros in all three outputs for the problems that are not computed; NaN in new_ref for a
    computed problem whose rows are not finite.  extras: A (B, Lq, 2V, 4) fp64 rows, lam (B, Lq, 4) eigenvalues of A^T A in ascending
    order, Vh (B, Lq, 4, 4) right singular vectors as rows (row 3: the null direction), null (B, Lq, 4), conf (B, V, Lq) in `dtype`,
    computed (B, Lq) bool, finite (B, Lq) bool."""
    Lq = NQ * J
    c = R._rec(cam_records, dtype).view(V, B, R.STRIDE).transpose(0, 1)                     # (B, V, 48)
    rr = r.detach().cpu().reshape(V, B, Lq, 2).transpose(0, 1).to(dtype)
    oo = o.detach().cpu().reshape(V, B, Lq, 3).transpose(0, 1).to(dtype)
    img = c[:, :, None, 36:38]
    conf = torch.softmax(oo[..., 2], 1)                                                     # over views
    proj2d = rr * img
    ref2d = (rr + oo[..., :2] / img) * img
    ud = R.uncrop_undistort(ref2d, cam_records, dtype)
    Pm = R.proj_matrices(cam_records, V, B, dtype)
    A = R.dlt_rows(Pm, ud, conf).double()                                                   # (B, Lq, 2V, 4)
    tok = computed_mask(valid, any_valid, J)
    finite = torch.isfinite(A).all(-1).all(-1)
    solve = tok & finite
    _, S, Vh = torch.linalg.svd(torch.where(solve[..., None, None], A, torch.zeros_like(A)))
    lam = torch.zeros(B, Lq, 4, dtype=F64)
    lam[..., :S.shape[-1]] = S * S
    lam = lam.flip(-1)
    null = -Vh[..., 3, :]
    X = null[..., :3] / null[..., 3:4]
    X = torch.where(solve[..., None], X, torch.full_like(X, float("nan")))
    X = torch.where(tok[..., None], X, torch.zeros_like(X))
    m = tok[:, None, :, None]
    ref2d = torch.where(m, ref2d, torch.zeros_like(ref2d))
    proj2d = torch.where(m, proj2d, torch.zeros_like(proj2d))
    return X, ref2d, proj2d, dict(A=A, lam=lam, Vh=Vh, null=null, conf=conf, computed=tok, finite=finite)


def gap_figure(X, extras):
    """sqrt((rho - l0) / (l1 - l0)) per problem (B, Lq): rho the Rayleigh quotient of (X, 1) in the fp64 Gram matrix A^T A, l0 <= l1
    its two smallest eigenvalues.  First order in the error -- about the sine of the angle between (X, 1) and the null vector, measured
    in the least constrained direction -- and independent of how far away the point lies.  Evaluated from the singular vectors v_i of
    A: with c_i = v_i . (X, 1),  rho - l0 = sum_i c_i^2 (l_i - l0) / sum_i c_i^2  exactly, with no cancellation, where l0 itself
    (1e-12 of the largest eigenvalue and less) is far below what rho - l0 as a difference of two computed numbers can resolve."""
    x = torch.cat([X.double().cpu(), torch.ones(X.shape[:-1] + (1,), dtype=F64)], -1)
    c = (extras["Vh"] @ x[..., None])[..., 0]                                               # (B, Lq, 4): index 3 = null direction
    l = extras["lam"].flip(-1)                                                              # descending, as the rows of Vh
    l0, l1 = l[..., 3:4], l[..., 2:3]
    num = (c[..., :3] ** 2 * (l[..., :3] - l0)).sum(-1)
    return torch.sqrt(num / ((l1 - l0)[..., 0] * (c * c).sum(-1)))


def gram32(extras32):
    """(n, 4, 4) fp64 Gram matrices of the fp32 rows of a dtype=F32 statement: what the kernel hands to null_vector_invit, up to the
    order of the fp64 sums."""
    A = extras32["A"].reshape(-1, extras32["A"].shape[-2], 4)
    return A.transpose(1, 2) @ A


# ---------------------------------------------------------------------------------------- the control flow of null_vector_invit
def _ldl4(G, sigma, first):
    g10, g20, g30, g21, g31, g32 = G[:, 0, 1], G[:, 0, 2], G[:, 0, 3], G[:, 1, 2], G[:, 1, 3], G[:, 2, 3]
    d0 = G[:, 0, 0] - sigma
    i0 = 1.0 / d0
    l10, l20, l30 = g10 * i0, g20 * i0, g30 * i0
    d1 = G[:, 1, 1] - sigma - l10 * g10
    i1 = 1.0 / d1
    t21, t31 = g21 - l20 * g10, g31 - l30 * g10
    l21, l31 = t21 * i1, t31 * i1
    d2 = G[:, 2, 2] - sigma - l20 * g20 - l21 * t21
    i2 = 1.0 / d2
    t32 = g32 - l30 * g20 - l31 * t21
    l32 = t32 * i2
    d3 = G[:, 3, 3] - sigma - l30 * g30 - l31 * t31 - l32 * t32
    raw = d3
    if first:
        d3 = np.fmax(d3, 1e-18 * G[:, 3, 3])
        ok = (d0 > 0) & (d1 > 1e-13 * G[:, 1, 1]) & (d2 > 1e-13 * G[:, 2, 2])
    else:
        ok = (d0 > 0) & (d1 > 0) & (d2 > 0) & (d3 > 0)
    f = np.stack([i0, i1, i2, 1.0 / d3, l10, l20, l30, l21, l31, l32], 0)
    return ok, f, raw


def _solve(f, w):
    i0, i1, i2, i3, l10, l20, l30, l21, l31, l32 = f
    w0, w1, w2, w3 = w
    y1 = w1 - l10 * w0
    y2 = w2 - l20 * w0 - l21 * y1
    y3 = w3 - l30 * w0 - l31 * y1 - l32 * y2
    z0, z1, z2 = w0 * i0, y1 * i1, y2 * i2
    w3 = y3 * i3
    w2 = z2 - l32 * w3
    w1 = z1 - l21 * w2 - l31 * w3
    w0 = z0 - l10 * w1 - l20 * w2 - l30 * w3
    return np.stack([w0, w1, w2, w3], 0)


def invit_path(G, details=False):
    """fp64 model of the control flow of null_vector_invit for the (n, 4, 4) Gram matrices G: the first factorisation's pivot tests,
    rounds of 4 solves, the 1e-11 parallel test, the shift to rho - |G x - rho x| taken only when all four pivots stay positive, and
    MAXR = 12.  -> list of "first" (settled at sigma = 0), "shifted" (settled after at least one refactorisation) or "declined" (unsafe
    pivots, or not settled: the Jacobi fallback) per problem; with details, also the last pivot of the first factorisation before
    its clamp.  Shows which paths a set of cases reaches; no kernel output is ever compared with it."""
    G = np.asarray(torch.as_tensor(G).double().numpy()).reshape(-1, 4, 4)
    n = G.shape[0]
    with np.errstate(all="ignore"):
        pivots_ok, f, raw = _ldl4(G, 0.0, True)
        sigma = np.zeros(n)
        x = np.ones((4, n))
        done = np.zeros(n, dtype=bool)
        shifted = np.zeros(n, dtype=bool)
        for _ in range(12):
            w = x
            for _k in range(4):
                p = w
                w = _solve(f, w)
            mw, mp = np.abs(w).max(0), np.abs(p).max(0)
            cmax = np.zeros(n)
            for a in range(4):
                for b in range(a + 1, 4):
                    cmax = np.fmax(cmax, np.abs(w[a] * p[b] - w[b] * p[a]))
            parallel = cmax <= 1e-11 * mw * mp
            ex = np.frexp(np.where(np.isfinite(mw) & (mw > 0), mw, 1.0))[1] - 1             # ilogb
            s = np.ldexp(w, -ex)
            upd = ~done
            x = np.where(upd, s, x)
            done = np.where(upd, parallel, done)
            if bool((done | ~pivots_ok).all()):
                break
            n2 = (x * x).sum(0)
            a_ = np.einsum("nij,jn->in", G, x)
            rho = (x * a_).sum(0) / n2
            res = a_ - rho * x
            cand = rho - np.sqrt((res * res).sum(0) / n2)
            ok2, f2, _ = _ldl4(G, cand, False)
            take = ~done & (cand > sigma) & ok2
            f = np.where(take, f2, f)
            sigma = np.where(take, cand, sigma)
            shifted |= take
    out = ["declined" if not (d and p_) else ("shifted" if s_ else "first") for d, p_, s_ in zip(done, pivots_ok, shifted)]
    return (out, raw) if details else out
