"""Plain torch statements of the camera-geometry operations of csrc/geom.hip (mvg_project, mvg_uncrop_undistort_jac,
mvg_dlt_forward / mvg_dlt_backward, mvg_pack_pyramid, mvg_gather_ref), fp64 by default, `dtype=` selectable, on the CPU.
They take the packed camera records (ops.pack_cameras: 48 floats per image, image n = v * B + b) directly, so a test can
hand over cameras that pack_cameras cannot build (an inverse crop affine with a rotation).  Differentiable where the
kernels have a backward.  Pinned to oracle/decoder_ref.py by tests/test_geom_ref_oracle.py; the GPU tests
(tests/test_geometry_fp64.py) compare the kernels with these statements.

Record layout: R 0:9 (row major), T 9:12, fx fy cx cy 12:16, k1 k2 k3 16:19, p1 p2 19:21, crop affine (2, 3) 21:27, inverse
crop affine (2, 3) 27:33, image (w, h) 33:35, clamp bound 35 (the batch's largest image side), network image (w, h) 36:38."""
import torch
import torch.nn.functional as F

F64 = torch.float64
STRIDE = 48


def _rec(cams, dtype):
    return cams.detach().cpu().reshape(-1, STRIDE).to(dtype)


def project(X, cam_records, shapes, dtype=F64):
    """X (B, Lq, 3) mm; records (V * B, 48); shapes [(H, W)] * L.  Returns r (V*B, Lq, 2) normalised network-image coordinates,
    ref_lvl (V*B, Lq, L, 2), inside (V*B, Lq) bool, and u (V*B, Lq, 2): the pixel in the original image BEFORE the clamp."""
    c = _rec(cam_records, dtype)
    n_img, B = c.shape[0], X.shape[0]
    X = X.detach().cpu().to(dtype)[torch.arange(n_img) % B]                         # (n, Lq, 3)
    R, T = c[:, 0:9].view(n_img, 3, 3), c[:, 9:12].view(n_img, 1, 3)
    xc = (X - T) @ R.transpose(1, 2)                                               # x_cam = R (x - T)
    y = xc[..., :2] / (xc[..., 2:3] + 1e-5)
    r2 = (y * y).sum(-1, keepdim=True)
    k, p = c[:, None, 16:19], c[:, None, 19:21]
    radial = 1 + (k[..., 0:1] * r2 + k[..., 1:2] * r2 ** 2 + k[..., 2:3] * r2 ** 3)
    tang = p[..., 0:1] * y[..., 1:2] + p[..., 1:2] * y[..., 0:1]
    y = y * (radial + 2 * tang) + p.flip(-1) * r2
    u = c[:, None, 12:14] * y + c[:, None, 14:16]
    wh = c[:, None, 33:35]
    inside = ((u >= 0) & (u < wh)).all(-1)
    uc = torch.minimum(torch.clamp(u, min=-1.0), c[:, None, 35:36])
    A = c[:, 21:27].view(n_img, 2, 3)
    nimg = uc @ A[:, :, :2].transpose(1, 2) + A[:, None, :, 2]
    r = nimg / c[:, None, 36:38]
    WH = torch.tensor([[float(w), float(h)] for h, w in shapes], dtype=dtype)       # (L, 2)
    ref_lvl = r.unsqueeze(2) * WH / (WH - 1)
    return r, ref_lvl, inside, u


def uncrop_undistort(ref2d, cam_records, dtype=F64, iters=5):
    """ref2d (B, V, Lq, 2) network-image px -> undistorted original-image px (B, V, Lq, 2): inverse crop affine, K^-1, five
    fixed-point iterations of the distortion model, K.  Differentiable in ref2d."""
    B, V = ref2d.shape[:2]
    c = _rec(cam_records, dtype).view(V, B, STRIDE).transpose(0, 1)[:, :, None]     # (B, V, 1, 48)
    kp = ref2d.to(dtype)
    uo = c[..., 27] * kp[..., 0] + c[..., 28] * kp[..., 1] + c[..., 29]
    vo = c[..., 30] * kp[..., 0] + c[..., 31] * kp[..., 1] + c[..., 32]
    fx, fy, cx, cy = c[..., 12], c[..., 13], c[..., 14], c[..., 15]
    k1, k2, k3, p1, p2 = (c[..., 16 + i] for i in range(5))
    x0 = uo * (1 / fx) + (-cx / fx)
    y0 = vo * (1 / fy) + (-cy / fy)
    x, y = x0, y0
    for _ in range(iters):
        r2 = x * x + y * y
        icd = 1 / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dX = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dY = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x, y = (x0 - dX) * icd, (y0 - dY) * icd
    return torch.stack([fx * x + cx, fy * y + cy], -1)


def uncrop_undistort_jac(ref2d, cam_records, dtype=F64):
    """(ud, jac (B, V, Lq, 2, 2) = d ud / d ref2d) by autograd: every point depends on its own input only, so two vectorised
    passes (one per output component) give the whole Jacobian."""
    x = ref2d.detach().cpu().to(dtype).requires_grad_(True)
    ud = uncrop_undistort(x, cam_records, dtype)
    rows = [torch.autograd.grad(ud[..., i].sum(), x, retain_graph=True)[0] for i in range(2)]
    return ud.detach(), torch.stack(rows, -2)


def proj_matrices(cam_records, V, B, dtype=F64):
    """(B, V, 3, 4) projection matrices K [R | -R T] of the records."""
    c = _rec(cam_records, dtype).view(V, B, STRIDE).transpose(0, 1)
    R, T = c[..., 0:9].reshape(B, V, 3, 3), c[..., 9:12].reshape(B, V, 3, 1)
    K = torch.zeros((B, V, 3, 3), dtype=dtype)
    K[..., 0, 0], K[..., 1, 1], K[..., 0, 2], K[..., 1, 2] = c[..., 12], c[..., 13], c[..., 14], c[..., 15]
    K[..., 2, 2] = 1
    return K @ torch.cat([R, -R @ T], -1)


def dlt_rows(Pm, ud, conf):
    """the (B, N, 2V, 4) row matrices conf * (u * P[2] - P[0]), conf * (v * P[2] - P[1])."""
    pt = ud.permute(0, 2, 1, 3)                                                     # (B, N, V, 2)
    A = Pm[:, None, :, 2:3, :] * pt[..., None]
    A = A - Pm[:, None, :, :2, :]
    A = A * conf.permute(0, 2, 1)[..., None, None]
    return A.reshape(A.shape[0], A.shape[1], -1, 4)


def dlt(Pm, ud, conf):
    """Pm (B, V, 3, 4), ud (B, V, N, 2), conf (B, V, N) -> X (B, N, 3): the right singular vector of the smallest singular value
    of the row matrix, dehomogenised.  In the dtype of its arguments; differentiable in ud and conf."""
    _, _, Vh = torch.linalg.svd(dlt_rows(Pm, ud, conf))
    Xh = -Vh[..., 3, :]
    return Xh[..., :3] / Xh[..., 3:4]


def pack_pyramid(src_views, shapes, starts, S, dtype=F64, fill=0.0):
    """L maps (N, C, H_l, W_l) -> (N, S, C): pixel (y, x) of level l is row starts[l] + y * W_l + x; other rows hold `fill`."""
    N, C = src_views[0].shape[:2]
    out = torch.full((N, S, C), fill, dtype=dtype)
    for src, (H, W), st in zip(src_views, shapes, starts):
        out[:, st:st + H * W] = src.detach().cpu().to(dtype).reshape(N, C, H * W).transpose(1, 2)
    return out


def gather_ref(feat, ref_lvl, x, shapes, starts, dtype=F64):
    """feat (N, S, C), ref_lvl (N, Lq, L, 2) as (x, y) in [0, 1], x (B, Lq, C) (image n belongs to batch element n % B) ->
    (N, Lq, L, C): bilinear sample of each level at clamp(2 ref - 1, -1.1, 1.1) (grid_sample, zero padding, align_corners=False)
    plus the query row."""
    N, _, C = feat.shape
    feat, ref_lvl, x = feat.detach().cpu().to(dtype), ref_lvl.detach().cpu().to(dtype), x.detach().cpu().to(dtype)
    B = x.shape[0]
    out = []
    for l, ((H, W), st) in enumerate(zip(shapes, starts)):
        img = feat[:, st:st + H * W].view(N, H, W, C).permute(0, 3, 1, 2)
        grid = torch.clamp(ref_lvl[:, :, l] * 2.0 - 1.0, -1.1, 1.1).unsqueeze(2)   # (N, Lq, 1, 2)
        s = F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False)   # (N, C, Lq, 1)
        out.append(s[..., 0].transpose(1, 2))
    return torch.stack(out, 2) + x[torch.arange(N) % B].unsqueeze(2)
