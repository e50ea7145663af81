"""Inputs, references and error bars of the geometry tests, all on the CPU: the camera records, point clouds, DLT inputs and
degenerate tokens that tests/test_geometry_fp64.py runs on the GPU, and whose properties (share of border pairs, visibility of
the distortion terms, coincident eigenvalues) tests/test_geom_ref_oracle.py checks without a device."""
import math
from fractions import Fraction

import numpy as np
import torch

from mvgformer_amd import synthetic as S
from tests import geom_ref as R

SENT_F = -7.25e5
EPS32 = 2.0 ** -23
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16

IMG_WH, ORIG_WH = (320, 192), (640, 360)
TARGET = (0.0, -200.0, 800.0)
STRONG_K, STRONG_P = (-0.30, 0.12, 0.02), (5e-3, -4e-3)
CENTERS = ((320.0, 180.0), (300.0, 190.0))        # per batch element: image sizes (640, 360) and (600, 380)


def bf_next(x, up):
    """the bf16 value next to the bf16-valued x towards +inf (up) or -inf, by its bit pattern."""
    t = x.to(BF16)
    b = t.view(torch.int16).int()
    if up:
        n = torch.where(t > 0, b + 1, torch.where(t < 0, b - 1, torch.ones_like(b)))
    else:
        n = torch.where(t > 0, b - 1, torch.where(t < 0, b + 1, torch.full_like(b, -32767)))
    return n.to(torch.int16).view(BF16).double()


# ------------------------------------------------------------------------------------------------------------ CPU builders
def camera_records(V, B=2, rotated=False):
    """(V * B, 48) fp32 records (image n = v * B + b) of ring cameras with fy = 1.08 fx, per-batch-element image centres (the
    clamp bound [35] is the batch's largest side, 640, not every image's own), strong distortion on images 0 and 3, none on
    image 4.  rotated: the inverse crop affine of images 0 and 2 becomes a similarity with a 20 degree rotation."""
    from mvgformer_amd import ops
    cams = S.ring_cameras(V, ORIG_WH, 480.0, 3200.0, TARGET, (-0.12, 0.06, 0.01), (2e-3, -1.5e-3), seed=11)
    meta = S.make_meta(cams, B, ORIG_WH, IMG_WH)
    for m in meta:
        for b in range(B):
            c = np.array(CENTERS[b % 2])
            m["center"][b] = torch.from_numpy(c)
            m["inv_affine_trans"][b, :2] = torch.from_numpy(S.crop_affine(c, m["scale"][b].numpy(), IMG_WH, inv=True))
    rec = ops.pack_cameras(meta, IMG_WH, "cpu").clone()
    N = V * B
    rec[:, 13] = rec[:, 12] * 1.08
    strong = {0, 3 % N}
    for n in strong:
        rec[n, 16:19] = torch.tensor(STRONG_K)
        rec[n, 19:21] = torch.tensor(STRONG_P)
    if 4 % N not in strong:
        rec[4 % N, 16:21] = 0.0
    if rotated:
        th = math.radians(20.0)
        for n in (0, 2 % N):
            s = float(rec[n, 27])
            M = s * np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
            t = rec[n, 33:35].double().numpy() / 2 - M @ (np.array(IMG_WH, dtype=np.float64) / 2)
            rec[n, 27:33] = torch.tensor([M[0, 0], M[0, 1], t[0], M[1, 0], M[1, 1], t[1]])
    return rec


def _backproject(c, uv, z):
    """the points at depth z [mm] whose distorted projection by record c is the pixel uv (fixed-point inverse of the distortion)."""
    c = c.double()
    x0, y0 = (uv[:, 0] - c[14]) / c[12], (uv[:, 1] - c[15]) / c[13]
    k1, k2, k3, p1, p2 = (c[16 + i] for i in range(5))
    x, y = x0, y0
    for _ in range(40):
        r2 = x * x + y * y
        icd = 1 / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        x, y = (x0 - (2 * p1 * x * y + p2 * (r2 + 2 * x * x))) * icd, (y0 - (p1 * (r2 + 2 * y * y) + 2 * p2 * x * y)) * icd
    return torch.stack([x * z, y * z, z], -1) @ c[0:9].view(3, 3) + c[9:12]


def project_cloud(rec, B=2, Lq=257, seed=5):
    """(B, Lq, 3) fp32 points for the records of camera_records(3, B): a cloud inside the scene, rows of points from 32 px inside
    to 32 px outside each of the four borders of view 0, points behind each of the three cameras, far-off-axis points of view 0
    that end at both clamps, and a wide cloud."""
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=F64)
    uni = lambda n, lo, hi: lo + (hi - lo) * torch.rand(n, generator=gen, dtype=F64)
    tgt = torch.tensor(TARGET, dtype=F64)
    out = []
    for b in range(B):
        c0 = rec[b].double()
        w, h = float(c0[33]), float(c0[34])
        pts = [tgt + rnd(100, 3) * torch.tensor([700.0, 700.0, 500.0], dtype=F64)]
        d = torch.tensor([0.25, 0.5, 1, 2, 4, 8, 16, 32], dtype=F64)
        d = torch.cat([d, -d])
        for side in range(4):
            along = uni(16, 20.0, (h if side < 2 else w) - 20.0)
            uv = [torch.stack([-d, along], -1), torch.stack([w + d, along], -1), torch.stack([along, -d], -1),
                  torch.stack([along, h + d], -1)][side]
            pts.append(_backproject(c0, uv, uni(16, 2500.0, 4000.0)))
        for v in range(3):
            c = rec[v * B + b].double()
            xc = torch.cat([rnd(8, 2) * 500.0, -uni(8, 1500.0, 3000.0)[:, None]], -1)
            pts.append(xc @ c[0:9].view(3, 3) + c[9:12])
        z = uni(16, 2000.0, 3500.0)
        sg = torch.tensor([[1.0, 1.0], [1.0, -1.0], [-1.0, 1.0], [-1.0, -1.0]], dtype=F64).repeat(4, 1)
        pts.append(torch.cat([sg * 4.5 * z[:, None], z[:, None]], -1) @ c0[0:9].view(3, 3) + c0[9:12])
        n = sum(p.shape[0] for p in pts)
        pts.append(tgt + rnd(Lq - n, 3) * torch.tensor([2500.0, 2500.0, 1200.0], dtype=F64))
        out.append(torch.cat(pts))
    return torch.stack(out).float()


def z_cam(X, rec):
    """(V * B, Lq) depth of every point in every camera, fp64."""
    c = rec.double()
    B = X.shape[0]
    Xn = X.double()[torch.arange(c.shape[0]) % B]
    return ((Xn - c[:, None, 9:12]) * c[:, None, 6:9]).sum(-1)


def bar32(ref64, ref32, eps=EPS32):
    """4 x the largest error of the fp32 evaluation of the reference + 2 ulp of the value (elementwise)."""
    return 4.0 * float((ref32.double() - ref64).abs().max()) + 2.0 * eps * ref64.abs()


def inside_margin(u64, u32, wh):
    """distance from a border below which `inside` is not compared: the error of the reference's own fp32 pixel -- 4 x the larger
    of the pair's own error and the largest error among the pairs within one image size of the image -- + 2 ulp."""
    e = (u32.double() - u64).abs()
    box = ((u64 > -wh) & (u64 < 2 * wh)).all(-1, keepdim=True)
    e_box = float((e * box).max())
    return 4.0 * torch.clamp(e, min=e_box) + 2.0 * EPS32 * torch.maximum(u64.abs(), wh)


def border_distance(u64, wh):
    return torch.minimum(u64.abs(), (u64 - wh).abs()).amin(-1)


def uncrop_points(B=2, V=3, Lq=129, seed=6):
    """(B, V, Lq, 2) fp32 network-image pixels spread over and 15 % beyond the image."""
    gen = torch.Generator().manual_seed(seed)
    return ((torch.rand(B, V, Lq, 2, generator=gen, dtype=F64) * 1.3 - 0.15) * torch.tensor(IMG_WH, dtype=F64)).float()


def dlt_inputs(V, B=2, NQ=9, J=15, seed=7):
    """fp32 (Pm (B, V, 3, 4), ud (B, V, Lq, 2), conf (B, V, Lq), gX (B, Lq, 3)): projection matrices of camera_records(V, B), exact
    pinhole projections of points in the scene + 2 px noise, softmax confidences."""
    gen = torch.Generator().manual_seed(seed + 100 * V + J)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=F64)
    Lq = NQ * J
    Pm = R.proj_matrices(camera_records(V, B), V, B).float()
    X = torch.tensor(TARGET, dtype=F64) + rnd(B, Lq, 3) * torch.tensor([600.0, 600.0, 400.0], dtype=F64)
    uvw = torch.einsum("bvij,bnj->bvni", Pm.double(), torch.cat([X, torch.ones(B, Lq, 1, dtype=F64)], -1))
    ud = (uvw[..., :2] / uvw[..., 2:3] + rnd(B, V, Lq, 2) * 2.0).float()
    conf = torch.softmax(rnd(B, V, Lq), 1).float()
    return Pm, ud, conf, rnd(B, Lq, 3).float()


def degenerate_token():
    """A two-view token (Pm (1, 2, 3, 4), ud (1, 2, 1, 2), conf (1, 2, 1)) whose four rows are 2 (1,0,0,1), 2 (0,1,1,0), (1,0,0,-1),
    (0,1,-1,0): small integers, so its fp64 Gram matrix [[5,0,0,3],[0,5,3,0],[0,3,5,0],[3,0,0,5]] is exact and symmetric under
    exchanging the coordinate pairs (0, 3) and (1, 2): eigenvalues 8, 8, 2, 2 -- the two smallest coincide."""
    Pm = torch.tensor([[[-2.0, 0, 0, -2], [0, -2, -2, 0], [0, 0, 0, 1]], [[-1.0, 0, 0, 1], [0, -1, 1, 0], [0, 0, 1, 1]]])[None]
    return Pm, torch.zeros(1, 2, 1, 2), torch.ones(1, 2, 1)


def _rn(fr):
    return float(fr)          # Fraction -> the nearest double (round to nearest even)


def boundary_token():
    """A two-view token whose fp64 Gram matrix is diagonal with eigenvalues (1, t, ~1/4, 0), t = fl(1e-14) to the last bit: the gap
    between the smallest eigenvalue (0, eigenvector e3: X = 0) and t EQUALS the backward's threshold 1e-14 * max |l|.  The kernels
    accumulate a diagonal entry as fl(fl(r1^2) + r2^2) (one rounded square, one fma): r1 = the fp32 value below sqrt(t),
    r2 = p2 * cf2 (a product of two fp32 values, exact in fp64) chosen so that the sum rounds to t.  Returns (Pm, ud, conf, t)."""
    t = 1e-14 * 1.0
    r1 = float(np.nextafter(np.float32(math.sqrt(t)), np.float32(0)))
    a = _rn(Fraction(r1) ** 2)
    delta = Fraction(t) - Fraction(a)
    assert delta > 0
    for i in range(1, 4096):                         # r2^2 must hit delta to 2^-30: about one fp32 pair in 64 does
        cf2 = float(np.float32(2.0 ** -20 * (1.0 + i / 4096.0)))
        p2 = float(np.float32(math.sqrt(float(delta)) / cf2))
        r2 = p2 * cf2
        if _rn(Fraction(r2) ** 2 + Fraction(a)) == t:
            break
    else:
        raise AssertionError("no fp32 pair reaches the threshold")
    d = float(np.float32(0.5 / cf2))                 # the fourth row: (0, 0, d * cf2, 0), about (0, 0, 1/2, 0)
    Pm = torch.tensor([[[0.0, -r1, 0, 0], [-1.0, 0, 0, 0], [0, 0, 0, 1]], [[0.0, -p2, 0, 0], [0, 0, -d, 0], [0, 0, 0, 1]]],
                      dtype=F64)[None].float()
    conf = torch.tensor([[[1.0], [cf2]]])
    assert float(Pm[0, 0, 0, 1]) == -r1 and float(Pm[0, 1, 0, 1]) == -p2
    return Pm, torch.zeros(1, 2, 1, 2), conf, t


def eig_families(seed=8):
    """(257, 4, 4) fp64 matrices at scale 1: random SPD, indefinite, diagonal, zero, diag(1,1,2,2) rotated (repeated eigenvalues),
    graded with condition number 1e12, non-symmetric."""
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=F64)
    A = rnd(40, 6, 4)
    spd = A.transpose(1, 2) @ A / 6
    ind = rnd(40, 4, 4)
    ind = 0.5 * (ind + ind.transpose(1, 2))
    dg = torch.diag_embed(rnd(36, 4))
    zero = torch.zeros(5, 4, 4, dtype=F64)
    Q = torch.linalg.qr(rnd(80, 4, 4))[0]
    rep = Q[:40] @ torch.diag(torch.tensor([1.0, 1, 2, 2], dtype=F64)) @ Q[:40].transpose(1, 2)
    rep = 0.5 * (rep + rep.transpose(1, 2))
    grd = Q[40:] @ torch.diag(torch.tensor([1.0, 1e-4, 1e-8, 1e-12], dtype=F64)) @ Q[40:].transpose(1, 2)
    grd = 0.5 * (grd + grd.transpose(1, 2))
    ns = rnd(56, 4, 4)
    G = torch.cat([spd, ind, dg, zero, rep, grd, ns])
    perm = torch.randperm(G.shape[0], generator=gen)            # every family within the first 255 and in both workgroups
    assert G.shape[0] == 257
    return G[perm]


def eig_figures(G, w, V):
    """(residual |G V - V diag(w)|, |V^T V - I|, sorted w against eigvalsh), each the largest over the batch of
    max-entry / largest |entry of G| (the zero matrix: absolute), for the symmetric part of G."""
    Gs = 0.5 * (G + G.transpose(1, 2))
    nrm = Gs.abs().amax((1, 2)).clamp_min(1e-300)
    res = ((Gs @ V - V * w[:, None, :]).abs().amax((1, 2)) / nrm).max()
    orth = (V.transpose(1, 2) @ V - torch.eye(4, dtype=F64)).abs().amax((1, 2)).max()
    ev = ((w.sort(-1)[0] - torch.linalg.eigvalsh(Gs)).abs().amax(-1) / nrm).max()
    return float(res), float(orth), float(ev)



PROJ_SHAPES = {1: [(5, 9)], 4: [(48, 80), (5, 9), (2, 3), (24, 40)]}

def dlt_reference(Pm, ud, conf, gX, tok):
    """fp64 SVD and its autograd on the tokens flagged in tok (B, Lq): (X, g_ud, g_conf) dense, zeros elsewhere."""
    bi, ti = tok.nonzero(as_tuple=True)
    p, c = ud.double().clone().requires_grad_(True), conf.double().clone().requires_grad_(True)
    X = torch.zeros(tok.shape + (3,), dtype=F64)
    if bi.numel():
        ref = R.dlt(Pm.double()[bi], p[bi, :, ti].unsqueeze(2), c[bi, :, ti].unsqueeze(2))[:, 0]
        (ref * gX.double()[bi, ti]).sum().backward()
        X[bi, ti] = ref.detach()
    z = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    return X, z(p), z(c)


def dlt_bars(Pm, ud, conf, gX, tok, ref, seed=3):
    """4 x the change of the fp64 reference under half an fp32 ulp on every input (random signs) + 2 ulp of the fp32 output."""
    gen = torch.Generator().manual_seed(seed)
    half = lambda t: t.double() * (1.0 + (torch.randint(0, 2, t.shape, generator=gen).double() * 2 - 1) * 2.0 ** -24)
    pert = dlt_reference(half(Pm), half(ud), half(conf), gX, tok)
    return [4.0 * float((a - b).abs().max()) + 2.0 * EPS32 * b.abs() for a, b in zip(pert, ref)]


def _valid(kind, B, NQ, gen):
    if kind == "mixed":
        v = (torch.rand(B, NQ, generator=gen) < 0.6).to(torch.uint8)
        v[0, 0], v[0, 1] = 1, 0
    else:
        v = torch.zeros(B, NQ, dtype=torch.uint8)
        if kind == "last":
            v[-1, -1] = 1
    return v



PYR_SHAPES = [(5, 13), (3, 7), (1, 2)]
PYR_STARTS = [0, 70, 96]            # 5 rows of gap behind every level
PYR_S = 103


def _pyramid_src(C_, seed=9):
    gen = torch.Generator().manual_seed(seed + C_)
    return [torch.randn(3, C_, H, W, generator=gen) for H, W in PYR_SHAPES]



def _gather_points(N, Lq, gen):
    """(N, Lq, L, 2) reference points: pixel centres, the corners, 0, 1, -0.06 and 1.06 (past the +-1.1 clamp in grid units), random."""
    ref = torch.rand(N, Lq, len(PYR_SHAPES), 2, generator=gen) * 1.2 - 0.1
    for l, (H, W) in enumerate(PYR_SHAPES):
        sp = [(0.0, 0.0), (1.0, 1.0), (0.0, 1.0), (1.0, 0.0), (-0.06, 0.5), (1.06, 0.5), (0.5, -0.06), (0.5, 1.06), (-0.06, 1.06)]
        sp += [((x + 0.5) / W, (y + 0.5) / H) for y in range(H) for x in range(min(W, 7))]
        ref[:, :len(sp), l] = torch.tensor(sp)[:Lq]
    return ref
