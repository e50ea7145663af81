"""Inputs of the triangulation tests, all seeded and built on the CPU: tests/test_tri_fp64.py runs them through triangulate_kernel
on the GPU, tests/test_tri_ref_cpu.py checks without a device that they reach what they are meant to reach.

A case is one launch: cameras of geom_cases.camera_records(V, B[, rotated]), a cloud of points around TARGET small enough that every
point projects inside every image (no clamp: the rays of class `meet` do meet), r = geom_ref.project(X, rec)[0].float(), and per
QUERY one of the classes below, which set the offsets o_xy [px] and the view logits:

    meet         o_xy = 0            logits N(0, 1)   the last pivot of the first factorisation is rounding noise of either sign
    noise2       N(0, 2 px)          N(0, 1)          the ordinary case
    off30        N(0, 30 px)         N(0, 1)          rays that do not meet: the shifted rounds
    off300       N(0, 300 px)        N(0, 1)
    logit_edges  N(0, 2 px)          by joint slot, in turn: all +80; all -1e4; a ramp from 0 to -100 (the trailing weight is an fp32
                                     subnormal, 3.8e-44); the same ramp to -120 (the trailing weight underflows to exactly 0).  The ramp
                                     is cubic in the view index, -100 (v / (V - 1))^3, so that the leading views keep comparable
                                     weight; it is used from V = 7 on (over two or three views it leaves ONE view: `degenerate`)
    degenerate   N(0, 2 px)          one view 0, the others -60: one useful view, the Jacobi fallback.  Every problem of V = 1 is one.

With rotated records the inverse crop affine of two images is no longer the inverse of their crop affine, so r is taken through
the inverse of the INVERSE affine instead (the kernel only ever sees the inverse one): the rays still meet."""
import functools

import torch

from tests import geom_ref as R
from tests.geom_cases import F64, TARGET, camera_records

CLASSES = ("meet", "noise2", "off30", "off300", "logit_edges")
OFFSET_PX = {"meet": 0.0, "noise2": 2.0, "off30": 30.0, "off300": 300.0, "logit_edges": 2.0, "degenerate": 2.0}
EDGE_KINDS = ("all+80", "all-1e4", "ramp-100", "ramp-120")
SPREAD = (220.0, 220.0, 180.0)                  # mm: 4 sigma stays inside the 640 x 360 images of cameras 3.2 m away
RAMP_MIN_V = 7

# (B, NQ, J): 1, 63, 64, 65 and 129 problems (one problem more or less than whole 64-problem workgroups, B = 1, 2, 3), and J = 15 and
# J = 17 at counts that are no multiple of 64 either
SHAPES = ((1, 1, 1), (1, 63, 1), (2, 32, 1), (1, 65, 1), (3, 43, 1), (2, 3, 15), (3, 5, 17))
VIEWS = (1, 2, 3, 7, 8, 9, 16, 17, 32)
RAGGED = (3, 5, 17)                             # every V runs at this shape: 255 problems, 4 workgroups, B = 3
FEW_V = (2, 9, 32)                              # ... and these at every shape
MEET_ONLY_V = (2, 3)                            # ... and 255 problems of class `meet` alone: about 3 % of their last pivots are negative


def query_classes(B, NQ, classes=CLASSES):
    """(B, NQ) list of lists: class of every query, in turn (shifted by the batch element)."""
    return [[classes[(i + b) % len(classes)] for i in range(NQ)] for b in range(B)]


def ramp(V, end):
    v = torch.arange(V, dtype=F64) / max(V - 1, 1)
    return end * v ** 3


@functools.lru_cache(maxsize=None)
def _base(V, B, NQ, J, rotated, seed):
    gen = torch.Generator().manual_seed(1000 * seed + 100 * V + 10 * B + NQ + J)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=F64)
    Lq = NQ * J
    rec = camera_records(V, B, rotated)
    X = (torch.tensor(TARGET, dtype=F64) + rnd(B, Lq, 3) * torch.tensor(SPREAD, dtype=F64)).float()
    r, _, inside, u = R.project(X, rec, [(8, 8)])
    if rotated:
        c = rec.double()
        M = c[:, 27:33].view(-1, 2, 3)
        kp = torch.linalg.solve(M[:, None, :, :2].expand(-1, Lq, -1, -1), u - M[:, None, :, 2])
        r = kp / c[:, None, 36:38]
    return rec, X, r.float().contiguous(), inside, rnd(V, B, Lq), rnd(V, B, Lq, 2)


def tri_case(V, B, NQ, J, classes=None, rotated=False, seed=0):
    """-> dict(r (V*B, Lq, 2), o (V*B, Lq, 3), rec (V*B, 48), X (B, Lq, 3), inside (V*B, Lq), cls: (B, Lq) list of class names,
    kind: (B, Lq) list of the logit_edges kind or None).  classes: (B, NQ) class names (default query_classes)."""
    rec, X, r, inside, logit, noise = _base(V, B, NQ, J, rotated, seed)
    classes = classes or query_classes(B, NQ)
    Lq = NQ * J
    o = torch.zeros(V, B, Lq, 3, dtype=F64)
    cls, kind = [[None] * Lq for _ in range(B)], [[None] * Lq for _ in range(B)]
    for b in range(B):
        for i in range(NQ):
            for j in range(J):
                q = i * J + j
                c = classes[b][i]
                if V == 1:
                    c = "degenerate"
                cls[b][q] = c
                o[:, b, q, :2] = noise[:, b, q] * OFFSET_PX[c]
                o[:, b, q, 2] = logit[:, b, q]
                if c == "logit_edges":
                    k = EDGE_KINDS[(j if J > 1 else i // len(CLASSES)) % (4 if V >= RAMP_MIN_V else 2)]
                    kind[b][q] = k
                    o[:, b, q, 2] = {"all+80": torch.full((V,), 80.0, dtype=F64), "all-1e4": torch.full((V,), -1e4, dtype=F64),
                                     "ramp-100": ramp(V, -100.0), "ramp-120": ramp(V, -120.0)}[k]
                elif c == "degenerate":
                    o[:, b, q, 2] = -60.0
                    o[q % V, b, q, 2] = 0.0
    return dict(r=r, o=o.float().view(V * B, Lq, 3).contiguous(), rec=rec, X=X, inside=inside, cls=cls, kind=kind, V=V, B=B, NQ=NQ, J=J)


def groups(case, tok):
    """{name: (B, Lq) bool} of the computed problems of each class present in the case, logit_edges split by kind: one yardstick each."""
    B, Lq = tok.shape
    out = {}
    for b in range(B):
        for q in range(Lq):
            if not bool(tok[b, q]):
                continue
            c = case["cls"][b][q]
            name = c if case["kind"][b][q] is None else "%s/%s" % (c, case["kind"][b][q])
            out.setdefault(name, torch.zeros(B, Lq, dtype=torch.bool))[b, q] = True
    return out


def main_cases():
    """(V, B, NQ, J) of the comparison with fp64: every V > 1 at the ragged shape, a few V at every shape."""
    out = [(V,) + RAGGED for V in VIEWS if V > 1]
    out += [(V,) + s for V in FEW_V for s in SHAPES if s != RAGGED]
    return out


def meet_only(B, NQ):
    return tuple(("meet",) * NQ for _ in range(B))


def all_valid(B, NQ):
    return torch.ones(B, NQ, dtype=torch.uint8)
