"""triangulate_kernel of csrc/geom.hip (mvg_triangulate, mvg_triangulate_project) against the fp64 statement of tests/tri_ref.py
(pinned to the oracle by tests/test_tri_ref_cpu.py), at the view counts, problem counts, masks and inputs where its code can go wrong
unseen.  Inputs: tests/tri_cases.py, whose properties tests/test_tri_ref_cpu.py checks without a device.

Error bars (measured from the reference, never from the kernel).  ref2d, proj2d: bar32 of the statement (4 x the largest error of its
fp32 evaluation + 2 ulp), every element.  new_ref: the yardstick is the statement with everything up to the rows in fp32 and the solve
in fp64 -- the kernel's own split -- against the statement in fp64, largest error over the launch's problems of one class
(logit_edges: of one kind); the kernel gets 4 x that + 2 ulp, in millimetres for meet, noise2 and logit_edges, and as tri_ref.gap_figure
for meet, noise2, off30 and off300 (rays that do not meet put the point up to 4e5 mm away, where millimetres mean nothing).  Every
comparison prints max err / bar.  Launches are raw C-ABI calls on buffers pre-filled with a NaN of a payload no arithmetic produces,
between sentinel guards: every element must come back written, the guards untouched."""
import ctypes as C_
import functools

import pytest
import torch

from tests import geom_ref as R
from tests import tri_cases as C
from tests import tri_ref as T
from tests.geom_cases import F32, PROJ_SHAPES, SENT_F, _valid, bar32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 1024
SENT_U8, FILL_U8 = 0xA5, 0xEE
FILL_NAN = 0x7FC0BEEF                                  # a quiet NaN with a payload
BADARG = 10001                                         # MVG_E_BADARG
MM_CLASSES = ("meet", "noise2", "logit_edges")
GAP_CLASSES = ("meet", "noise2", "off30", "off300")
I32 = torch.int32


def _lib():
    from mvgformer_amd import _lib as L
    return L


def _i64(rows):
    flat = [int(x) for r in rows for x in r]
    return (C_.c_int64 * len(flat))(*flat)


class Out:
    """n elements pre-filled with the NaN (uint8: 0xEE) between two guards of the sentinel."""

    def __init__(self, n, dtype=F32):
        self.n, self.u8 = n, dtype == torch.uint8
        self.buf = torch.full((2 * GUARD + n,), SENT_U8 if self.u8 else SENT_F, dtype=dtype, device=DEV)
        self.mid = self.buf[GUARD:GUARD + n]
        if self.u8:
            self.mid.fill_(FILL_U8)
        elif n:
            self.mid.view(I32).fill_(FILL_NAN)
        self.before = self.buf.clone()

    def ptr(self):
        """address of the first element (also when n = 0, where an empty tensor has no address of its own)"""
        return C_.c_void_p(self.buf.data_ptr() + GUARD * self.buf.element_size())

    def guards_ok(self):
        s = SENT_U8 if self.u8 else SENT_F
        return bool((self.buf[:GUARD] == s).all()) and bool((self.buf[GUARD + self.n:] == s).all())

    def all_written(self):
        return not bool((self.mid == FILL_U8).any() if self.u8 else (self.mid.view(I32) == FILL_NAN).any())

    def untouched(self):
        b = (self.buf, self.before) if self.u8 else (self.buf.view(I32), self.before.view(I32))
        return torch.equal(*b)


def launch(r, o, rec, valid, any_valid, V, B, NQ, J, shapes=None, null=(), expect=0):
    """one raw launch of mvg_triangulate (shapes None) or mvg_triangulate_project on guarded outputs -> dict of CPU tensors (+ the
    device new_ref).  null: names of arguments passed as null pointers.  Asserts the return code, the guards, and that every element
    was written (rc 0, at least one problem) or none (otherwise)."""
    Lm = _lib()
    Lq = NQ * J
    n = B * Lq
    outs = dict(new_ref=Out(n * 3), ref2d=Out(n * V * 2), proj2d=Out(n * V * 2))
    dev = dict(r=r.to(DEV).contiguous(), o=o.to(DEV).contiguous(), cams=rec.to(DEV).contiguous(), valid=valid.to(DEV).contiguous(),
               any_valid=torch.tensor([int(any_valid)], dtype=I32, device=DEV))           # held until the launch has finished
    p = lambda name: None if name in null else (outs[name].ptr() if name in outs else Lm.ptr(dev[name]))
    args = [p(k) for k in ("r", "o", "cams", "valid", "any_valid", "new_ref", "ref2d", "proj2d")] + [V, B, NQ, J]
    if shapes is None:
        rc = Lm.load().mvg_triangulate(*args, Lm.stream_ptr())
    else:
        L = len(shapes)
        outs.update(r_next=Out(n * V * 2), ref_lvl_next=Out(n * V * L * 2), inside_next=Out(n * V, torch.uint8))
        sh = None if "shapes_host" in null else _i64(shapes)
        rc = Lm.load().mvg_triangulate_project(*args, sh, L, p("r_next"), p("ref_lvl_next"), p("inside_next"), Lm.stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, rc
    for k, ob in outs.items():
        assert ob.guards_ok(), k
        assert (ob.all_written() if rc == 0 and n and V > 0 else ob.untouched()), k
    res = {k: ob.mid.clone() for k, ob in outs.items()}
    res["new_ref_dev"] = res["new_ref"].view(B, Lq, 3) if n else None
    view = dict(new_ref=(B, Lq, 3), ref2d=(B, V, Lq, 2), proj2d=(B, V, Lq, 2), r_next=(V * B, Lq, 2), inside_next=(V * B, Lq))
    for k in outs:
        res[k] = res[k].cpu().view(view[k]) if k in view else res[k].cpu().view(V * B, Lq, len(shapes), 2)
    return res


def launch_case(case, valid=None, any_valid=1, **kw):
    V, B, NQ, J = case["V"], case["B"], case["NQ"], case["J"]
    valid = C.all_valid(B, NQ) if valid is None else valid
    return launch(case["r"], case["o"], case["rec"], valid, any_valid, V, B, NQ, J, **kw)


def bits(t):
    return t.contiguous().view(I32 if t.dtype == F32 else torch.uint8)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def _refs_cached(key, valid_bytes, any_valid):
    V, B, NQ, J, rotated, seed, klass = key
    case = C.tri_case(V, B, NQ, J, classes=klass, rotated=rotated, seed=seed)
    valid = torch.tensor(list(valid_bytes), dtype=torch.uint8).view(B, NQ)
    return (T.triangulate(case["r"], case["o"], case["rec"], valid, any_valid, V, B, NQ, J),
            T.triangulate(case["r"], case["o"], case["rec"], valid, any_valid, V, B, NQ, J, dtype=F32))


def refs(case_key, valid, any_valid=1):
    """(fp64 statement, fp32 statement) of a case of tri_cases.tri_case: computed once per module, shared, never changed."""
    V, B, NQ, J = case_key[:4]
    extra = tuple(case_key[4:])
    rotated, seed, klass = extra + (False, 0, None)[len(extra):]
    klass = None if klass is None else tuple(tuple(x) for x in klass)
    return _refs_cached((V, B, NQ, J, rotated, seed, klass), bytes(valid.flatten().tolist()), int(any_valid))


def check(name, got, ref, bar):
    err = (got.double() - ref).abs()
    bar = bar if isinstance(bar, torch.Tensor) else torch.full_like(err, bar)
    ratio = float((err / bar.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print("%s: max err %.3e, max err / bar %.3f" % (name, float(err.max()) if err.numel() else 0.0, ratio))
    assert bool((err <= bar).all()), (name, ratio)
    return ratio


def compare(tag, case, out, ref64, ref32):
    """all three outputs of a launch against the statement: ref2d / proj2d every element, new_ref per class; exact zeros elsewhere."""
    x64, r64, p64, e64 = ref64
    x32, r32, p32, _ = ref32
    tok = e64["computed"]
    check(tag + " ref2d", out["ref2d"], r64, bar32(r64, r32))
    check(tag + " proj2d", out["proj2d"], p64, bar32(p64, p32))
    m4 = tok[:, None, :, None].expand_as(r64)
    assert bool((out["ref2d"][~m4] == 0).all()) and bool((out["proj2d"][~m4] == 0).all()) and bool((out["new_ref"][~tok] == 0).all())
    gk, g32 = T.gap_figure(out["new_ref"], e64), T.gap_figure(x32, e64)
    for name, m in sorted(C.groups(case, tok).items()):
        klass = name.split("/")[0]
        if klass in MM_CLASSES:
            check("%s %s n=%d new_ref [mm]" % (tag, name, int(m.sum())), out["new_ref"][m], x64[m], bar32(x64[m], x32[m]))
        if klass in GAP_CLASSES:
            check("%s %s n=%d new_ref [gap figure]" % (tag, name, int(m.sum())), gk[m], torch.zeros_like(gk[m]), 4.0 * float(g32[m].max()))


# ---------------------------------------------------------------------------------------------------------- against fp64
@pytest.mark.parametrize("V,B,NQ,J", C.main_cases(), ids=lambda v: str(v))
def test_triangulation_against_fp64(V, B, NQ, J):
    """every V of (2, 3, 7, 8, 9, 16, 17, 32) at 255 problems (B = 3, J = 17), V = 2, 9, 32 at 1, 63, 64, 65, 129, 90 problems: the clamp
    min(sub, V - 1), the second to fourth trip of the view loops, the -inf lanes of the 8-lane reductions and the idx = nprob - 1 clamp
    of the last workgroup; every class of tests/tri_cases.py in every launch of more than one query."""
    case = C.tri_case(V, B, NQ, J)
    out = launch_case(case)
    compare("V=%d B=%d NQ=%d J=%d" % (V, B, NQ, J), case, out, *refs((V, B, NQ, J), C.all_valid(B, NQ)))


@pytest.mark.parametrize("V", C.MEET_ONLY_V)
def test_rays_that_meet_against_fp64(V):
    """255 problems of class `meet` alone at V = 2 and 3, where about 3 % of the last pivots of the first factorisation are rounding
    noise below zero (asserted on the CPU): the fmax(d3, 1e-18 G33) clamp."""
    B, NQ, J = C.RAGGED
    classes = C.meet_only(B, NQ)
    case = C.tri_case(V, B, NQ, J, classes=classes)
    compare("V=%d meet only" % V, case, launch_case(case), *refs((V, B, NQ, J, False, 0, classes), C.all_valid(B, NQ)))


@pytest.mark.parametrize("V", [3, 9])
def test_view_order_regroups_the_sums_only(V):
    """views and their records permuted: ref2d / proj2d move with their views bit for bit, new_ref stays within the bars (not bitwise:
    the partial Gram matrices of the 8 lanes regroup)."""
    B, NQ, J = 2, 5, 15
    case = C.tri_case(V, B, NQ, J)
    Lq = NQ * J
    perm = torch.randperm(V, generator=torch.Generator().manual_seed(V))
    assert not torch.equal(perm, torch.arange(V))
    pc = dict(case, r=case["r"].view(V, B, Lq, 2)[perm].reshape(V * B, Lq, 2), o=case["o"].view(V, B, Lq, 3)[perm].reshape(V * B, Lq, 3),
              rec=case["rec"].view(V, B, 48)[perm].reshape(V * B, 48))
    a, b = launch_case(case), launch_case(pc)
    assert same_bits(b["ref2d"], a["ref2d"][:, perm]) and same_bits(b["proj2d"], a["proj2d"][:, perm])
    ref64, ref32 = refs((V, B, NQ, J), C.all_valid(B, NQ))
    pick = lambda t: (t[0], t[1][:, perm], t[2][:, perm], t[3])
    compare("V=%d permuted views" % V, case, b, pick(ref64), pick(ref32))
    print("V=%d permuted views: %d of %d new_ref values keep their bits" % (V, int((bits(a["new_ref"]) == bits(b["new_ref"])).sum()), B * Lq * 3))


# --------------------------------------------------------------------------------------------------------------- masking
@pytest.fixture(scope="module")
def mask_case():
    V, B, NQ, J = 3, 2, 9, 15
    case = C.tri_case(V, B, NQ, J, rotated=True)
    return case, launch_case(case)


@pytest.mark.parametrize("any_valid", [0, 1])
@pytest.mark.parametrize("kind", ["mixed", "none", "last"])
def test_masking_and_any_valid(mask_case, kind, any_valid):
    """V = 3, B = 2, 270 problems, strong distortion and a rotated inverse crop affine: zeros for the queries that are not computed,
    query (0, 0) computed exactly when any_valid = 0, the computed problems within the bars of fp64 and bit for bit what they are
    with every query valid."""
    case, full = mask_case
    V, B, NQ, J = 3, 2, 9, 15
    valid = _valid(kind, B, NQ, torch.Generator().manual_seed(5))
    out = launch_case(case, valid, any_valid)
    ref64, ref32 = refs((V, B, NQ, J, True), valid, any_valid)
    tok = ref64[3]["computed"]
    want = valid.bool().clone()
    if any_valid == 0:
        want[0, 0] = True
    assert torch.equal(tok, want.repeat_interleave(J, 1))
    assert int(tok.sum()) == {("none", 0): J, ("none", 1): 0, ("last", 0): 2 * J, ("last", 1): J}.get((kind, any_valid), int(valid.sum()) * J)
    assert torch.equal(out["proj2d"].abs().sum((1, 3)) != 0, tok) and torch.equal(out["ref2d"].abs().sum((1, 3)) != 0, tok)
    compare("mask %s any_valid=%d" % (kind, any_valid), case, out, ref64, ref32)
    m4 = tok[:, None].expand(B, V, NQ * J)
    assert same_bits(out["new_ref"][tok], full["new_ref"][tok]) and same_bits(out["ref2d"][m4], full["ref2d"][m4])
    assert same_bits(out["proj2d"][m4], full["proj2d"][m4])


# ------------------------------------------------------------------------------------------------- views of zero weight
@pytest.mark.parametrize("V", [9, 32])
def test_views_of_zero_weight_add_exact_zeros(V):
    """views 8 ... V - 1 with a logit of -1e4 (weight exactly 0) against the launch of the first 8 views alone: new_ref bit for bit, and
    the first 8 views of ref2d / proj2d: the second to fourth trip of the view loops adds exact zeros to the softmax denominator and to
    the Gram matrix, and reads the right views doing so (their ref2d is compared with fp64)."""
    B, NQ, J = 2, 5, 15
    Lq = NQ * J
    case = C.tri_case(V, B, NQ, J, classes=C.query_classes(B, NQ, ("noise2", "off30", "meet")))
    o = case["o"].clone().view(V, B, Lq, 3)
    o[8:, :, :, 2] = -1e4
    big = launch(case["r"], o.view(V * B, Lq, 3), case["rec"], C.all_valid(B, NQ), 1, V, B, NQ, J)
    small = launch(case["r"].view(V, B, Lq, 2)[:8].reshape(8 * B, Lq, 2), o[:8].reshape(8 * B, Lq, 3), case["rec"].view(V, B, 48)[:8].reshape(8 * B, 48),
                   C.all_valid(B, NQ), 1, 8, B, NQ, J)
    assert bool(torch.isfinite(big["new_ref"]).all())
    assert same_bits(big["new_ref"], small["new_ref"])
    assert same_bits(big["ref2d"][:, :8], small["ref2d"]) and same_bits(big["proj2d"][:, :8], small["proj2d"])
    x64, r64, p64, _ = T.triangulate(case["r"], o.view(V * B, Lq, 3), case["rec"], C.all_valid(B, NQ), 1, V, B, NQ, J)
    x32, r32, p32, _ = T.triangulate(case["r"], o.view(V * B, Lq, 3), case["rec"], C.all_valid(B, NQ), 1, V, B, NQ, J, dtype=F32)
    check("V=%d zero-weight views ref2d" % V, big["ref2d"], r64, bar32(r64, r32))
    check("V=%d zero-weight views proj2d" % V, big["proj2d"], p64, bar32(p64, p32))


# --------------------------------------------------------------------------------------------------------- tails and batch
@pytest.mark.parametrize("V", [3, 9])
@pytest.mark.parametrize("B,NQ,J", C.SHAPES, ids=lambda v: str(v))
def test_tails_and_batch_elements(V, B, NQ, J):
    """1, 63, 64, 65, 129, 90 and 255 problems at B = 1, 2, 3: element b of a batch gives the bits it gives alone (its problems then sit
    in other workgroups and lanes, next to other neighbours), and two runs give the same bits."""
    case = C.tri_case(V, B, NQ, J)
    Lq = NQ * J
    a, again = launch_case(case), launch_case(case)
    for k in ("new_ref", "ref2d", "proj2d"):
        assert same_bits(a[k], again[k]), k
    for b in range(B):
        one = launch(case["r"].view(V, B, Lq, 2)[:, b].contiguous(), case["o"].view(V, B, Lq, 3)[:, b].contiguous(),
                     case["rec"].view(V, B, 48)[:, b].contiguous(), C.all_valid(1, NQ), 1, V, 1, NQ, J)
        for k in ("new_ref", "ref2d", "proj2d"):
            assert same_bits(one[k][0], a[k][b]), (k, b)


# ------------------------------------------------------------------------------------------------------------ degenerate
def _with_degenerate(B, NQ):
    base = C.query_classes(B, NQ, ("noise2", "meet", "off300"))
    deg = [list(row) for row in base]
    for b in range(B):
        for i in range(1 + b, NQ, 4):
            base[b][i], deg[b][i] = "noise2", "degenerate"
    return base, deg


@pytest.mark.parametrize("V", [2, 9])
def test_degenerate_problems_are_contained(V):
    """every fourth query holds one-view problems (one logit 0, the others -60): the inverse iteration declines them and the Jacobi
    takes over.  Nothing is promised about their values; the launch returns 0 inside its buffers, and every other problem of the
    launch keeps, bit for bit, what it gives when noise2 problems sit in the same slots.  (What comes back: DESIGN.md section 9s.)"""
    B, NQ, J = 2, 9, 15
    base, deg = _with_degenerate(B, NQ)
    ca, cd = C.tri_case(V, B, NQ, J, classes=base), C.tri_case(V, B, NQ, J, classes=deg)
    a, d = launch_case(ca), launch_case(cd)
    isd = torch.tensor([[c == "degenerate" for c in row] for row in cd["cls"]])
    assert 0 < int(isd.sum()) < isd.numel() and same_bits(cd["r"], ca["r"])
    assert same_bits(d["new_ref"][~isd], a["new_ref"][~isd])
    x = d["new_ref"][isd]
    fin = torch.isfinite(x)
    print("V=%d one-view problems: %d of %d values finite, largest finite %.3e mm" % (V, int(fin.sum()), x.numel(),
                                                                                      float(x[fin].abs().max()) if fin.any() else 0.0))
    compare("V=%d next to one-view problems" % V, cd, d, *refs((V, B, NQ, J, False, 0, deg), C.all_valid(B, NQ)))


def test_single_view_is_rank_deficient_but_contained():
    """V = 1: two rows for four unknowns, every problem degenerate; ref2d and proj2d are still held to fp64."""
    V, B, NQ, J = (1,) + C.RAGGED
    case = C.tri_case(V, B, NQ, J)
    out = launch_case(case)
    x64, r64, p64, _ = T.triangulate(case["r"], case["o"], case["rec"], C.all_valid(B, NQ), 1, V, B, NQ, J)
    _, r32, p32, _ = T.triangulate(case["r"], case["o"], case["rec"], C.all_valid(B, NQ), 1, V, B, NQ, J, dtype=F32)
    check("V=1 ref2d", out["ref2d"], r64, bar32(r64, r32))
    check("V=1 proj2d", out["proj2d"], p64, bar32(p64, p32))
    x = out["new_ref"]
    fin = torch.isfinite(x)
    print("V=1: %d of %d values finite, largest finite %.3e mm" % (int(fin.sum()), x.numel(), float(x[fin].abs().max()) if fin.any() else 0.0))
    again = launch_case(case)
    assert same_bits(again["new_ref"], x)


# ------------------------------------------------------------------------------------------------------ non-finite input
def test_non_finite_inputs_stay_in_their_problem():
    """V = 9, B = 2, 270 problems: a NaN in dx of view 8 (second trip of the view loop) of one problem, a NaN logit in another, r = +Inf in
    a third.  The three problems come back non-finite; every other problem keeps its bits; ref2d / proj2d are non-finite exactly where
    the statement's are (the affected view; a logit touches neither) and keep their bits everywhere else."""
    V, B, NQ, J = 9, 2, 9, 15
    Lq = NQ * J
    case = C.tri_case(V, B, NQ, J)
    clean = launch_case(case)
    r, o = case["r"].clone().view(V, B, Lq, 2), case["o"].clone().view(V, B, Lq, 3)
    hit = [(0, 7), (1, 70), (1, Lq - 1)]
    o[8, 0, 7, 0] = float("nan")
    o[1, 1, 70, 2] = float("nan")
    r[0, 1, Lq - 1, 1] = float("inf")
    out = launch(r.view(V * B, Lq, 2), o.view(V * B, Lq, 3), case["rec"], C.all_valid(B, NQ), 1, V, B, NQ, J)
    _, r64, p64, _ = T.triangulate(r.view(V * B, Lq, 2), o.view(V * B, Lq, 3), case["rec"], C.all_valid(B, NQ), 1, V, B, NQ, J)
    other = torch.ones(B, Lq, dtype=torch.bool)
    for b, q in hit:
        other[b, q] = False
        print("non-finite input -> new_ref", out["new_ref"][b, q].tolist())
        assert not bool(torch.isfinite(out["new_ref"][b, q]).any())
    assert same_bits(out["new_ref"][other], clean["new_ref"][other]) and bool(torch.isfinite(out["new_ref"][other]).all())
    for got, ref, cl in ((out["ref2d"], r64, clean["ref2d"]), (out["proj2d"], p64, clean["proj2d"])):
        bad = ~torch.isfinite(got)
        assert torch.equal(bad, ~torch.isfinite(ref))
        assert same_bits(got[~bad], cl[~bad])
        assert torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.equal(got[bad & ~torch.isnan(got)].double(), ref[bad & ~torch.isnan(ref)])
    bad = ~torch.isfinite(out["ref2d"]).all(-1)
    want = torch.zeros(B, V, Lq, dtype=torch.bool)
    want[0, 8, 7] = want[1, 0, Lq - 1] = True
    assert torch.equal(bad, want)


# ------------------------------------------------------------------------------------------------------ fused projection
@pytest.mark.parametrize("V", [3, 9])
@pytest.mark.parametrize("L", [1, 4])
def test_fused_projection_equals_project_of_the_new_points(V, L):
    """mvg_triangulate_project on level tables other than the workload's (one level; four non-square levels), B = 2, 150 problems, mixed
    validity, one-view problems in the launch: new_ref / ref2d / proj2d are mvg_triangulate's bits, and (r_next, ref_lvl_next,
    inside_next) are, as integers, what mvg_project gives on that new_ref -- for the masked problems the projection of the origin."""
    Lm = _lib()
    B, NQ, J = 2, 5, 15
    Lq = NQ * J
    _, deg = _with_degenerate(B, NQ)
    case = C.tri_case(V, B, NQ, J, classes=deg)
    valid = _valid("mixed", B, NQ, torch.Generator().manual_seed(3))
    valid[0, 1], valid[1, 2] = 1, 1                                             # two of the one-view queries are computed
    assert deg[0][1] == "degenerate" and deg[1][2] == "degenerate" and 0 < int(valid.sum()) < B * NQ
    plain = launch_case(case, valid, 1)
    fused = launch_case(case, valid, 1, shapes=PROJ_SHAPES[L])
    for k in ("new_ref", "ref2d", "proj2d"):
        assert same_bits(plain[k], fused[k]), k
    n = V * B * Lq
    outs = dict(r=Out(n * 2), lv=Out(n * L * 2), ins=Out(n, torch.uint8))
    recd = case["rec"].to(DEV)
    Lm.check(Lm.load().mvg_project(Lm.ptr(fused["new_ref_dev"]), Lm.ptr(recd), _i64(PROJ_SHAPES[L]), L, Lm.ptr(outs["r"].mid),
                                   Lm.ptr(outs["lv"].mid), Lm.ptr(outs["ins"].mid), V, B, Lq, Lm.stream_ptr()), "mvg_project")
    torch.cuda.synchronize()
    assert all(ob.guards_ok() and ob.all_written() for ob in outs.values())
    assert torch.equal(bits(fused["r_next"]).flatten(), bits(outs["r"].mid.cpu()))
    assert torch.equal(bits(fused["ref_lvl_next"]).flatten(), bits(outs["lv"].mid.cpu()))
    assert torch.equal(fused["inside_next"].flatten(), outs["ins"].mid.cpu())
    # masked problems: new_ref = 0, so every masked problem of an image projects to the same pixel, the origin's, which geom_ref gives
    tok = T.computed_mask(valid, 1, J)
    assert bool((fused["new_ref"][~tok] == 0).all())
    r0 = R.project(torch.zeros(B, 1, 3), case["rec"], PROJ_SHAPES[L])
    r032 = R.project(torch.zeros(B, 1, 3), case["rec"], PROJ_SHAPES[L], dtype=F32)
    m = (~tok)[torch.arange(V * B) % B]                                          # (V * B, Lq)
    got = fused["r_next"][m].view(-1, 2)
    check("fused projection L=%d V=%d: origin of the masked problems" % (L, V), got, r0[0].expand(V * B, Lq, 2)[m], bar32(r0[0], r032[0]).max())
    print("fused projection L=%d V=%d: %d of %d new_ref values non-finite" % (L, V, int((~torch.isfinite(fused["new_ref"])).sum()), B * Lq * 3))


# -------------------------------------------------------------------------------------------------------------- arguments
def test_arguments_are_checked_before_anything_is_written():
    V, B, NQ, J = 3, 2, 3, 2
    case = C.tri_case(V, B, NQ, J)
    a = (case["r"], case["o"], case["rec"], C.all_valid(B, NQ), 1)
    for name in ("r", "o", "cams", "valid", "any_valid", "new_ref", "ref2d", "proj2d"):
        launch(*a, V, B, NQ, J, null=(name,), expect=BADARG)
        launch(*a, V, B, NQ, J, shapes=PROJ_SHAPES[4], null=(name,), expect=BADARG)
    for name in ("shapes_host", "r_next", "ref_lvl_next", "inside_next"):
        launch(*a, V, B, NQ, J, shapes=PROJ_SHAPES[4], null=(name,), expect=BADARG)
    launch(*a, 0, B, NQ, J, expect=BADARG)
    launch(*a, 0, B, NQ, J, shapes=PROJ_SHAPES[1], expect=BADARG)
    # no problems: success, nothing written (launch() asserts that no element of any buffer changed)
    for shape in ((0, NQ, J), (B, 0, J), (B, NQ, 0)):
        launch(*a, V, *shape, expect=0)
        launch(*a, V, *shape, shapes=PROJ_SHAPES[1], expect=0)
