"""The sampling kernels -- the deterministic backward chain of csrc/msda_bwd.hip (bw_absmax, bw_part, bw_prefix, bw_scan, bw_reduce, bw_shared),
the fp32-atomic and fp64 backward and the forward kernels of csrc/msda.hip -- against the fp64 statement of tests/msda_ref.py (pinned to the
oracle by tests/test_msda_ref_oracle.py), on the cases of tests/msda_cases.py: small shapes that reach every branch of the chain.

Error bars (no fixed figure): an output element's bar is k * 2^-24 * A + 2 ulp of the value, A being the sum of the absolute values of the
element's terms and k 4 x the largest |ref32 - ref64| / (2^-24 A) over the case, ref32 the reference evaluated in fp32 on the CPU -- it
measures the reference, never the kernel.  The deterministic grad_value adds the rounding its kernel documents, cnt * 2^-31 * bound_n
(cnt contributions to the pixel, bound_n = max |grad_output[n]| * max |attn_weight[n]| over the finite entries).  fp64 outputs: 2^-53 for
2^-24.  Every assertion prints max err / bar.  The backward kernels are called through the C ABI on outputs pre-filled with NaN between
sentinel guards (grad_value of the atomic kernels: zeros, their contract): every element must come back finite and the guards untouched.
The fixed-point term is tight by construction: a pixel that receives one small contribution carries exactly the half-unit rounding of
that contribution, 2^-31 bound_n, and the kernel reaches it (max err / bar 0.999 on many_bins, fp32 and bf16 value): a 0.999 there is the
documented rounding, not a kernel close to failing, and a figure above 1 means more than half a unit per contribution.
Samples whose cell depends on whether ly * H - 0.5 is fused (tests/msda_ref.ambiguous; none in these seeds) are left out of the grad_loc
comparison only."""
import ctypes as C

import pytest
import torch

from tests import msda_cases as MC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 1024
SENT_F = -7.25e5
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
KINDS = ("det_f32", "det_bf16", "atomic_f32", "f64")
GRADS = ("grad_value", "grad_loc", "grad_attn")


def _lib():
    from mvgformer_amd import _lib as L
    return L


def _i64(t):
    flat = [int(x) for x in t.flatten().tolist()]
    return (C.c_int64 * len(flat))(*flat)


def _guarded(shape, dtype, fill):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), SENT_F, dtype=dtype, device=DEV)
    buf[GUARD:GUARD + n] = fill
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guard_ok(buf):
    return bool((buf[:GUARD] == SENT_F).all()) and bool((buf[-GUARD:] == SENT_F).all())


def _check(name, got, ref, bar, keep=None):
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all()), name + ": an element was not written, or is not finite"
    err = (got - ref).abs()
    if keep is not None:
        err = err * keep
    ratio = float((err / bar.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print("%s: max err %.3e, max err / bar %.3f" % (name, float(err.max()) if err.numel() else 0.0, ratio))
    assert bool((err <= bar).all()), (name, ratio)
    return ratio


def _backward(kind, c, go=None, ws_byte=0xA5, value=None):
    """one launch of a backward entry point on guarded outputs -> (grad_value, grad_loc, grad_attn) on the device."""
    Lm = _lib()
    lib = Lm.load()
    value = c["value"] if value is None else value
    go = c["go"] if go is None else go
    N, S, M, D = value.shape
    _, Lq, _, L, P, _ = c["loc"].shape
    ft = F64 if kind == "f64" else F32
    v = value.to(DEV, BF16 if kind == "det_bf16" else ft).contiguous()
    loc, wgt, god = (t.to(DEV, ft).contiguous() for t in (c["loc"], c["weight"], go))
    assert wgt.data_ptr() % 16 == 0 and god.data_ptr() % 16 == 0           # the lead / tail figures of msda_cases.properties assume it
    det = kind.startswith("det")
    gvb, gv = _guarded((N, S, M, D), ft, float("nan") if det else 0.0)
    glb, gl = _guarded((N, Lq, M, L, P, 2), ft, float("nan"))
    gab, ga = _guarded((N, Lq, M, L, P), ft, float("nan"))
    dims = (N, S, M, D, L, Lq, P)
    if det:
        shapes_c, starts_c = _i64(c["shapes"]), _i64(c["starts"])
        nbytes = int(lib.mvg_msda_backward_det_workspace(N, S, M, D, L, Lq, P, shapes_c))
        assert nbytes > 0 and nbytes % 256 == 0
        wsb = torch.full((nbytes + 2 * GUARD,), 0x3C, dtype=torch.uint8, device=DEV)
        ws = wsb[GUARD:GUARD + nbytes]
        ws.fill_(ws_byte)
        fn = lib.mvg_msda_backward_det_f32 if kind == "det_f32" else lib.mvg_msda_backward_det_bf16
        rc = fn(Lm.ptr(v), shapes_c, starts_c, Lm.ptr(loc), Lm.ptr(wgt), Lm.ptr(god), Lm.ptr(gv), Lm.ptr(gl), Lm.ptr(ga), *dims,
                Lm.ptr(ws), nbytes, Lm.stream_ptr())
        torch.cuda.synchronize()
        assert bool((wsb[:GUARD] == 0x3C).all()) and bool((wsb[-GUARD:] == 0x3C).all())
    else:
        shapes_d, starts_d = c["shapes"].to(DEV), c["starts"].to(DEV)
        fn = lib.mvg_msda_backward_f64 if kind == "f64" else lib.mvg_msda_backward_f32
        rc = fn(Lm.ptr(v), Lm.ptr(shapes_d), Lm.ptr(starts_d), Lm.ptr(loc), Lm.ptr(wgt), Lm.ptr(god), Lm.ptr(gv), Lm.ptr(gl), Lm.ptr(ga),
                *dims, Lm.stream_ptr())
        torch.cuda.synchronize()
    assert rc == 0, rc
    assert _guard_ok(gvb) and _guard_ok(glb) and _guard_ok(gab)
    return gv.clone(), gl.clone(), ga.clone()


def _bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int64)


def _same_bits(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------- backward against the fp64 statement
BACKWARD = [(n, k) for n in MC.DET_CASES for k in KINDS] + [(n, k) for n in MC.ATOMIC_ONLY_CASES for k in ("atomic_f32", "f64")]


@pytest.mark.parametrize("name,kind", BACKWARD, ids=["%s-%s" % nk for nk in BACKWARD])
def test_backward_against_fp64(name, kind):
    """every case of tests/msda_cases.py on every backward kernel that takes its shape: all three gradients within their per-element bars,
    every element written and finite.  det_bf16: the value is rounded to bf16 first and the reference is evaluated on the rounded value.
    nonfinite_go runs on its cleaned grad_output here (its contract is the test below)."""
    c = MC.case(name)
    mode = "bf16" if kind == "det_bf16" else "f64" if kind == "f64" else "f32"
    ref, k = MC.reference(name, mode)
    go = c.get("go_clean", c["go"])
    print("%s %s: k %s" % (name, kind, "  ".join("%s %.2f" % (g, k[g]) for g in GRADS)))
    got = _backward(kind, c, go)
    eps = 2.0 ** -53 if kind == "f64" else 2.0 ** -24
    fx = MC.bound_per_image(go, c["weight"]) if kind.startswith("det") else None
    keep = (~ref["ambiguous"]).double().unsqueeze(-1)
    for g, x in zip(GRADS, got):
        _check("%s %s %s" % (name, kind, g), x, ref[g], MC.bar(ref, k, g, eps, fx if g == "grad_value" else None), keep if g == "grad_loc" else None)
    if name == "range_zero" and kind.startswith("det"):        # scale 0: exact zeros, not NaN (0 * inf) and not 1 / 0
        assert bool((got[0][0] == 0).all())


# ----------------------------------------------------------------------------------------- properties of the deterministic form, bitwise
@pytest.mark.parametrize("kind", ["det_f32", "det_bf16"])
@pytest.mark.parametrize("name", ["one_bin", "many_bins_b", "coincident_corner", "range"])
def test_deterministic_backward_repeats_itself_and_ignores_what_the_workspace_held(name, kind):
    """two runs give the same bits, and a workspace pre-filled with 0x00 gives the same bits as one pre-filled with 0xA5 / 0xFF: every word
    of the workspace is written by the chain before it is read (accum: bw_shared<0> zeroes exactly the shared pixels that bw_reduce adds to
    and bw_shared<1> reads; gmax: reset by bw_shared<0>; cnt: every (part, bin) by bw_part<0>; total, offset: every bin by bw_prefix /
    bw_scan; list: every position of a non-empty bin by bw_part<1>)."""
    c = MC.case(name)
    a = _backward(kind, c, ws_byte=0xA5)
    assert _same_bits(a, _backward(kind, c, ws_byte=0xA5))
    assert _same_bits(a, _backward(kind, c, ws_byte=0x00))
    assert _same_bits(a, _backward(kind, c, ws_byte=0xFF))


def test_deterministic_backward_of_an_image_does_not_depend_on_its_batch():
    """image n of `range` alone (N = 1) gives the bits it gives inside the batch of three: the scale is per image (1, 1e6 and 1e-30 here)
    and nothing of the chain crosses an image."""
    c = MC.case("range")
    full = _backward("det_f32", c)
    for n in range(3):
        one = {k: (v[n:n + 1].contiguous() if k in ("value", "loc", "weight", "go") else v) for k, v in c.items()}
        alone = _backward("det_f32", one)
        assert _same_bits([t[n:n + 1] for t in full], alone), n


@pytest.mark.parametrize("name", ["range", "many_bins_b", "one_bin"])
def test_deterministic_backward_is_equivariant_to_a_permutation_of_the_queries(name):
    """queries permuted: grad_value keeps its bits (integer sums), grad_loc and grad_attn are permuted (one writer per sample, a fixed
    reduction order over the channels)."""
    c = MC.case(name)
    Lq = c["loc"].shape[1]
    perm = torch.randperm(Lq, generator=torch.Generator().manual_seed(3))
    p = dict(c, loc=c["loc"][:, perm].contiguous(), weight=c["weight"][:, perm].contiguous(), go=c["go"][:, perm].contiguous())
    gv, gl, ga = _backward("det_f32", c)
    pv, pl, pa = _backward("det_f32", p)
    perm = perm.to(DEV)
    assert _same_bits((gv, gl[:, perm], ga[:, perm]), (pv, pl, pa))


# -------------------------------------------------------------------------------------------------- non-finite grad_output: the contract
@pytest.mark.parametrize("kind", ["det_f32", "det_bf16"])
def test_non_finite_grad_output_does_not_enter_grad_value(kind):
    """ops.msda_backward: "Non-finite grad_output entries do not enter grad_value".  NaN, +Inf and -Inf entries, one of them on a sample at a
    texel centre (three corner weights are zero: Inf * 0) and on generic samples (Inf * w): grad_value has the bits of the run with those
    entries replaced by 0, so have grad_loc / grad_attn of every other (query, head) row; the affected rows are non-finite or zero, as the
    atomic kernel leaves them."""
    c = MC.case("nonfinite_go")
    clean = _backward(kind, c, c["go_clean"])
    dirty = _backward(kind, c, c["go"])
    rows = c["bad_rows"].to(DEV)
    bad_v = int((_bits(dirty[0]) != _bits(clean[0])).sum())
    print("%s: %d elements of grad_value differ from the run on the cleaned grad_output, %d are not finite"
          % (kind, bad_v, int((~torch.isfinite(dirty[0])).sum())))
    assert bad_v == 0
    for d, cl in zip(dirty[1:], clean[1:]):
        assert torch.equal(_bits(d)[~rows], _bits(cl)[~rows])
        assert bool((~torch.isfinite(d[rows]) | (d[rows] == 0)).all())
    atomic = _backward("atomic_f32", c, c["go"])
    for d in atomic[1:]:
        assert bool((~torch.isfinite(d[rows]) | (d[rows] == 0)).all())


# ------------------------------------------------------------------------------------------------------------------- forward, same cases
@pytest.mark.parametrize("dtype", [F32, BF16, F64], ids=["f32", "bf16", "f64"])
@pytest.mark.parametrize("name", list(MC.CASES))
def test_forward_against_fp64(name, dtype):
    """ops.msda_forward in fp32, bf16 and fp64 under all three work mappings (fwd_map 0, 1, 2) against the reference's forward; bf16: the
    reference on the rounded value, and half a bf16 ulp of the output on top of the bar."""
    from mvgformer_amd import ops
    c = MC.case(name)
    ref, k = MC.reference(name, "bf16" if dtype == BF16 else "f64" if dtype == F64 else "f32")
    eps = 2.0 ** -53 if dtype == F64 else 2.0 ** -24
    bar = MC.bar(ref, k, "out", eps)
    if dtype == BF16:
        bar = bar + 2.0 ** -8 * ref["out"].abs()
    lt = F64 if dtype == F64 else F32
    args = (c["value"].to(DEV, dtype), c["shapes"].to(DEV), c["starts"].to(DEV), c["loc"].to(DEV, lt), c["weight"].to(DEV, lt))
    for fwd_map in (0, 1, 2):
        with _lib().tuning(fwd_map=fwd_map):
            y = ops.msda_forward(*args)
            assert y.dtype == dtype
            _check("%s forward %s fwd_map=%d (k %.2f)" % (name, str(dtype).split(".")[1], fwd_map, k["out"]), y, ref["out"], bar)
