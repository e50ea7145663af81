"""The fused sampling kernels of the decoder -- msda_gsamp_kernel / msda_gsamp_pipe_kernel (bf16), msda_gfused_f32_hp_kernel (fp32) and
msda_fused_kernel<float> / <bf16, 8> (csrc/msda.hip, csrc/gsamp_dev.h) -- against the fp64 statement of tests/gsamp_ref.py (pinned to the
oracle by tests/test_gsamp_ref_cpu.py) on the cases of tests/gsamp_cases.py: small inputs that reach the kernels' edge branches.

Error bars (no figure is taken from a kernel's output): fp32 kernels k * 2^-24 * out_A + 2 ulp of the value, out_A the error scale the
reference carries through the footprint, the softmax and the sampling, k 4 x the largest |ref32 - ref64| / (2^-24 out_A) over the case,
ref32 the statement evaluated in fp32 on the CPU.  bf16 G-sampling: the reference on the bf16 operands as stored, plus what the kernel
documents -- blend weights rounded to bf16 (2^-8 x the sum of the absolute values of the output's terms) and the output rounded to bf16
(2^-8 |out|).  msda_fused<bf16>: the output rounding only.  Outputs are pre-filled with NaN between sentinel guards: every element must
come back finite (a masked pair's row exactly zero) and inside its bar -- none is left out --, the guards untouched.  Every assertion
prints max err / bar."""
import pytest
import torch

from tests import gsamp_cases as GC
from tests import gsamp_ref as GR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 1024
SENT = -65536.0
F32, BF16 = torch.float32, torch.bfloat16
KERNELS = ("gsamp_bf16", "gfused_f32", "fused_f32", "fused_bf16")
def _lm():
    from mvgformer_amd import _lib as L
    return L


def _guarded(rows, dtype):
    buf = torch.full((rows * 256 + 2 * GUARD,), SENT, dtype=dtype, device=DEV)
    buf[GUARD:GUARD + rows * 256] = float("nan")
    return buf, buf[GUARD:GUARD + rows * 256].view(rows, 256)


def _guard_ok(buf):
    return bool((buf[:GUARD] == SENT).all()) and bool((buf[-GUARD:] == SENT).all())


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def _run(kernel, c, order="case", pair_mask="case", oa=None):
    """one launch of a kernel on the case's tensors, into a NaN-filled row block between guards -> samp (n_img * Lq, 256) on the device.
    order / pair_mask: "case" = the case's own ("bin": ops.bin_pairs on the case's reference points and mask), else a tensor or None;
    msda_fused takes neither, and oa (pairs * L, 192) instead of G and xw."""
    from mvgformer_amd import ops
    Lm = _lm()
    lib = Lm.load()
    levels = ops.Levels(c["shapes"], c["starts"])
    n_img, Lq, L, _ = c["ref_lvl"].shape
    S = c["value"].shape[1]
    r = c["ref_lvl"].to(DEV).contiguous()
    mask = c["pair_mask"] if isinstance(pair_mask, str) else pair_mask
    mask = None if mask is None else mask.to(DEV).contiguous()
    order = c["order"] if isinstance(order, str) and order == "case" else order
    if isinstance(order, str):
        assert order == "bin"
        order = ops.bin_pairs(r, None if mask is None else mask.view(n_img, Lq), levels)
        assert sorted(order.tolist()) == list(range(n_img * Lq))
    order = None if order is None else order.to(DEV).contiguous()
    if kernel == "gsamp_bf16":
        buf, samp = _guarded(n_img * Lq, BF16)
        ops.msda_gsamp(GC.planes(c["value"]).to(DEV, BF16), c["G"].to(DEV, BF16), c["xw"].to(DEV), r, levels, c["B"], mask, order, out=samp)
    elif kernel == "gfused_f32":
        buf, samp = _guarded(n_img * Lq, F32)
        value, G, xw = c["value"].to(DEV), c["G"].to(DEV), c["xw"].to(DEV)
        Lm.check(lib.mvg_msda_gfused_f32(Lm.ptr(value), Lm.ptr(G), Lm.ptr(xw), Lm.ptr(r), levels.shapes_c, levels.starts_c, Lm.ptr(samp),
                                         Lm.ptr(mask), Lm.ptr(order), n_img, Lq, L, S, c["B"], Lm.stream_ptr()), "mvg_msda_gfused_f32")
    else:
        dt = F32 if kernel == "fused_f32" else BF16
        buf, samp = _guarded(n_img * Lq, dt)
        value, oad = c["value"].to(DEV, dt), oa.to(DEV)
        Lm.check(lib.mvg_msda_fused(Lm.ptr(value), Lm.dtype_code(dt), Lm.ptr(oad), Lm.ptr(r), levels.shapes_c, levels.starts_c, Lm.ptr(samp),
                                    n_img, Lq, L, S, Lm.stream_ptr()), "mvg_msda_fused")
    torch.cuda.synchronize()
    assert _guard_ok(buf), kernel + ": a guard around samp was written"
    return samp.clone()


def _check(label, got, ref, bar):
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all()), label + ": an element was not written, or is not finite"
    err = (got - ref["out"]).abs()
    ratio = float((err / bar.clamp_min(1e-300)).max())
    print("%s: max err %.3e, max err / bar %.3f" % (label, float(err.max()), ratio))
    assert bool((err <= bar).all()), (label, ratio)
    return ratio


def _reference(kernel, name):
    """(ref, k, bar, oa) of a kernel on a case."""
    mode = "bf16" if kernel.endswith("bf16") else "f32"
    if kernel.startswith("fused"):
        oa, ref, k = GC.reference_fused(name, mode)
        return ref, k, GR.bar(ref, k, "fused_bf16" if mode == "bf16" else "f32"), oa
    ref, k = GC.reference(name, mode)
    return ref, k, GR.bar(ref, k, "gsamp_bf16" if mode == "bf16" else "f32"), None


# ------------------------------------------------------------------------------------------------------- against the fp64 statement
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", list(GC.CASES))
def test_forward_against_fp64(name, kernel):
    """every case on every kernel: all elements finite and inside their bars, masked rows exactly zero, nothing written past the rows."""
    c = GC.case(name)
    ref, k, bar, oa = _reference(kernel, name)
    got = _run(kernel, c, oa=oa)
    _check("%s %s (k %.2f)" % (name, kernel, k), got, ref, bar)
    if not kernel.startswith("fused") and c["pair_mask"] is not None:
        assert bool((_bits(got)[c["pair_mask"].to(DEV) == 0] == 0).all())
    if name == "softmax":                                  # every sample of the pair outside the map: +0 everywhere, not exp(..) * 0 of something
        rows = torch.arange(40)[torch.arange(40) % 5 == GC.SOFTMAX_KINDS.index("all_outside")]
        assert bool((got[rows.to(DEV)] == 0).all())


def test_ops_wrappers_run_the_same_kernels():
    """ops.msda_gfused_f32 and ops.msda_fused (which allocate their own output) give the bits of the guarded launches above."""
    from mvgformer_amd import ops
    c = GC.case("levels_3")
    levels = ops.Levels(c["shapes"], c["starts"])
    r = c["ref_lvl"].to(DEV)
    y = ops.msda_gfused_f32(c["value"].to(DEV), c["G"].to(DEV), c["xw"].to(DEV), r, levels, c["B"])
    assert torch.equal(_bits(y), _bits(_run("gfused_f32", c)))
    oa = GC.reference_fused("levels_3")[0]
    for kernel, dt in (("fused_f32", F32), ("fused_bf16", BF16)):
        y = ops.msda_fused(c["value"].to(DEV, dt), oa.to(DEV), r, levels)
        assert y.dtype == dt and torch.equal(_bits(y), _bits(_run(kernel, c, oa=oa)))


# -------------------------------------------------------------------------------------------------------------- variants, bit for bit
GSAMP_VARIANTS = [dict(gsamp_pipe=1), dict(gsamp_pipe=2), dict(auto_small=0)] \
    + [dict(auto_small=0, gsamp_threads=t) for t in (128, 256, 512, 1024)] \
    + [dict(auto_small=0, gsamp_map=m) for m in (0, 1, 4, 8)] \
    + [dict(gsamp_map=m) for m in (0, 8)] \
    + [dict(auto_small=0, gsamp_pipe=1, gsamp_threads=1024, gsamp_map=0)]
GFUSED_VARIANTS = [dict(gfused_chunk=n) for n in (0, 1, 4, 16)]
VARIANT_CASES = ["lattice", "thin", "footprint", "levels_3", "ragged_count_257_none", "ragged_count_257_bin", "ragged_count_257_perm"]


@pytest.mark.parametrize("name", VARIANT_CASES)
def test_variants_are_bit_identical_on_the_edge_cases(name):
    """gsamp_pipe 1 / 2, auto_small 0, gsamp_threads 128 / 256 / 512 / 1024, gsamp_map 0 / 1 / 4 / 8 (msda_gsamp) and gfused_chunk
    0 / 1 / 4 / 16 (msda_gfused_f32): the rows of the default variant, bit for bit, on inputs that reach the edge branches."""
    c = GC.case(name)
    base16, base32 = _bits(_run("gsamp_bf16", c)), _bits(_run("gfused_f32", c))
    for knobs in GSAMP_VARIANTS:
        with _lm().tuning(**knobs):
            assert torch.equal(_bits(_run("gsamp_bf16", c)), base16), knobs
    for knobs in GFUSED_VARIANTS:
        with _lm().tuning(**knobs):
            assert torch.equal(_bits(_run("gfused_f32", c)), base32), knobs


# ------------------------------------------------------------------------------------------------------------------ batch independence
def _subset(c, keep):
    """the case restricted to the queries `keep` (of every image and batch item)."""
    n_img, Lq = c["ref_lvl"].shape[:2]
    sub = dict(c, ref_lvl=c["ref_lvl"][:, keep].contiguous(), xw=c["xw"].view(c["B"], Lq, 192)[:, keep].reshape(-1, 192).contiguous(), order=None)
    if c["pair_mask"] is not None:
        sub["pair_mask"] = c["pair_mask"].view(n_img, Lq)[:, keep].reshape(-1).contiguous()
    return sub


@pytest.mark.parametrize("name", ["levels_3", "batch", "ragged_count_257_none", "lattice"])
def test_a_pair_s_row_does_not_depend_on_the_launch(name):
    """a subset of the queries run alone gives the rows it has in the full run, bit for bit (all four kernels), and the rows do not depend
    on the processing order (None, ops.bin_pairs', a seeded permutation)."""
    c = GC.case(name)
    n_img, Lq = c["ref_lvl"].shape[:2]
    keep = torch.randperm(Lq, generator=torch.Generator().manual_seed(7))[:max(1, Lq // 3)].sort().values
    sub = _subset(c, keep)
    oa = GC.reference_fused(name)[0]
    oa_sub = oa.view(n_img, Lq, -1, 192)[:, keep].reshape(-1, 192).contiguous()
    for kernel in KERNELS:
        fused = kernel.startswith("fused")
        full = _run(kernel, c, order=None, oa=oa if fused else None).view(n_img, Lq, 256)
        part = _run(kernel, sub, oa=oa_sub if fused else None).view(n_img, len(keep), 256)
        assert torch.equal(_bits(full[:, keep.to(DEV)]), _bits(part)), kernel
        if fused:
            continue
        perm = torch.randperm(n_img * Lq, generator=torch.Generator().manual_seed(8)).to(torch.int32)
        for order in ("bin", perm):
            assert torch.equal(_bits(_run(kernel, c, order=order).view(n_img, Lq, 256)), _bits(full)), (kernel, "bin" if isinstance(order, str) else "perm")
