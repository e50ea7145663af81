"""The two bf16 GEMMs through the C ABI against the fp64 statement of their operation (tests/bf16_gemm_ref.py): the pyramid products
mvg_pyramid_group_ws (csrc/wreg_gemm.hip: value head planes and G) and the bf16 paths of mvg_linear / mvg_linear_sum
(csrc/gemm.hip), at the shapes where their code switches paths (tests/bf16_gemm_cases.py, whose coverage, straddler shares and
power against eight emulated defects tests/test_bf16_gemm_ref_cpu.py checks without a GPU).

The only pass condition is err <= bound elementwise.  For an fp32 output the bound is d = LAMBDA lin_err (fp32 accumulation over
K + 1 terms); for a bf16 output the expected value is bf(y) and the bound is ZERO -- bit equality -- except at the straddlers, where
[y - d, y + d] reaches a bf16 rounding boundary and one bf16 step is allowed.  Every output is pre-filled with NaN and sits between
sentinel guard regions; each assertion prints max err / bound, the number of straddlers and how many of them flipped, and the
running figures of its kernel and dtype combination.

Measured on an MI355X, over all cases of this module (for a bf16 output max err / bound can only be 0 or 1 -- the figure that says
something is how many straddlers came out on the other side of their boundary; every other element was bit-equal to bf(y)):
  pyramid planes (bf16)    straddlers 1.26 % of 10.3 M elements, 0.44 % of them flipped (565); the tie case: 71 116 ties, none off
  pyramid G (bf16)         straddlers 1.54 % of 7.5 M elements, 0.42 % of them flipped (486); the tie case: 53 312 ties, none off
  linear bf16 A -> fp32    max err / bound 0.110
  linear fp32 A -> fp32    max err / bound 0.110 (A rounded on load, A + A2 included)
  linear bf16 A -> bf16    straddlers 0.82 % of 1.34 M elements, 0.32 % of them flipped (35)
  linear fp32 A -> bf16    straddlers 0.83 % of 1.34 M elements, 0.33 % of them flipped (37)
A ratio of 0.11 leaves the bound of the fp32 outputs an order of magnitude of room: it does not depend on the k order of a correct
kernel.  Few straddlers flip because the kernels' error is that far inside d.
What the tests found: linear_kernel's ReLU was fmaxf(x, 0), which returns 0 for a NaN, so a NaN row came out of a ReLU GEMM as
zeros (test_linear_non_finite_inputs_stay_in_their_rows failed with ReLU on both tile shapes; one epilogue serves all dtype
combinations, the fp32 forms included); it is the IEEE 754-2019
maximum now, as torch.relu and the kernels of csrc/f32s.hip have it.  The pyramid products passed everything as they were.

bf16 subnormals: how the matrix cores treat subnormal bf16 operands on this part is not established in this repository, so every
operand, product and partial sum of these tests stays in the normal range of bf16 and fp32 (the widest case spreads the rows over
1e-12 .. 1e12); neither flushing nor gradual underflow is asserted."""
import ctypes as C

import pytest
import torch

from tests import bf16_gemm_cases as Cs
from tests import bf16_gemm_ref as B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 1024
SENT = -7.25e5
BADARG = 10001                  # MVG_E_BADARG
BF = torch.bfloat16
_BITS = {torch.bfloat16: torch.int16, torch.float32: torch.int32}


def _lib():
    from mvgformer_amd import _lib as L
    return L


def _sent(dtype):
    return torch.tensor(SENT, dtype=dtype, device=DEV)


def _guarded(n, dtype):
    """(buffer, view of n elements behind a front guard): guards = sentinel, payload = NaN."""
    buf = torch.full((GUARD + n + GUARD,), SENT, dtype=dtype, device=DEV)
    buf[GUARD:GUARD + n] = float("nan")
    return buf, buf[GUARD:GUARD + n]


def _guard_ok(buf, n):
    s = _sent(buf.dtype)
    return bool((buf[:GUARD] == s).all()) and bool((buf[GUARD + n:] == s).all())


def _bits(t):
    return t.contiguous().view(_BITS[t.dtype])


_STATS = {}


def _check(key, name, got, exp, bound):
    """err <= bound elementwise (a NaN -- an element never written -- fails); prints the figures of this call and the running ones
    of `key`."""
    err = (got.double() - exp).abs()
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    n_str, n_flip = int(pos.sum()), int((pos & (err > 0)).sum())
    s = _STATS.setdefault(key, [0.0, 0, 0, 0])
    s[0], s[1], s[2], s[3] = max(s[0], ratio), s[1] + n_str, s[2] + n_flip, s[3] + err.numel()
    bad = int((~(err <= bound)).sum())
    print("%s %s: max err %.3e, max err / bound %.3f, straddlers %d of %d, flipped %d, outside %d  [%s so far: ratio %.3f, "
          "straddlers %d of %d, flipped %d]" % (key, name, float(err.max()) if err.numel() else 0.0, ratio, n_str, err.numel(), n_flip,
                                                bad, key, s[0], s[1], s[3], s[2]))
    assert bad == 0, (key, name, bad)


# ------------------------------------------------------------------------------------------------------------ pyramid products
def _swizzled(W):
    """a plain (256 | 192, 256) bf16 weight on the device in the kernel's fragment order (192 rows: padded with zeros)."""
    from mvgformer_amd import ops
    if W.shape[0] == 192:
        W = torch.cat([W, W.new_zeros(64, 256)], 0)
    return ops.swizzle_weight(W.contiguous())


def _group(feat, n_img, S, jobs, slots=0, expect=0, **raw):
    """one raw launch.  jobs: list of (W plain bf16 on the device, bias | None, planes).  raw: overrides of single arguments for the
    argument checks (njobs, N = {job: value}, no_feat, no_W = job, no_out = job, arg_n_img, arg_S).  Returns the outputs in the
    layouts of the kernel, (n_img, 8, S, 32) and (M, 192); checks the return code and the guards, and, for a refused call, that
    every output is still NaN."""
    L = _lib()
    M = feat.shape[0]
    n = len(jobs)
    keep = [_swizzled(W) for W, _, _ in jobs]
    bufs = [_guarded(M * (256 if planes else 192), BF) for _, _, planes in jobs]
    vp = C.c_void_p * max(n, 9)
    pad = lambda xs: list(xs) + [xs[-1]] * (max(n, 9) - n)
    Wf = vp(*pad([None if raw.get("no_W") == j else w.data_ptr() for j, w in enumerate(keep)]))
    bias = vp(*pad([None if b is None else b.data_ptr() for _, b, _ in jobs]))
    outs = vp(*pad([None if raw.get("no_out") == j else o.data_ptr() for j, (_, o) in enumerate(bufs)]))
    Ns = (C.c_int * max(n, 9))(*pad([raw.get("N", {}).get(j, 256 if planes else 192) for j, (_, _, planes) in enumerate(jobs)]))
    pl = (C.c_int * max(n, 9))(*pad([1 if planes else 0 for _, _, planes in jobs]))
    rc = L.load().mvg_pyramid_group_ws(None if raw.get("no_feat") else L.ptr(feat), raw.get("arg_n_img", n_img), raw.get("arg_S", S),
                                       raw.get("njobs", n), Wf, bias, outs, Ns, pl, int(slots), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, rc
    res = []
    for (buf, out), (_, _, planes) in zip(bufs, jobs):
        assert _guard_ok(buf, out.numel())
        if expect != 0:
            assert bool(torch.isnan(out).all())
        res.append(out.view(n_img, 8, S, 32).clone() if planes else out.view(M, 192).clone())
    return res


_JOBS = {}


def _job(j):
    if j not in _JOBS:
        W, b, planes = Cs.pyr_job(j)
        _JOBS[j] = (W.to(DEV), None if b is None else b.to(DEV), planes)
    return _JOBS[j]


def _rows(out, planes):
    return B.from_planes(out) if planes else out


def _check_job(name, feat, job, out):
    W, b, planes = job
    exp, bound = B.expected(feat, W, b)
    got = _rows(out, planes)
    assert bool(torch.isfinite(got).all()), name
    _check("pyramid planes" if planes else "pyramid G", name, got, exp, bound)


@pytest.mark.parametrize("c", Cs.PYR_CASES, ids=Cs.pyr_id)
def test_pyramid_products_against_fp64(c):
    """every case of the list -- workgroups with 0, 1, 2, 3 and >= 4 tiles per job kind, ragged last tiles of 1 and 31 rows, images of
    1 to 1237 pixels -- with jobs alternating value (bias, head planes) and G (192 columns, no bias): every output finite, within
    the bound of the fp64 statement element by element, guards intact."""
    n_img, S, jobs, slots = c
    feat = Cs.pyr_case_feat(c).to(DEV)
    outs = _group(feat, n_img, S, [_job(j) for j in range(jobs)], slots)
    for j, out in enumerate(outs):
        _check_job("%s job %d" % (Cs.pyr_id(c), j), feat, _job(j), out)


@pytest.mark.parametrize("n_img,S", [(3, 277), (109, 5), (3, 1237)])
def test_pyramid_products_do_not_depend_on_the_split(n_img, S):
    """bit-identical outputs for slots 0, 1, 2, 32, 64 and for the wreg_grid knob 64, 256, 512: a product's bytes depend neither on
    how many workgroups share its tiles nor on which ring slot a tile lands in."""
    L = _lib()
    feat = Cs.pyr_feat(n_img * S, 5).to(DEV)
    jobs = [_job(j) for j in range(4)]
    base = _group(feat, n_img, S, jobs, 0)
    for j, out in enumerate(base):
        _check_job("split base %dx%d job %d" % (n_img, S, j), feat, jobs[j], out)
    for slots in (1, 2, 32, 64):
        for a, b in zip(base, _group(feat, n_img, S, jobs, slots)):
            assert torch.equal(_bits(a), _bits(b)), slots
    for grid in (64, 256, 512):
        with L.tuning(wreg_grid=grid):
            for a, b in zip(base, _group(feat, n_img, S, jobs, 0)):
                assert torch.equal(_bits(a), _bits(b)), grid


@pytest.mark.parametrize("n_img,S", [(3, 277), (51, 5)])
def test_pyramid_row_and_pixel_permutations(n_img, S):
    """any permutation of the rows of feat permutes the rows of G bit for bit; a permutation of the pixels within every image
    permutes that image's planes (and G) bit for bit."""
    M = n_img * S
    gen = torch.Generator().manual_seed(S)
    feat = Cs.pyr_feat(M, 6).to(DEV)
    jobs = [_job(0), _job(1)]
    vh, G = _group(feat, n_img, S, jobs)
    perm = torch.randperm(M, generator=gen).to(DEV)
    _, G2 = _group(feat[perm].contiguous(), n_img, S, jobs)
    assert torch.equal(_bits(G2), _bits(G[perm]))
    pix = torch.stack([torch.randperm(S, generator=gen) for _ in range(n_img)]).to(DEV)                  # (n_img, S)
    rows = (torch.arange(n_img, device=DEV)[:, None] * S + pix).reshape(-1)
    vh3, G3 = _group(feat[rows].contiguous(), n_img, S, jobs)
    assert torch.equal(_bits(G3), _bits(G[rows]))
    want = torch.gather(vh, 2, pix[:, None, :, None].expand(n_img, 8, S, 32))
    assert torch.equal(_bits(vh3), _bits(want))


@pytest.mark.parametrize("kind", ["rows_24_decades", "zero_rows", "zero_weight", "ties"])
def test_pyramid_operand_edges(kind):
    """289 rows (17 images of 17 pixels): rows spread over 24 decades inside the normal range; zero rows give exactly bf(bias) in the
    planes and +0 in G; a zero weight gives the bias; small-integer operands whose exact results sit on bf16 ties come out
    rounded to nearest EVEN, bit for bit (the accumulation is exact there, so no straddler allowance applies)."""
    n_img, S = 17, 17
    M = n_img * S
    Wv, bv, _ = _job(0)
    Wg = _job(1)[0]
    if kind == "ties":
        feat, Wv, bv, Wg = (t.to(DEV) for t in Cs.tie_case(M))
    else:
        feat = Cs.pyr_edge_rows("randn" if kind == "zero_weight" else kind, M).to(DEV)
    if kind == "zero_weight":
        Wv, Wg = torch.zeros_like(Wv), torch.zeros_like(Wg)
    jobs = [(Wv, bv, True), (Wg, None, False)]
    vh, G = _group(feat, n_img, S, jobs)
    _check_job(kind + " planes", feat, jobs[0], vh)
    _check_job(kind + " G", feat, jobs[1], G)
    v = B.from_planes(vh)
    bias16 = bv.to(BF).view(1, 256)
    if kind == "zero_rows":
        assert torch.equal(_bits(v[::3]), _bits(bias16.expand(v[::3].shape[0], 256)))
        assert bool((_bits(G[::3]) == 0).all())
    if kind == "zero_weight":
        assert torch.equal(_bits(v), _bits(bias16.expand(M, 256))) and bool((_bits(G) == 0).all())
    if kind == "ties":
        for got, W, b in ((v, Wv, bv), (G, Wg, None)):
            y = B.lin(feat, W, b)
            tie = (y >= 128) & (y < 256) & (y - torch.floor(y) == 0.5)
            assert float(tie.double().mean()) > 0.5
            assert torch.equal(got.double(), B.bf(y))
            print("ties: %d of %d results, all rounded to even" % (int(tie.sum()), y.numel()))


@pytest.mark.parametrize("n_img,S,nan_row,inf_row", [(17, 17, 40, 288), (17, 17, 288, 100), (3, 277, 830, 5), (51, 5, 31, 254)])
def test_pyramid_non_finite_rows_stay_in_their_rows(n_img, S, nan_row, inf_row):
    """a NaN in one row and an Inf in another -- among them the last row of a ragged tile, which the ring re-reads for the rows
    past the end: the NaN row comes back NaN in every column, the Inf row non-finite in every column, every other row
    bit-identical to the clean run."""
    M = n_img * S
    feat = Cs.pyr_feat(M, 8).to(DEV)
    jobs = [_job(0), _job(1), _job(2)]
    col = 77
    assert all(bool((W[:, col] != 0).all()) for W, _, _ in jobs)
    clean = _group(feat, n_img, S, jobs)
    bad = feat.clone()
    bad[nan_row, 3] = float("nan")
    bad[inf_row, col] = float("inf")
    got = _group(bad, n_img, S, jobs)
    others = torch.ones(M, dtype=torch.bool, device=DEV)
    others[[nan_row, inf_row]] = False
    for (_, _, planes), a, b in zip(jobs, clean, got):
        a, b = _rows(a, planes), _rows(b, planes)
        assert bool(torch.isnan(b[nan_row]).all())
        assert not bool(torch.isfinite(b[inf_row]).any())
        assert torch.equal(_bits(a[others]), _bits(b[others]))
        assert bool(torch.isfinite(a).all())


def test_pyramid_argument_checks():
    """MVG_E_BADARG with every output still NaN: njobs 0 and 9, a planes job with 192 columns or without bias, a row-major job
    with 256 columns, a null feat / weight / output, n_img = 0, S = 0."""
    n_img, S = 3, 40
    feat = Cs.pyr_feat(n_img * S, 2).to(DEV)
    value, G = _job(0), _job(1)
    both = [value, G]
    assert len(_group(feat, n_img, S, both)) == 2                                        # the good call
    for raw in (dict(njobs=0), dict(njobs=9), dict(N={0: 192}), dict(N={1: 256}), dict(no_feat=True), dict(no_W=0), dict(no_W=1),
                dict(no_out=0), dict(no_out=1), dict(arg_n_img=0), dict(arg_S=0)):
        _group(feat, n_img, S, both, expect=BADARG, **raw)
    _group(feat, n_img, S, [(value[0], None, True), G], expect=BADARG)                   # planes without bias
    _group(feat, n_img, S, [_job(j % 2) for j in range(8)], slots=64)                    # 8 jobs at the slot limit: runs


# ------------------------------------------------------------------------------------------------------------------ bf16 linear
_TORCH = {"bf16": torch.bfloat16, "f32": torch.float32}


def _strided(t, pad, fill):
    """(rows, n) -> the same values as a view of a (rows, n + pad) buffer whose padding columns hold `fill`."""
    wide = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=t.dtype, device=DEV)
    wide[:, :t.shape[1]] = t
    return wide[:, :t.shape[1]]


def _linear(a, a2, w, b, mask, relu, o_dt, strided=False, tiles=1, expect=0, **raw):
    """one raw mvg_linear_sum launch.  a (M, K) bf16 | fp32 and a2 (fp32 | None) on the device; strided: A (and A2) and out are views
    of wider buffers (A's padding holds NaN, out's the sentinel, which must survive).  raw: overrides for the argument checks
    (M, N, K, lda, ldc, off_a / off_w / off_out in bytes).  Returns out (M, N) or None for a refused call (checked: nothing written)."""
    L = _lib()
    M, K = a.shape
    N = w.shape[0]
    odt = _TORCH[o_dt]
    pad_a = (16 // a.element_size()) if strided else 0
    pad_o = (16 // (2 if o_dt == "bf16" else 4)) if strided else 0
    if strided:
        a = _strided(a, pad_a, float("nan"))
        a2 = None if a2 is None else _strided(a2, pad_a, float("nan"))
    ldc = N + pad_o
    buf, flat = _guarded(max(M, 1) * ldc, odt)
    out = flat.view(max(M, 1), ldc)
    out[:, N:] = SENT
    off = lambda t, k: None if t is None else C.c_void_p(t.data_ptr() + raw.get(k, 0))
    with L.tuning(linear_tiles=tiles):
        rc = L.load().mvg_linear_sum(off(a, "off_a"), L.ptr(a2), L.dtype_code(a.dtype), raw.get("lda", a.stride(0)), off(w, "off_w"),
                                     L.dtype_code(w.dtype), L.ptr(b), off(out, "off_out"), L.dtype_code(odt), raw.get("ldc", ldc), L.ptr(mask),
                                     1 if relu else 0, raw.get("M", M), raw.get("N", N), raw.get("K", K), L.stream_ptr())
        torch.cuda.synchronize()
    assert rc == expect, rc
    assert _guard_ok(buf, flat.numel())
    assert bool((out[:, N:] == _sent(odt)).all())
    if expect != 0 or raw.get("M", M) == 0:
        assert bool(torch.isnan(out[:, :N]).all())
        return None
    return out[:, :N].clone()


def _a_of(inp, a_dt):
    """(A, A2) on the device as the kernel takes them: bf16 A already rounded (no A2), fp32 A (+ A2) rounded on load."""
    if a_dt == "bf16":
        return B.operand(inp["a"]).to(DEV), None
    return inp["a"].to(DEV), None if inp["a2"] is None else inp["a2"].to(DEV)


@pytest.mark.parametrize("k", range(len(Cs.LIN_CASES)), ids=[Cs.lin_id(c) for c in Cs.LIN_CASES])
def test_linear_bf16_against_fp64(k):
    """every shape of the list (three tile shapes, ragged M and N, the linear_tiles knob) in the four dtype combinations, with the
    case's ReLU / row mask / bias / row strides / A + A2: within the bound element by element, masked rows exactly +0, the
    padding columns of a strided output untouched."""
    c = Cs.LIN_CASES[k]
    inp = Cs.lin_inputs(c, k)
    w = inp["w"].to(DEV)
    b = None if inp["b"] is None else inp["b"].to(DEV)
    mask = None if inp["mask"] is None else inp["mask"].to(DEV)
    for a_dt, o_dt in Cs.DTYPES:
        a, a2 = _a_of(inp, a_dt)
        got = _linear(a, a2, w, b, mask, c["relu"], o_dt, strided=c["strided"], tiles=c["tiles"])
        x = Cs.lin_operand(inp, a_dt).to(DEV)
        exp, bound = B.expected(x, w, b, out_bf16=o_dt == "bf16", relu=c["relu"], mask=mask)
        assert bool(torch.isfinite(got).all())
        _check("linear %s->%s" % (a_dt, o_dt), "%s tile %s" % (Cs.lin_id(c), B.linear_tile(c["M"], c["N"], c["tiles"])), got, exp, bound)
        if mask is not None:
            assert bool((_bits(got[mask == 0]) == 0).all())


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("tiles", [0, 1])
def test_linear_non_finite_inputs_stay_in_their_rows(tiles, relu):
    """a NaN and an Inf in single elements of A, the Inf in the last row of a ragged tile, which the loader re-reads for the rows
    past the end: the NaN row is NaN in every column -- behind the ReLU too, as torch.relu has it --, the Inf row +-Inf (behind
    the ReLU: +Inf or 0), every other row bit-identical to the clean run; the same NaN in a masked row gives exactly +0."""
    c = dict(M=129, N=136, K=128, a2=True, bias=True, mask=True)
    inp = Cs.lin_inputs(c, 3)
    w, b = inp["w"].to(DEV), inp["b"].to(DEV)
    nan_row, inf_row, col = 5, 128, 77
    assert bool((w[:, col] != 0).all())
    others = torch.ones(c["M"], dtype=torch.bool, device=DEV)
    others[[nan_row, inf_row]] = False
    hide = torch.ones(c["M"], dtype=torch.uint8, device=DEV)
    hide[nan_row] = 0
    for a_dt, o_dt in Cs.DTYPES:
        a, a2 = _a_of(inp, a_dt)
        clean = _linear(a, a2, w, b, None, relu, o_dt, tiles=tiles)
        bad = a.clone()
        bad[nan_row, 3] = float("nan")
        bad[inf_row, col] = float("inf")
        got = _linear(bad, a2, w, b, None, relu, o_dt, tiles=tiles)
        assert bool(torch.isnan(got[nan_row]).all()), (a_dt, o_dt)
        inf = got[inf_row].float().abs() == float("inf")
        assert bool((inf | (got[inf_row] == 0)).all() if relu else inf.all()), (a_dt, o_dt)
        assert bool(inf.any())
        assert torch.equal(_bits(got[others]), _bits(clean[others])), (a_dt, o_dt)
        masked = _linear(bad, a2, w, b, hide, relu, o_dt, tiles=tiles)
        assert bool((_bits(masked[nan_row]) == 0).all()), (a_dt, o_dt)
        assert torch.equal(_bits(masked[others]), _bits(clean[others]))


def test_linear_argument_checks():
    """MVG_E_BADARG with the output untouched: K not a multiple of 64, N not a multiple of 8, a misaligned A, W or out, an lda / ldc
    whose byte stride is not a multiple of 16, A2 with a bf16 A; M = 0 returns 0 and writes nothing."""
    M, N, K = 65, 136, 128
    gen = torch.Generator().manual_seed(1)
    a32 = torch.randn(M, K + 64, generator=gen).to(DEV)
    w = (torch.randn(N + 8, K + 64, generator=gen) / 8).to(BF).to(DEV)
    b = torch.randn(N + 8, generator=gen).to(DEV)
    for a_dt, o_dt in Cs.DTYPES:
        a = a32.to(_TORCH[a_dt])
        av, wv = a[:, :K], w[:N].reshape(-1)[:N * K].view(N, K)            # A: a view with lda = K + 64; W: contiguous (N, K)
        assert _linear(av, None, wv, b, None, False, o_dt) is not None                    # the good call
        half = 8 // a.element_size()
        for raw in (dict(K=96), dict(K=32), dict(N=132), dict(N=4), dict(off_a=8), dict(off_w=8), dict(off_out=8),
                    dict(lda=K + 64 + half), dict(ldc=N + 16 // (2 if o_dt == "bf16" else 4) // 2)):
            assert _linear(av, None, wv, b, None, False, o_dt, expect=BADARG, **raw) is None, (a_dt, o_dt, raw)
        assert _linear(av, None, wv, b, None, False, o_dt, M=0) is None
    a16 = a32.to(BF)[:, :K]
    assert _linear(a16, a32[:, :K], w[:N].reshape(-1)[:N * K].view(N, K), b, None, False, "f32", expect=BADARG) is None
