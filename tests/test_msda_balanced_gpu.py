"""The balanced mode of the deterministic sampling backward (csrc/msda_bwd.hip: bw_plan, bw_reduce_bal, bw_finish;
mvg_msda_backward_bal_f32 / _bf16) against the det mode, bit for bit: every comparison is torch.equal on the bit patterns, no
tolerance.  det itself is held to the fp64 statement by tests/test_msda_fp64.py, on the same cases (tests/msda_cases.py).

At chunk 256 (computed with tests/msda_ref.bins): one_bin has one bin of 903 entries (4 chunks, the last partial), coincident_centre /
_corner one bin of 4 096 entries (16 full chunks; _corner also adds to pixels that four tiles share), range / range_zero 24 two-chunk
bins at gradient scales 1, 1e6 and 1e-30; the other cases have no split bin and pin the unsplit path.  `clustered` (defined here) has
split bins at a map's corner, on the second level and in the second image, next to empty and one-chunk bins; its figures are
re-computed and asserted below.  Outputs are pre-filled with NaN between sentinel guards, the workspace with a byte pattern."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import msda_cases as MC
from tests import msda_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 1024
SENT_F = -7.25e5
F32, BF16 = torch.float32, torch.bfloat16
MVG_E_BADARG = 10001


def _lib():
    from mvgformer_amd import _lib as L
    return L


def _i64(t):
    flat = [int(x) for x in t.flatten().tolist()]
    return (C.c_int64 * len(flat))(*flat)


def _guarded(shape, fill):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENT_F, dtype=F32, device=DEV)
    buf[GUARD:GUARD + n] = fill
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guard_ok(buf):
    return bool((buf[:GUARD] == SENT_F).all()) and bool((buf[-GUARD:] == SENT_F).all())


def clustered():
    """two images, two levels (20 x 27: partial tiles in both directions; 9 x 13), M = 2: every sample of image 0 around (0.93, 0.90)
    -- the corner of the maps, a part of them outside --, the first 80 queries of image 1 around the centre, the rest uniform."""
    c = MC._generic([(20, 27), (9, 13)], N=2, M=2, D=32, Lq=160, P=4, seed=301)
    rs = np.random.RandomState(302)
    loc = c["loc"]
    a = rs.standard_normal(tuple(loc[0].shape)).astype(np.float32)
    b = rs.standard_normal(tuple(loc[1, :80].shape)).astype(np.float32)
    loc[0] = torch.tensor([0.93, 0.90]) + 0.04 * torch.from_numpy(a)
    loc[1, :80] = torch.tensor([0.5, 0.5]) + 0.02 * torch.from_numpy(b)
    return c


def boundary(Lq):
    """one 8 x 8 map, M = L = P = 1, locations in [0, 1]^2: one bin of Lq entries"""
    return MC._generic([(8, 8)], 1, 1, 32, Lq, 1, 310 + Lq, lo=0.0, hi=1.0)


@functools.lru_cache(maxsize=None)
def _case(name):
    if name == "clustered":
        return clustered()
    if name.startswith("boundary_"):
        return boundary(int(name.split("_")[1]))
    return MC.case(name)


def _bin_counts(c):
    N, S, M, D = c["value"].shape
    b, T_total = R.bins(c["loc"], c["shapes"], M, MC.BW_T)
    bpi = T_total * M
    key = (torch.arange(N).view(N, 1, 1, 1, 1) * bpi + b)[b >= 0]
    return torch.bincount(key, minlength=N * bpi), bpi, T_total, b


def _backward(c, bf16, chunk=None, ws_byte=0xA5, go=None):
    """one launch of det (chunk None) or balanced (chunk 0 / 256 / ...) through the C ABI on guarded outputs -> (rc, three gradients)"""
    Lm = _lib()
    lib = Lm.load()
    value = c["value"]
    go = c["go"] if go is None else go                       # nonfinite_go: WITH its NaN / Inf entries, det takes them
    N, S, M, D = value.shape
    _, Lq, _, L, P, _ = c["loc"].shape
    v = value.to(DEV, BF16 if bf16 else F32).contiguous()
    loc, wgt, god = (t.to(DEV, F32).contiguous() for t in (c["loc"], c["weight"], go))
    gvb, gv = _guarded((N, S, M, D), float("nan"))
    glb, gl = _guarded((N, Lq, M, L, P, 2), float("nan"))
    gab, ga = _guarded((N, Lq, M, L, P), float("nan"))
    dims = (N, S, M, D, L, Lq, P)
    shapes_c, starts_c = _i64(c["shapes"]), _i64(c["starts"])
    det_bytes = int(lib.mvg_msda_backward_det_workspace(*dims, shapes_c))
    assert det_bytes > 0
    if chunk is None:
        nbytes, tail = det_bytes, ()
        fn = lib.mvg_msda_backward_det_bf16 if bf16 else lib.mvg_msda_backward_det_f32
    else:
        nbytes, tail = int(lib.mvg_msda_backward_bal_workspace(*dims, shapes_c, chunk)), (chunk,)
        fn = lib.mvg_msda_backward_bal_bf16 if bf16 else lib.mvg_msda_backward_bal_f32
        if nbytes == 0:                      # an illegal chunk: the call itself must refuse it; hand it det's workspace
            nbytes = det_bytes
        else:
            assert nbytes >= det_bytes and nbytes % 256 == 0
    wsb = torch.full((nbytes + 2 * GUARD,), 0x3C, dtype=torch.uint8, device=DEV)
    ws = wsb[GUARD:GUARD + nbytes]
    ws.fill_(ws_byte)
    rc = fn(Lm.ptr(v), shapes_c, starts_c, Lm.ptr(loc), Lm.ptr(wgt), Lm.ptr(god), Lm.ptr(gv), Lm.ptr(gl), Lm.ptr(ga), *dims,
            Lm.ptr(ws), nbytes, Lm.stream_ptr(), *tail)
    torch.cuda.synchronize()
    assert bool((wsb[:GUARD] == 0x3C).all()) and bool((wsb[-GUARD:] == 0x3C).all())
    assert _guard_ok(gvb) and _guard_ok(glb) and _guard_ok(gab)
    return rc, (gv.clone(), gl.clone(), ga.clone())


@functools.lru_cache(maxsize=None)
def _det(name, bf16):
    """det's three gradients of a case (computed once, read-only)"""
    rc, out = _backward(_case(name), bf16)
    assert rc == 0
    return out


def _bits(t):
    return t.view(torch.int32)


def _assert_same_bits(got, want, what):
    for g, a, b in zip(("grad_value", "grad_loc", "grad_attn"), got, want):
        diff = int((_bits(a) != _bits(b)).sum())
        assert diff == 0, "%s %s: %d of %d elements differ from det" % (what, g, diff, a.numel())


def _balanced_equals_det(name, bf16, chunk, ws_byte=0xA5):
    rc, got = _backward(_case(name), bf16, chunk, ws_byte)
    assert rc == 0, rc
    _assert_same_bits(got, _det(name, bf16), "%s %s chunk %d" % (name, "bf16" if bf16 else "fp32", chunk))
    return got


# ------------------------------------------------------------------------------------------------------------- 1. the cases of det
@pytest.mark.parametrize("chunk", [0, 256, 512])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", MC.DET_CASES)
def test_balanced_equals_det_on_every_det_case(name, bf16, chunk):
    _balanced_equals_det(name, bf16, chunk)


def test_the_det_cases_split_where_the_docstring_says():
    """at chunk 256: one_bin 1 x 4 chunks (903 entries), coincident_* 1 x 16 full chunks, range / range_zero 24 two-chunk bins"""
    def chunks(name):
        cnt = _bin_counts(MC.case(name))[0]
        return cnt, (cnt + 255) // 256
    cnt, n = chunks("one_bin")
    assert int(cnt.max()) == 903 and int(n.max()) == 4 and int((n > 1).sum()) == 1
    for name in ("coincident_centre", "coincident_corner"):
        cnt, n = chunks(name)
        assert int(cnt.max()) == 4096 and int(n.max()) == 16 and int((n > 1).sum()) == 1
    for name in ("range", "range_zero"):
        cnt, n = chunks(name)
        assert int((n == 2).sum()) == 24 and int(n.max()) == 2


# -------------------------------------------------------------------------------------------------------------------- 2. clustered
def test_clustered_has_the_bins_it_is_meant_to_have():
    c = _case("clustered")
    cnt, bpi, T_total, b = _bin_counts(c)
    n = (cnt + 255) // 256
    M = c["value"].shape[2]
    split = torch.nonzero(n >= 2).flatten()
    tile = (split % bpi) // M
    level1_tile0 = 3 * 4                                       # level 0 is 20 x 27: 3 x 4 tiles
    print("clustered: %d bins, %d empty, %d one-chunk, %d two-chunk, %d with >= 3 chunks, largest %d, split %s, out of map %d, "
          "ambiguous %d" % (cnt.numel(), int((cnt == 0).sum()), int((n == 1).sum()), int((n == 2).sum()), int((n >= 3).sum()),
                            int(cnt.max()), [(int(s), int(cnt[s])) for s in split], int((b < 0).sum()),
                            int(R.ambiguous(c["loc"], c["shapes"]).sum())))
    assert int((n >= 3).sum()) >= 2
    assert split.numel() >= 6
    assert int((tile >= level1_tile0).sum()) >= 1              # a split bin on level 1
    assert int((split >= bpi).sum()) >= 1                      # a split bin in image 1
    assert int((cnt == 0).sum()) >= 10
    assert int((n == 1).sum()) >= 20
    assert bool((cnt[split] % 256 != 0).any())                 # a partial last chunk
    assert int(R.ambiguous(c["loc"], c["shapes"]).sum()) == 0


@pytest.mark.parametrize("chunk", [0, 256, 512])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_balanced_equals_det_on_clustered(bf16, chunk):
    _balanced_equals_det("clustered", bf16, chunk)


# ----------------------------------------------------------------------------------------------------------- 3. the chunk boundary
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("Lq", [256, 257, 512, 513])
def test_chunk_boundary(Lq, bf16):
    """one bin of Lq entries at chunk 256: 1 chunk, 2 chunks with a last chunk of one entry, 2 full chunks, 3 chunks"""
    name = "boundary_%d" % Lq
    cnt = _bin_counts(_case(name))[0]
    assert cnt.numel() == 1 and int(cnt[0]) == Lq              # locations in [0, 1]^2 never leave the map
    _balanced_equals_det(name, bf16, 256)


# ------------------------------------------------------------------------------------- 4. repeats, and what the workspace held before
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", ["clustered", "coincident_corner", "one_bin"])
def test_balanced_repeats_itself_and_ignores_what_the_workspace_held(name, bf16):
    """two runs give the same bits (det's), and so does a workspace pre-filled with 0x00 / 0xA5 / 0xFF: the interior of a split bin
    is zeroed by bw_plan, the item table and the item counts are written by it before bw_reduce_bal reads them"""
    for ws_byte in (0xA5, 0xA5, 0x00, 0xFF):
        _balanced_equals_det(name, bf16, 256, ws_byte)


# ---------------------------------------------------------------------------------------------------------------- 5. graph capture
def _uniform_variant(c):
    u = MC._generic([(20, 27), (9, 13)], N=2, M=2, D=32, Lq=160, P=4, seed=303)
    assert all(u[k].shape == c[k].shape for k in ("value", "loc", "weight", "go"))
    return u


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_captured_balanced_backward_replays_on_other_data(bf16):
    """ops.msda_backward in balanced mode captured once on static buffers that hold `clustered`; replayed there and, after a
    uniform-location variant of the same shapes is copied in, again: each replay equals det on that data -- the launch does not depend
    on the data (a grid sized by the clustered item count would lose items of the variant, and the other way round)"""
    from mvgformer_amd import ops
    c = _case("clustered")
    u = _uniform_variant(c)
    cnt_c, cnt_u = _bin_counts(c)[0], _bin_counts(u)[0]
    assert int(((cnt_c + 255) // 256).clamp_min(1).sum()) != int(((cnt_u + 255) // 256).clamp_min(1).sum())    # other item counts
    vdt = BF16 if bf16 else F32
    keys = ("value", "loc", "weight", "go")
    static = {k: c[k].to(DEV, vdt if k == "value" else F32).contiguous() for k in keys}
    shapes, starts = c["shapes"].to(DEV), c["starts"].to(DEV)
    saved = ops.BACKWARD_MODE, ops.BACKWARD_CHUNK

    def call():
        return ops.msda_backward(static["value"], shapes, starts, static["loc"], static["weight"], static["go"])

    def load(case):
        for k in keys:
            static[k].copy_(case[k].to(DEV, static[k].dtype))

    try:
        ops.BACKWARD_MODE, ops.BACKWARD_CHUNK = "det", None
        want = {}
        for tag, case in (("uniform", u), ("clustered", c)):
            load(case)
            want[tag] = [t.clone() for t in call()]
        ops.BACKWARD_MODE, ops.BACKWARD_CHUNK = "balanced", 256
        _assert_same_bits(call(), want["clustered"], "eager balanced")      # one eager call before the capture
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            call()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = call()
        for tag, case in (("clustered", c), ("uniform", u), ("clustered", c)):
            load(case)
            for t in out:
                t.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            _assert_same_bits(out, want[tag], "replay on " + tag)
    finally:
        ops.BACKWARD_MODE, ops.BACKWARD_CHUNK = saved


# ------------------------------------------------------------------------------------------------- 6. through autograd and the step
@pytest.mark.parametrize("tdt", [F32, BF16], ids=["fp32", "bf16"])
def test_graphed_balanced_step_equals_eager_det_step(tdt):
    """the setup of tests/test_train_graph_gpu.py (mini5, NQ 128, 2 layers, KNN 5): three replays of a GraphedTrainStep captured under
    BACKWARD_MODE = "balanced" equal three eager det steps from the same state in every parameter, moment, loss and norm"""
    from mvgformer_amd import ops
    from tests import test_train_graph_gpu as TG
    saved = ops.BACKWARD_MODE, ops.BACKWARD_CHUNK
    try:
        ops.BACKWARD_MODE, ops.BACKWARD_CHUNK = "det", None
        want = TG._run(TG.Rig(tdt), 3, replay=False)
        ops.BACKWARD_MODE, ops.BACKWARD_CHUNK = "balanced", 256
        rig = TG.Rig(tdt).captured()
        got = TG._run(rig, 3, replay=True)
        TG._assert_same(got, want, "balanced replay vs det eager")
        assert len({float(m[0]) for m in got[0]}) == 3                       # the weights do move
    finally:
        ops.BACKWARD_MODE, ops.BACKWARD_CHUNK = saved


# ------------------------------------------------------------------------------------------------------------------- 7. arguments
@pytest.mark.parametrize("chunk", [100, -256])
def test_illegal_chunk_is_refused(chunk):
    """chunk 100 (no multiple of a workgroup pass) and -256: MVG_E_BADARG from both entry points, and nothing is launched (the outputs
    keep their NaN fill)"""
    for bf16 in (False, True):
        rc, out = _backward(_case("one_bin"), bf16, chunk)
        assert rc == MVG_E_BADARG
        assert all(bool(torch.isnan(t).all()) for t in out)


def test_balanced_mode_has_dets_availability():
    """D = 16: no deterministic form (workspace 0) -- ops.msda_backward in balanced mode runs the atomic kernel, as in det mode"""
    from mvgformer_amd import ops
    Lm = _lib()
    lib = Lm.load()
    c = MC.case("generic_d16")
    N, S, M, D = c["value"].shape
    _, Lq, _, L, P, _ = c["loc"].shape
    shapes_c = _i64(c["shapes"])
    assert int(lib.mvg_msda_backward_det_workspace(N, S, M, D, L, Lq, P, shapes_c)) == 0
    assert int(lib.mvg_msda_backward_bal_workspace(N, S, M, D, L, Lq, P, shapes_c, 256)) == 0
    args = [c[k].to(DEV) for k in ("value", "shapes", "starts", "loc", "weight", "go")]
    ref, k = MC.reference("generic_d16", "f32")
    saved = ops.BACKWARD_MODE, ops.BACKWARD_CHUNK
    try:
        got = {}
        for mode in ("atomic", "det", "balanced"):
            ops.BACKWARD_MODE, ops.BACKWARD_CHUNK = mode, 256 if mode == "balanced" else None
            got[mode] = ops.msda_backward(*args)
        torch.cuda.synchronize()
    finally:
        ops.BACKWARD_MODE, ops.BACKWARD_CHUNK = saved
    for mode in ("det", "balanced"):
        # grad_loc / grad_attn of the atomic kernel have one writer per sample: the same bits; grad_value: fp32 atomics, within the bar
        assert torch.equal(_bits(got[mode][1]), _bits(got["atomic"][1])) and torch.equal(_bits(got[mode][2]), _bits(got["atomic"][2]))
        err = (got[mode][0].double().cpu() - ref["grad_value"]).abs()
        assert bool((err <= MC.bar(ref, k, "grad_value")).all())
    with pytest.raises(Lm.MvgError):
        ops.BACKWARD_MODE, ops.BACKWARD_CHUNK = "balanced", 100
        try:
            ops.msda_backward(*[_case("one_bin")[k].to(DEV) for k in ("value", "shapes", "starts", "loc", "weight", "go")])
        finally:
            ops.BACKWARD_MODE, ops.BACKWARD_CHUNK = saved
