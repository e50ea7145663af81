"""mvg_structural_triangulate on the device: bit-equal to its numpy restatement (tests/st_ref.py) over both addressing modes, both
methods, both trees and the step counts; against the reference's outputs (tests/golden/st.npz) at the CPU test's bars; independent
of the other persons of a launch; status codes; argument refusals."""
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import st_ref
from tests.golden.st_cases import scene
from tests.test_structural_cpu import BAR_FP32_REF, BAR_FP64_REF, golden, golden_cases, scene_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _parent(J):
    from mvgformer_amd.structural import H36M17_PARENT, PANOPTIC15_PARENT
    return {15: PANOPTIC15_PARENT, 17: H36M17_PARENT}[J]


@functools.lru_cache(maxsize=None)
def _inputs(B, V, NQ, J, seed=0):
    """NQ queries per batch element as the kernel wants them: ud (B, V, NQ*J, 2), conf (B, V, NQ*J), Pm (B, V, 3, 4), per-query
    bone lengths (B, NQ, J-1); 2 px of noise; the second element's projection matrices are rescaled (the same geometry, other bits)"""
    sc = scene(seed + 100 * V + J, V, _parent(J), persons=B * NQ, noise=2.0)
    ud = sc["ud"].reshape(B, NQ, V, J, 2).transpose(0, 2, 1, 3, 4).reshape(B, V, NQ * J, 2)
    conf = sc["conf"].reshape(B, NQ, V, J).transpose(0, 2, 1, 3).reshape(B, V, NQ * J)
    Pm = np.broadcast_to(sc["Pm"], (B, V, 3, 4)).copy()
    Pm[1:] *= np.float32(1.5)
    return np.ascontiguousarray(ud), np.ascontiguousarray(conf), Pm, sc["bone_len"].reshape(B, NQ, J - 1)


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(DEV)  # a writable, contiguous copy


def _launch(ud, conf, Pm, parent, bone_len, **kw):
    from mvgformer_amd import ops
    for k in ("valid", "rows", "count"):
        if kw.get(k) is not None:
            kw[k] = _dev(kw[k])
    X, status = ops.structural_triangulate(_dev(ud), _dev(conf), _dev(Pm), parent, _dev(bone_len), **kw)
    torch.cuda.synchronize()
    return X.cpu().numpy(), status.cpu().numpy()


def _same(got, want):
    return np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])


# the product of the grid: (V, P, J) by parametrisation, and inside a test every (method, n_steps) x weights given / null x shared /
# per-person lengths; LS takes no steps, so it runs once
SHAPES = list(itertools.product((3, 5), (1, 5, 8), (15, 17)))
SOLVES = [("LS", 1), ("ST", 1), ("ST", 3), ("ST", 8)]
COMBOS = list(itertools.product(SOLVES, (True, False), (False, True)))


@pytest.mark.parametrize("V,P,J", SHAPES)
def test_dense_mode_equals_the_restatement(V, P, J):
    ud, conf_all, Pm, bl = _inputs(2, V, P, J)
    valid = np.ones((2, P), np.uint8)
    valid[1, ::3] = 0                                   # element 0 whole, element 1 loses every third query
    dev = [_dev(a) for a in (ud, conf_all, Pm, bl, bl[0, 0], valid)]
    from mvgformer_amd import ops
    for (method, steps), weights, per_person in COMBOS:
        conf, lengths = (conf_all if weights else None), (bl if per_person else bl[0, 0])
        for mask in ((None, valid) if (method, steps, weights, per_person) == ("ST", 3, True, True) else (valid,)):
            X, status = ops.structural_triangulate(dev[0], dev[1] if weights else None, dev[2], _parent(J), dev[3] if per_person else dev[4],
                                                   valid=None if mask is None else dev[5], n_steps=steps, method=method)
            got = (X.cpu().numpy(), status.cpu().numpy())
            want = st_ref.dense(ud, conf, Pm, _parent(J), lengths, valid=mask, method=method, n_steps=steps)
            assert _same(got, want), (method, steps, weights, per_person, np.abs(got[0] - want[0]).max(), got[1], want[1])
            # a person is computed (0, or 2 where a later step's multiplier system was not positive definite) or masked out (-1)
            assert (got[1] >= 0).sum() == (2 * P if mask is None else int(valid.sum())) and got[0].dtype == np.float32
            assert (got[1] == 0).any()


@pytest.mark.parametrize("V,R,J", SHAPES)
def test_rows_mode_equals_the_restatement(V, R, J):
    NQ = R + 3
    ud, conf_all, Pm, bl = _inputs(2, V, NQ, J, seed=7)
    rng = np.random.default_rng(R)
    wide = np.stack([rng.permutation(NQ) for _ in range(2)]).astype(np.int32)       # (B, NQ): rows are its first R columns
    own = np.stack([bl[b, wide[b, :R]] for b in range(2)])                          # per person: the lengths of the query a row names
    dev = [_dev(a) for a in (ud, conf_all, Pm, own, bl[1, 2], wide)]
    from mvgformer_amd import ops

    def both(count, method, steps, weights, per_person, rows=None):
        rows_dev = dev[5][:, :R] if rows is None else _dev(rows)
        X, status = ops.structural_triangulate(dev[0], dev[1] if weights else None, dev[2], _parent(J), dev[3] if per_person else dev[4],
                                               rows=rows_dev, count=_dev(count), n_steps=steps, method=method)
        got = (X.cpu().numpy(), status.cpu().numpy())
        want = st_ref.by_rows(ud, conf_all if weights else None, Pm, _parent(J), own if per_person else bl[1, 2],
                              wide[:, :R] if rows is None else rows, count, method=method, n_steps=steps)
        assert _same(got, want), (count, method, steps, weights, per_person, np.abs(got[0] - want[0]).max(), got[1], want[1])
        return got

    for (method, steps), weights, per_person in COMBOS:                             # count 3 (or R below 3) and R
        got = both(np.array([[min(3, R), 5], [R, 0]], np.int32), method, steps, weights, per_person)
        assert [(got[1][b] >= 0).sum() for b in range(2)] == [min(3, R), R] and (got[1][0, min(3, R):] == -1).all()
    for counts in ((0, min(3, R)), (R + 4, 0), None):                               # count 0, above R, and no count at all
        count = None if counts is None else np.array([[counts[0], 5], [counts[1], 0]], np.int32)
        got = both(count, "ST", 3, False, True)
        live = [R, R] if counts is None else [min(c, R) for c in counts]
        assert [(got[1][b] >= 0).sum() for b in range(2)] == live and [(got[1][b] == -1).sum() for b in range(2)] == [R - n for n in live]
    bad = wide[:, :R].copy()                            # a row index outside the queries is not computed
    bad[0, 0], bad[1, R - 1] = NQ, -1
    got = both(None, "ST", 1, True, False, rows=bad)
    assert got[1][0, 0] == -1 and got[1][1, R - 1] == -1


def test_kernel_meets_the_reference_outputs_at_the_cpu_bars():
    """the kernel's X is the fp64 result rounded once to fp32: half an fp32 ulp of the coordinate comes on top of the CPU bars"""
    g = golden()
    worst = {"pan": 0.0, "h36m": 0.0}
    for key, name, tag, method, steps, w in golden_cases():
        ud, conf, Pm, bl = scene_inputs(key)
        V, J = ud.shape[1], ud.shape[2]
        udq = ud.transpose(1, 0, 2, 3).reshape(1, V, 4 * J, 2)
        cfq = conf.transpose(1, 0, 2).reshape(1, V, 4 * J) if w == "w" else None
        X, status = _launch(udq, cfq, Pm[:1], g[name + "_parent"].tolist(), bl[None], n_steps=steps, method=method)
        want = g["%s_%s_%s" % (key, tag, w)].astype(np.float64)
        assert (status == 0).all(), (key, tag, w, status)
        err = np.abs(X[0].astype(np.float64) - want)
        half_ulp = 0.5 * np.spacing(np.maximum(np.abs(X[0]), np.abs(want).astype(np.float32))).astype(np.float64)
        bar = BAR_FP32_REF if name == "pan" else BAR_FP64_REF
        worst[name] = max(worst[name], float((err - half_ulp).max()))
        assert (err <= bar + half_ulp).all(), (key, tag, w, float(err.max()))
    print("max (|kernel - reference| - half an fp32 ulp) mm: fp32 reference %.4g, fp64 reference %.4g" % (worst["pan"], worst["h36m"]))


def test_a_person_does_not_depend_on_the_others_of_the_launch():
    V, P, J = 5, 8, 15
    ud, conf, Pm, bl = _inputs(2, V, P, J, seed=3)
    base = _launch(ud, conf, Pm, _parent(J), bl, n_steps=3, method="ST")
    perm = np.random.default_rng(1).permutation(P)
    udp = ud.reshape(2, V, P, J, 2)[:, :, perm].reshape(2, V, P * J, 2)
    cfp = conf.reshape(2, V, P, J)[:, :, perm].reshape(2, V, P * J)
    got = _launch(udp, cfp, Pm, _parent(J), bl[:, perm], n_steps=3, method="ST")
    assert _same(got, (base[0][:, perm], base[1][:, perm]))
    alone = _launch(ud[:1, :, :J], conf[:1, :, :J], Pm[:1], _parent(J), bl[:1, :1], n_steps=3, method="ST")
    assert _same(alone, (base[0][:1, :1], base[1][:1, :1]))


def test_poisoned_persons_get_status_1_and_disturb_nobody():
    V, P, J = 3, 5, 15
    ud, conf, Pm, bl = (a.copy() for a in _inputs(2, V, P, J, seed=5))
    clean = _launch(ud, conf, Pm, _parent(J), bl, n_steps=3, method="ST")
    conf.reshape(2, V, P, J)[0, :, 1] = 0.0                     # nobody saw person (0, 1)
    ud.reshape(2, V, P, J, 2)[1, 2, 3, 9, 1] = np.nan           # one NaN observation of person (1, 3)
    got = _launch(ud, conf, Pm, _parent(J), bl, n_steps=3, method="ST")
    assert _same(got, st_ref.dense(ud, conf, Pm, _parent(J), bl, method="ST", n_steps=3))
    want_status = np.zeros((2, P), np.int32)
    want_status[0, 1] = want_status[1, 3] = 1
    assert np.array_equal(got[1], want_status) and not got[0][0, 1].any() and not got[0][1, 3].any()
    keep = want_status == 0
    assert np.array_equal(got[0][keep].view(np.uint32), clean[0][keep].view(np.uint32))


def test_unsupported_arguments_are_refused():
    from mvgformer_amd import _lib, ops
    ud, conf, Pm, bl = (_dev(a) for a in _inputs(2, 3, 5, 15))
    parent = _parent(15)
    ok = ops.structural_triangulate(ud, conf, Pm, parent, bl)
    assert tuple(ok[0].shape) == (2, 5, 15, 3) and tuple(ok[1].shape) == (2, 5)
    chain18 = (-1,) + tuple(range(17))
    with pytest.raises(_lib.MvgError, match="18 joints"):
        ops.structural_triangulate(ud.reshape(2, 3, -1, 2)[:, :, :72], None, Pm, chain18, None, method="LS")
    for steps in (0, 9):
        with pytest.raises(_lib.MvgError, match="n_steps"):
            ops.structural_triangulate(ud, conf, Pm, parent, bl, n_steps=steps)
    # the library itself refuses the same, and launches nothing
    lib, out = _lib.load(), ops.structural_buffers(2, 5, 15, DEV)
    import ctypes
    par = (ctypes.c_int * 18)(*chain18)

    def raw(J, steps, method=1, parent_c=par):
        return lib.mvg_structural_triangulate(_lib.ptr(ud), None, _lib.ptr(Pm), None, None, 0, None, parent_c, _lib.ptr(bl), 1, method,
                                              steps, _lib.ptr(out["poses"]), _lib.ptr(out["status"]), 3, 2, 5, 5, J, _lib.stream_ptr())
    assert raw(18, 1) == raw(15, 0) == raw(15, 9) == raw(15, 1, method=2) == 10001
    assert raw(15, 1, parent_c=(ctypes.c_int * 15)(*([-1] + [1] * 14))) == 10001           # joint 1 hangs from itself
    for bad, kw in ((ud.double(), {}), (ud[:, :, ::2], {}), (ud, dict(conf=conf.half())), (ud, dict(Pm=Pm.double())),
                    (ud, dict(bl=bl.double())), (ud, dict(bl=bl[:, :, :5])), (ud, dict(valid=torch.ones((2, 5), device=DEV))),
                    (ud, dict(rows=torch.zeros((2, 5), dtype=torch.int64, device=DEV))),
                    (ud, dict(count=torch.zeros((2, 2), dtype=torch.int32, device=DEV)))):
        with pytest.raises(RuntimeError, match="mvg_structural_triangulate"):
            ops.structural_triangulate(bad, kw.get("conf", conf), kw.get("Pm", Pm), parent, kw.get("bl", bl), valid=kw.get("valid"),
                                       rows=kw.get("rows"), count=kw.get("count"))
    with pytest.raises(RuntimeError, match="host ints"):
        ops.structural_triangulate(ud, conf, Pm, torch.tensor(parent, device=DEV), bl)
    torch.cuda.synchronize()
