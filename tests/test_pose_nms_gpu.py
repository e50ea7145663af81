"""ops.pose_nms / mvg_pose_nms on the MI355X against the numpy restatement of its contract (tests/nms_ref.py, pinned to the
reference in tests/test_pose_nms_cpu.py).  Every comparison is exact: keep[:count], count and dets[:count] equal the
restatement's on the same fp32 array, the rows behind the count are -1 (keep) or 0 with flag -1 (dets)."""
import numpy as np
import pytest
import torch

from tests import nms_cases, nms_ref
from tests.golden.eval_cases import NMS_CASES, panoptic_scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _poisoned(B, N, J, dets_rows=None):
    from mvgformer_amd import ops
    out = ops.pose_nms_buffers(B, N, J, dets_rows, DEV)
    for t in out.values():
        t.view(torch.uint8).fill_(0xFF)
    return out


def _run(pred, poison=True, **kw):
    """pred (B, N, J, 5) numpy fp32 -> keep, count, dets as numpy, from buffers filled with 0xFF before the call"""
    from mvgformer_amd import ops
    B, N, J = pred.shape[:3]
    out = _poisoned(B, N, J, kw.get("dets_rows")) if poison else None
    keep, count, dets = ops.pose_nms(torch.from_numpy(np.array(pred)).to(DEV), out=out, **kw)
    return keep.cpu().numpy(), count.cpu().numpy(), dets.cpu().numpy()


def _check_element(pred, want, keep, count, dets):
    """one batch element against the restatement's (keep, count, dets, stats)"""
    w_keep, w_count, w_dets, _ = want
    k = int(count[0])
    assert count.tolist() == w_count
    assert keep[:k].tolist() == w_keep
    assert (keep[k:] == -1).all()
    rows = min(k, len(dets))
    assert np.array_equal(dets[:rows], w_dets[:rows], equal_nan=True)
    tail = dets[rows:]
    assert (tail[..., 3] == -1).all() and (tail[..., :3] == 0).all() and (tail[..., 4] == 0).all()


@pytest.mark.parametrize("name", sorted(NMS_CASES))
def test_golden_cases(name):
    """the reference's golden scenes cast to fp32 (flags as generated), the restatement run on the cast array"""
    spec = NMS_CASES[name]
    preds, _, _ = panoptic_scene(spec["seed"], frames=spec["frames"])
    kw = dict(dist_thr=spec["dist_thr"], num_nearby_joints_thr=spec["num_nearby"], max_dets=spec.get("max_dets", -1))
    for variant in ("flags", "all"):
        for f, p in enumerate(preds):
            p32 = p.astype(np.float32)
            if variant == "all":
                p32[:, :, 3] = 0.0                                   # every row a candidate, as the golden keep lists were made
            keep, count, dets = _run(p32[None], **kw)
            _check_element(p32, nms_ref.pose_nms(p32, **kw), keep[0], count[0], dets[0])


@pytest.mark.parametrize("name", ["n1", "n63", "n64", "n65", "n130", "n130_flagged", "n65_j14", "n130_maxdets", "n1024",
                                  "n2048_sparse"])
def test_generated_scenes(name):
    """word boundaries of the bit matrix (63 / 64 / 65 / 130), ~40 % of the rows not candidates (compaction, rank -> row), J = 14
    with the J // 2 default, max_dets, every row of 1024 a candidate (16 words, 1024 greedy steps), 2048 rows at ~10 %"""
    pred, kw, want = nms_cases.generated(name)
    keep, count, dets = _run(pred[None], **kw)
    _check_element(pred, want, keep[0], count[0], dets[0])


@pytest.mark.parametrize("name", ["ties_small", "ties_large", "ties_large_maxdets", "zero_extent", "nan_coordinate", "all_flagged",
                                  "one_candidate"])
def test_degenerate_inputs(name):
    pred, kw, want = nms_cases.degenerate_reference(name)
    keep, count, dets = _run(pred[None], **kw)
    _check_element(pred, want, keep[0], count[0], dets[0])
    if name in ("zero_extent", "nan_coordinate"):
        assert count[0, 1] == 1
    if name == "all_flagged":
        assert count[0].tolist() == [0, 0]


def test_batch_of_three_equals_single_calls():
    """a full scene, an element without a candidate and an element with one, in one call"""
    full = nms_cases.generated("n130_flagged")
    N = len(full[0])
    none = np.array(full[0])
    none[:, :, 3] = -1.0
    one = np.array(none)
    one[77, :, 3] = 0.0
    batch = np.stack([full[0], none, one])
    keep, count, dets = _run(batch)
    assert count[1].tolist() == [0, 0] and count[2].tolist() == [1, 0] and keep[2, 0] == 77
    for b in range(3):
        _check_element(batch[b], nms_ref.pose_nms(batch[b]) if b else full[2], keep[b], count[b], dets[b])
        k1, c1, d1 = _run(batch[b:b + 1])
        assert np.array_equal(k1[0], keep[b]) and np.array_equal(c1[0], count[b]) and np.array_equal(d1[0], dets[b])
    assert N == 130


def test_two_calls_are_bit_identical_and_poison_does_not_matter():
    pred, kw, want = nms_cases.generated("n130")
    a = _run(pred[None], poison=True)
    b = _run(pred[None], poison=True)
    c = _run(pred[None], poison=False)                               # fresh buffers from the allocator
    for x, y, z in zip(a, b, c):
        assert x.tobytes() == y.tobytes() == z.tobytes()
    _check_element(pred, want, a[0][0], a[1][0], a[2][0])


def test_static_buffers_are_rewritten_by_every_call():
    """the serving pattern: the same out buffers for frame after frame; a frame with fewer poses leaves nothing behind"""
    from mvgformer_amd import ops
    big, _, want_big = nms_cases.generated("n130")
    small = np.array(big)
    small[10:, :, 3] = -1.0
    out = _poisoned(1, 130, 15, dets_rows=32)
    for pred, want in ((big, want_big), (small, nms_ref.pose_nms(small)), (big, want_big)):
        keep, count, dets = ops.pose_nms(torch.from_numpy(np.array(pred))[None].to(DEV), dets_rows=32, out=out)
        assert dets.shape == (1, 32, 15, 5) and keep.data_ptr() == out["keep"].data_ptr()
        _check_element(pred, want, keep[0].cpu().numpy(), count[0].cpu().numpy(), dets[0].cpu().numpy())


def test_filter_and_nms_device_equals_host_path():
    from mvgformer_amd import evaluate as E
    preds, _, _ = panoptic_scene(11, frames=6)
    for p in preds:
        p32 = torch.from_numpy(p.astype(np.float32))
        want = E.filter_and_nms(p32.clone())
        got = E.filter_and_nms_device(p32.to(DEV))
        assert got.is_cuda and torch.equal(got.cpu(), want)
    N = min(len(p) for p in preds)
    batch = torch.stack([torch.from_numpy(p[:N].astype(np.float32)) for p in preds[:3]])
    got = E.filter_and_nms_device(batch.to(DEV))
    assert isinstance(got, list) and len(got) == 3
    for g, b in zip(got, batch):
        assert torch.equal(g.cpu(), E.filter_and_nms(b.clone()))


def test_operator_is_capturable_in_a_graph():
    """fixed shapes, no synchronisation: capture once, replay on two inputs"""
    from mvgformer_amd import ops
    a, _, want_a = nms_cases.generated("n130")
    b, _, want_b = nms_cases.generated("n130_flagged")
    src = torch.from_numpy(np.array(a))[None].to(DEV)
    out = _poisoned(1, 130, 15)
    ops.pose_nms(src, out=out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.pose_nms(src, out=out)
    for pred, want in ((b, want_b), (a, want_a)):
        src.copy_(torch.from_numpy(np.array(pred))[None])
        g.replay()
        torch.cuda.synchronize()
        _check_element(pred, want, out["keep"][0].cpu().numpy(), out["count"][0].cpu().numpy(), out["dets"][0].cpu().numpy())
