"""serving.GraphedDecoder(postprocess=...): classification filter + NMS captured in the decoder's HIP graph, and
validate.main --device-nms.  mini5, 2 layers, valid_fraction 0.5, bf16 as in tests/test_serving.py.

mini5's 12 queries score at most 0.096 with these weights, so nothing passes the default 0.1: the runner is built with
threshold 0.02, where the frame of seed 4 has 7 candidates of which the host path keeps 6 (asserted below: at least two poses
kept and at least one suppressed, so the comparison is not vacuous)."""
import functools

import pytest
import torch

from mvgformer_amd.synthetic import build_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THRESHOLD = 0.02
PANOPTIC = "configs/panoptic/knn5-lr4-q1024-g8.yaml"


def _eq(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[:4], b[:4])) and all(torch.equal(x, y) for x, y in zip(a[4], b[4]))


def _clone(o):
    return [t.clone() for t in o[:4]] + [[p.clone() for p in o[4]]]


def test_postprocess_in_the_graph_equals_the_host_path():
    from mvgformer_amd import evaluate as E
    from mvgformer_amd.factory import build_decoder_for_case, case_to_device
    from mvgformer_amd.serving import GraphedDecoder
    cases = [case_to_device(build_case("mini5", seed=s, layers=2, valid_fraction=0.5), DEV) for s in (4, 3)]
    dec = build_decoder_for_case(cases[0], DEV, dtype=torch.bfloat16)
    c = cases[0]
    args = (dec, c.meta, c.spatial_shapes, c.level_start_index)
    plain = GraphedDecoder(*args, batch=1, num_queries=c.NQ, threshold=THRESHOLD)
    post = GraphedDecoder(*args, batch=1, num_queries=c.NQ, threshold=THRESHOLD, postprocess=dict(dist_thr=0.3, num_nearby_joints_thr=7))
    assert plain.detections is None and plain.pred is None and post.postprocess["max_dets"] == -1
    graphs, kept_total, suppressed_total = set(), 0, 0
    for i, c in enumerate(cases * 2):                                   # frames alternate, no re-capture
        for run in (plain, post):
            run.set_cameras(c.meta)
            run.load(src_views=c.src_views, tgt=c.tgt, query_pos=c.query_pos, reference_points=c.reference_points)
        want_out = _clone(plain.replay())
        got_out = post.replay()                                         # the capture itself: no synchronisation inside pose_nms
        graphs.add(id(post.graph))
        torch.cuda.synchronize()
        assert _eq(got_out, want_out), i                                # the same five tensors, bit for bit
        dets, count, keep = post.detections
        assert all(t.data_ptr() in [p.data_ptr() for p in post._pinned] for t in (dets, count, keep, post.post.nms["workspace"]))
        pred = post.pred[0].cpu()
        assert tuple(post.pred.shape) == (1, c.NQ, 15, 5)
        want = E.filter_and_nms(pred.clone())
        k = int(count[0, 0])
        candidates = int((pred[:, 0, 3] >= 0).sum())
        print("frame", i, "candidates", candidates, "host keeps", len(want), "device keeps", k)
        assert k == len(want) and int(count[0, 1]) == 0
        assert torch.equal(dets[0, :k].cpu(), want)
        assert torch.equal(pred[keep[0, :k].cpu().long()], want) and bool((keep[0, k:] == -1).all())
        assert bool((dets[0, k:, :, 3] == -1).all()) and float(dets[0, k:, :, :3].abs().sum()) == 0.0
        if i < 2:
            kept_total += len(want)
            suppressed_total += candidates - len(want)
        # eager() takes the same path as the capture: same outputs, same detections in the same static buffers
        snap = [t.clone() for t in (dets, count, keep)]
        assert _eq(post.eager(), want_out)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(snap, post.detections)) and torch.equal(post.pred.cpu()[0], pred)
    assert len(graphs) == 1
    assert kept_total >= 2 and suppressed_total >= 1, (kept_total, suppressed_total)


def test_postprocess_rejects_unknown_keys():
    from mvgformer_amd.factory import build_decoder_for_case, case_to_device
    from mvgformer_amd.serving import GraphedDecoder
    c = case_to_device(build_case("mini5", seed=4, layers=2, with_features=False), DEV)
    dec = build_decoder_for_case(c, DEV, dtype=torch.bfloat16)
    with pytest.raises(TypeError, match="unknown postprocess keys"):
        GraphedDecoder(dec, c.meta, c.spatial_shapes, c.level_start_index, 1, c.NQ, 0.1, postprocess=dict(threshold=0.3))


@functools.lru_cache(maxsize=None)
def _report(graph, device_nms):
    from mvgformer_amd import validate
    return validate.main(["--cfg", "extract:" + PANOPTIC, "--frames", "2", "--graph", str(graph), "--device-nms", str(device_nms)])


def _comparable(rep, drop=()):
    rows = [{k: v for k, v in r.items() if k not in ("decoder_ms_per_frame",) + tuple(drop)} for r in rep["results"]]
    return {k: v for k, v in rep.items() if k not in ("device_nms", "results")}, rows


@pytest.mark.parametrize("graph", [1, 0])
def test_validate_reports_are_equal_with_and_without_device_nms(graph):
    """the same synthetic frames through validate.main: every field but `device_nms` and the timing is equal; with --graph 1 the
    kept poses come from the graph's static buffers, with --graph 0 from those of a postprocess.PostProcess behind the eager head"""
    host, dev = _report(1, 0), _report(graph, 1)
    assert host["device_nms"] is False and dev["device_nms"] is True
    assert dev["results"][0]["hip_graph"] is bool(graph)
    drop = () if graph else ("hip_graph",)                             # the host report is the --graph 1 one
    assert _comparable(host, drop) == _comparable(dev, drop)
    row = dev["results"][0]
    print(row)
    assert row["frames"] == 2 and 0 <= row["poses_after_nms"] <= row["candidates_above_thr"] <= 2 * 1024
