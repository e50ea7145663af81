"""Validation scoring on the device (csrc/evalacc.hip -> ops.eval_match / ops.eval_pcp -> evaluate.DeviceEvaluator ->
serving.GraphedDecoder(evaluation=...) -> validate --device-eval) against the host functions of mvgformer_amd/evaluate.py.

Inputs: the seeded scenes of tests/golden/eval_cases.py with the seeds of tests/test_evaluate.py, coordinates rounded to fp32
first; the same rounded arrays go to the host reference (filter_and_nms, then match_predictions / evaluate_pcp) and, padded into
(B, R, J, 5) with `count`, to the device (tests/eval_device_cases.py).  Bounds: gt_id, order, score, NaN positions, total_gt and
every integer counter are equal; mpjpe is within 1e-12 relative (the project's bound for another summation order of <= 45 fp64
terms, see evaluate.py); AP / recall / recall@500 are equal to the host's and within 1e-9 of tests/golden/eval.npz.  So that a
tie cannot hide a defect, the host reference of every case is first checked for: best and second-best mean more than 1e-6 mm
apart, no mpjpe within 1e-2 mm of a threshold (25..150, 500), no limb margin below 1e-6 mm.

tests/golden/eval.npz holds the reference's PCP of the classification-filtered candidates WITHOUT the NMS (as
tests/test_evaluate.py feeds them), and the NMS drops rows that change it: the PCP test therefore scores both inputs, the kept
rows against the host tuple and counters, the unfiltered candidates (flag -1 rows between them, count = None) against the
golden file as well."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from mvgformer_amd import evaluate as E
from mvgformer_amd import ops
from mvgformer_amd.synthetic import build_case
from tests import eval_device_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "eval.npz"))
RTOL = 1e-12


def _dev(*tensors):
    return [None if t is None else t.to(DEV) for t in tensors]


def _assert_list(got, want, what=""):
    """entry list against the host's: ids, order, scores and NaN positions equal, mpjpe within RTOL"""
    (g, g_total), (w, w_total) = got, want
    assert g_total == w_total, what
    assert g["gt_id"].dtype == np.int64 and g["mpjpe"].dtype == np.float64 and g["score"].dtype == np.float64
    assert g["gt_id"].tolist() == w["gt_id"].tolist(), what
    assert np.array_equal(g["score"], w["score"]), what
    assert np.array_equal(np.isnan(g["mpjpe"]), np.isnan(w["mpjpe"])), what
    ok = ~np.isnan(w["mpjpe"])
    err = np.abs(g["mpjpe"][ok] - w["mpjpe"][ok]) / np.maximum(np.abs(w["mpjpe"][ok]), 1e-300)
    print(what, "entries", len(w["mpjpe"]), "max relative mpjpe error %.3g" % (err.max() if len(err) else 0.0))
    assert (err <= RTOL).all(), (what, err.max())


def _assert_preconditions(case):
    assert case["best_gap"] > 1e-6 and case["threshold_gap"] > 1e-2, (case["best_gap"], case["threshold_gap"])


def _feed_panoptic(ev, case, R=8, G=6, J=15, filler_flag=0.0):
    """one call per frame, B = 1; the rows behind the count carry flag 0: only `count` keeps them out"""
    for k, g, v in zip(case["kept"], case["gts"], case["vis"]):
        dets, count = C.pad_rows(k, R, J, filler_flag)
        ev.update(*_dev(dets, count, *C.pad_ground_truth(g, v, G, J)))
    return ev


# ---- 1: the Panoptic list and the metrics -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", C.PANOPTIC_SEEDS)
def test_panoptic_list_and_metrics_equal_the_host(seed):
    case = C.panoptic_case(seed)
    _assert_preconditions(case)
    assert len(case["ev"]["mpjpe"]) >= 10 and any(len(g) == 0 for g in case["gts"])       # a frame without ground truth is in it
    ev = _feed_panoptic(E.DeviceEvaluator("panoptic", capacity=64, device=DEV), case)
    _assert_list(ev.eval_list(), (case["ev"], case["total_gt"]), "seed %d" % seed)
    st = ev.state()
    assert st["frames"] == 6 and st["overflow"] == 0 and st["kept_rows"] == sum(len(k) for k in case["kept"])
    assert st["n_entries"] == len(case["ev"]["mpjpe"])
    aps, recs, mpjpe, rec500 = ev.panoptic()
    h_aps, h_recs, h_mpjpe, h_rec500 = case["metrics"]
    assert aps == h_aps and recs == h_recs and rec500 == h_rec500
    assert abs(mpjpe - h_mpjpe) <= RTOL * abs(h_mpjpe)
    gold = GOLD["pan_%d_nms" % seed]
    np.testing.assert_allclose(np.asarray(aps + recs + [rec500]), np.delete(gold, 12), rtol=0, atol=1e-9)
    # reset() empties it
    assert ev.reset().state() == dict.fromkeys(ops.EVAL_STATE, 0) and len(ev.eval_list()[0]["mpjpe"]) == 0


# ---- 2: a batch in one call -------------------------------------------------------------------------------------------------------
def _batch_inputs(case, frames, R, G, J=15):
    """frames of the case as ONE call: the kept rows of every element spread over R rows with flag -1 rows between them"""
    dets = np.zeros((len(frames), R, J, 5), np.float32)
    dets[:, :, :, 3] = -1.0
    j3d, vis, num = [], [], []
    for b, f in enumerate(frames):
        k = case["kept"][f]
        assert 2 * len(k) + 1 <= R
        dets[b, 1:2 * len(k) + 1:2] = k                                  # rows 1, 3, 5, ...: row order is kept
        a, v, n = C.pad_ground_truth(case["gts"][f], case["vis"][f], G, J)
        j3d.append(a), vis.append(v), num.append(n)
    return torch.from_numpy(dets), None, torch.cat(j3d), torch.cat(vis), torch.cat(num)


def test_batch_in_one_call_keeps_the_reference_order():
    case = C.panoptic_case(11)
    _assert_preconditions(case)
    first, second = (0, 1, 2), (3, 4, 5)                                    # frame 2 has no ground truth: skipped entirely
    assert [len(case["gts"][f]) for f in first].count(0) == 1 and len({len(case["gts"][f]) for f in range(6)}) >= 3
    ev = E.DeviceEvaluator("panoptic", capacity=64, device=DEV)
    ev.update(*_dev(*_batch_inputs(case, first, R=13, G=6)))
    want_first = E.match_predictions([case["kept"][f] for f in first], [case["gts"][f] for f in first], [case["vis"][f] for f in first])
    _assert_list(ev.eval_list(), want_first, "first call")
    ev.update(*_dev(*_batch_inputs(case, second, R=13, G=6)))
    _assert_list(ev.eval_list(), (case["ev"], case["total_gt"]), "both calls")
    st = ev.state()
    assert st["frames"] == 6 and st["kept_rows"] == sum(len(k) for k in case["kept"]) and st["total_gt"] == case["total_gt"]
    # an element without ground truth appends nothing but its kept rows are counted: more kept rows than entries
    no_gt = [f for f in range(6) if len(case["gts"][f]) == 0]
    assert st["kept_rows"] - st["n_entries"] == sum(len(case["kept"][f]) for f in no_gt)


# ---- 3: edges ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J", [15, 14])
def test_edges_nan_means_and_smallest_shapes(J):
    case = C.panoptic_case(12, J)
    _assert_preconditions(case)
    f = max(range(6), key=lambda i: (len(case["gts"][i]) >= 2) * len(case["kept"][i]))
    kept, gt, vis = case["kept"][f], case["gts"][f], np.array(case["vis"][f])
    assert len(gt) >= 2 and len(kept) >= 2
    # (a) person 0 has no visible joint: its mean is NaN and ordered last, every row goes to another person
    vis_a = vis.copy()
    vis_a[0] = 0.0
    # (b) a row with a NaN coordinate: every mean is NaN, the host appends NaN with the first person
    kept_b = kept.copy()
    kept_b[1, 3, 0] = np.nan
    # (c) nobody is visible: every mean of every row is NaN
    vis_c = np.zeros_like(vis)
    frames = [(kept, gt, vis_a), (kept_b, gt, vis), (kept, gt, vis_c), (kept[:1], gt[:1], vis[:1])]
    want = E.match_predictions([k for k, _, _ in frames], [g for _, g, _ in frames], [v for _, _, v in frames])
    n = len(kept)
    assert 0 not in (want[0]["gt_id"][:n] - 0).tolist() and not np.isnan(want[0]["mpjpe"][:n]).any()          # (a)
    assert np.isnan(want[0]["mpjpe"][n + 1]) and want[0]["gt_id"][n + 1] == len(gt)                              # (b)
    assert np.isnan(want[0]["mpjpe"][2 * n:3 * n]).all() and set(want[0]["gt_id"][2 * n:3 * n]) == {2 * len(gt)}  # (c)
    ev = E.DeviceEvaluator("panoptic", capacity=64, device=DEV)
    for k, g, v in frames[:3]:
        dets, count = C.pad_rows(k, len(k) + 1, J)
        ev.update(*_dev(dets, count, *C.pad_ground_truth(g, v, len(g), J)))
    k, g, v = frames[3]                                                      # R = 1 and Gmax = 1
    dets, count = C.pad_rows(k, 1, J)
    ev.update(*_dev(dets, count, *C.pad_ground_truth(g, v, 1, J)))
    _assert_list(ev.eval_list(), want, "edges J = %d" % J)


def test_bad_arguments_are_refused():
    from mvgformer_amd import _lib
    b = ops.eval_buffers(4, 2, DEV)
    mk = lambda B=1, R=2, J=15, G=2: _dev(torch.zeros((B, R, J, 5)), None, torch.zeros((B, G, J, 3)), torch.zeros((B, G, J)),
                                         torch.zeros((B,), dtype=torch.int32))
    with pytest.raises(_lib.MvgError, match="mvg_eval_match"):
        ops.eval_match(*mk(J=33), b)
    with pytest.raises(_lib.MvgError, match="mvg_eval_match"):
        ops.eval_match(*mk(G=65), b)
    with pytest.raises(_lib.MvgError, match="mvg_eval_pcp"):
        ops.eval_pcp(*mk(J=15), b)                                          # the PCP limbs are those of the 14-joint format
    with pytest.raises(_lib.MvgError, match="mvg_eval_pcp"):
        ops.eval_pcp(*mk(J=14), b, alpha=float("nan"))
    with pytest.raises(RuntimeError, match="float32"):
        ops.eval_match(torch.zeros((1, 2, 15, 5), dtype=torch.float64, device=DEV), *mk()[1:], b)
    torch.cuda.synchronize()
    assert int(b["state"].abs().sum()) == 0                                 # nothing was launched


# ---- 4: overflow -------------------------------------------------------------------------------------------------------------------
def test_overflow_writes_nothing_past_the_capacity():
    case = C.panoptic_case(11)
    n = len(case["ev"]["mpjpe"])
    cap = n - 5
    ev = E.DeviceEvaluator("panoptic", capacity=cap, device=DEV)
    # deliberately over-allocated arrays: the evaluator sees the first `cap` elements, the memory behind them holds a sentinel
    big = {k: torch.full((n + 8,), -7, dtype=ev.buffers[k].dtype, device=DEV) for k in ("mpjpe", "score", "gt_id")}
    for k, t in big.items():
        ev.buffers[k] = t[:cap]
    _feed_panoptic(ev, case)
    st = ev.state()
    assert st["overflow"] == 1 and st["n_entries"] == n and st["total_gt"] == case["total_gt"]      # it keeps counting
    for k, t in big.items():
        assert bool((t[cap:] == -7).all()), k                                                        # untouched
    assert big["gt_id"][:cap].cpu().tolist() == case["ev"]["gt_id"][:cap].tolist()
    assert np.array_equal(big["score"][:cap].cpu().numpy(), case["ev"]["score"][:cap])
    np.testing.assert_allclose(big["mpjpe"][:cap].cpu().numpy(), case["ev"]["mpjpe"][:cap], rtol=RTOL, atol=0)
    with pytest.raises(RuntimeError, match="capacity >= %d" % n):
        ev.eval_list()
    with pytest.raises(RuntimeError, match="capacity"):
        ev.panoptic()


# ---- 5: PCP ------------------------------------------------------------------------------------------------------------------------
def _feed_pcp(ev, rows_per_frame, actors, R, use_count):
    for f, rows in enumerate(rows_per_frame):
        if use_count:
            dets, count = C.pad_rows(rows, R, 14, filler_flag=0.0)
        else:                                                                # the rows as they are, flag -1 rows among them
            dets, count = C.pad_rows(rows, R, 14)[0], None
        ev.update(*_dev(dets, count, *C.pad_ground_truth_pcp(actors, f)))
    return ev


@pytest.mark.parametrize("seed", C.PCP_SEEDS)
def test_pcp_counters_equal_the_host(seed):
    case = C.pcp_case(seed)
    for k in (case["counters"], case["counters_unfiltered"]):
        assert k["row_gap"] > 1e-6 and k["limb_gap"] > 1e-6 and k["recall_gap"] > 1e-2, k
    assert any(g is None for a in case["actors"] for g in a)                 # an actor that is not annotated in some frame
    assert any((p[:, 0, 3] < 0).any() for p in case["preds"])                # a flag -1 row in the unfiltered input
    for rows, counters, host, use_count in ((case["kept"], case["counters"], case["host"], True),
                                            (case["preds"], case["counters_unfiltered"], case["host_unfiltered"], False)):
        ev = _feed_pcp(E.DeviceEvaluator("pcp", actors=4, device=DEV), rows, case["actors"], R=7, use_count=use_count)
        st = ev.state()
        for key in ("correct", "total", "bone_correct"):
            assert ev.buffers[key].dtype == torch.int64 and np.array_equal(ev.buffers[key].cpu().numpy(), counters[key]), key
        assert st["match_gt"] == counters["match_gt"] and st["total_gt"] == counters["total_gt"] and st["empty_frame"] == 0
        assert st["frames"] == len(rows) and st["kept_rows"] == sum(int((np.asarray(r)[:, 0, 3] >= 0).sum()) for r in rows)
        np.testing.assert_allclose(C.flat_pcp(ev.pcp()), C.flat_pcp(host), rtol=0, atol=0)
    np.testing.assert_allclose(C.flat_pcp(ev.pcp()), GOLD["pcp_%d" % seed], rtol=1e-9, atol=1e-9)   # the unfiltered input


def test_pcp_frame_without_a_prediction_raises_like_the_host():
    case = C.pcp_case(21)
    kept = [k.copy() for k in case["kept"]]
    f = next(i for i in range(1, len(kept)) if any(a[i] is not None for a in case["actors"]))
    kept[f][:, :, 3] = -1.0                                                  # nothing passes the classification filter there
    with pytest.raises(ValueError) as host:
        E.evaluate_pcp(kept, case["actors"])
    ev = _feed_pcp(E.DeviceEvaluator("pcp", actors=4, device=DEV), kept, case["actors"], R=7, use_count=True)
    torch.cuda.synchronize()                                                 # the run went on over the later frames
    assert ev.state()["frames"] == len(kept) and ev.state()["empty_frame"] == f + 1
    with pytest.raises(ValueError) as dev:
        ev.pcp()
    assert str(dev.value) == str(host.value) and ("frame %d " % f) in str(dev.value)
    from mvgformer_amd import validate
    assert validate.pcp_report(None, None, None, ev) == {"error": str(host.value)}


# ---- 6: reproducibility ------------------------------------------------------------------------------------------------------------
def test_two_fresh_evaluators_give_the_same_bits():
    pan, pcp = C.panoptic_case(12), C.pcp_case(22)
    runs = []
    for _ in range(2):
        a = _feed_panoptic(E.DeviceEvaluator("panoptic", capacity=64, device=DEV), pan)
        b = _feed_pcp(E.DeviceEvaluator("pcp", actors=4, device=DEV), pcp["kept"], pcp["actors"], R=7, use_count=True)
        runs.append([t.clone() for ev in (a, b) for t in ev.buffers.values()])
    assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(*runs))
    assert int(runs[0][2].abs().sum()) > 0


# ---- 7: in the graph ---------------------------------------------------------------------------------------------------------------
THRESHOLD = 0.02                     # mini5 as in tests/test_serving_nms_gpu.py: at 0.1 nothing is a candidate


def _mini5_ground_truth(seed, persons):
    rng = np.random.default_rng(seed)
    from tests.golden.eval_cases import _person
    gt = C.round32(np.stack([_person(rng) for _ in range(persons)]))
    vis = (rng.uniform(size=(persons, 15)) > 0.2).astype(np.float64)
    vis[:, 0] = 1.0
    return gt, vis[..., None]


def _sync_debug(mode):
    """torch.cuda.set_sync_debug_mode, False where this build refuses it"""
    try:
        torch.cuda.set_sync_debug_mode(mode)
        return True
    except Exception as e:           # noqa: BLE001
        print("set_sync_debug_mode is not usable here:", e)
        return False


def test_evaluation_in_the_graph_equals_the_host_list():
    """One graph for all frames, decoder outputs bit-equal to a runner without `evaluation`, the evaluator's list equal to
    match_predictions on the cloned dets[:k] of every frame, eager() the same.  The load-ground-truth + replay region and the
    evaluator's update run under torch.cuda.set_sync_debug_mode("error") where this torch build accepts the call (torch 2.10 for
    ROCm 7 does; the test prints what it found)."""
    from mvgformer_amd.factory import build_decoder_for_case, case_to_device
    from mvgformer_amd.serving import GraphedDecoder
    from tests.test_serving_nms_gpu import _clone, _eq
    cases = [case_to_device(build_case("mini5", seed=s, layers=2, valid_fraction=0.5), DEV) for s in (4, 3)]
    gts = [_mini5_ground_truth(1, 2), _mini5_ground_truth(2, 3)]
    gts_dev = [_dev(*C.pad_ground_truth(g, v, 3, 15)) for g, v in gts]
    dec = build_decoder_for_case(cases[0], DEV, dtype=torch.bfloat16)
    c = cases[0]
    args = (dec, c.meta, c.spatial_shapes, c.level_start_index)
    pp = dict(dist_thr=0.3, num_nearby_joints_thr=7)
    plain = GraphedDecoder(*args, batch=1, num_queries=c.NQ, threshold=THRESHOLD, postprocess=pp)
    post = GraphedDecoder(*args, batch=1, num_queries=c.NQ, threshold=THRESHOLD, postprocess=pp,
                          evaluation=dict(kind="panoptic", capacity=64, max_persons=4))
    assert plain.evaluator is None and post.evaluator.kind == "panoptic" and tuple(post.ground_truth[0].shape) == (1, 4, 15, 3)
    graphs, kept, want_gt, want_vis = set(), [], [], []
    for i, c in enumerate(cases * 2):                                        # frames alternate, no re-capture
        for run in (plain, post):
            run.set_cameras(c.meta)
            run.load(src_views=c.src_views, tgt=c.tgt, query_pos=c.query_pos, reference_points=c.reference_points)
        if post.graph is None:
            post.load(ground_truth=gts_dev[1]).capture()                    # the warm-up forwards score nothing
            torch.cuda.synchronize()
            assert post.evaluator.state() == dict.fromkeys(ops.EVAL_STATE, 0)
        want_out = _clone(plain.replay())
        torch.cuda.synchronize()
        checked = _sync_debug("error")
        try:
            got_out = post.load(ground_truth=gts_dev[i % 2]).replay()       # no host synchronisation in here
        finally:
            _sync_debug("default")
        print("frame", i, "replay under sync debug mode 'error':", checked)
        graphs.add(id(post.graph))
        torch.cuda.synchronize()
        assert _eq(got_out, want_out), i
        dets, count, _ = post.detections
        assert torch.equal(dets, plain.detections[0]) and torch.equal(count, plain.detections[1])
        kept.append(dets[0, :int(count[0, 0])].clone().cpu().numpy())
        want_gt.append(gts[i % 2][0]), want_vis.append(gts[i % 2][1])
        assert all(t.data_ptr() in [p.data_ptr() for p in post._pinned] for t in list(post.evaluator.buffers.values()) + list(post.ground_truth))
    assert len(graphs) == 1
    want = E.match_predictions(kept, want_gt, want_vis)
    for k, g, v in zip(kept, want_gt, want_vis):                             # the tie precondition on the host reference
        m = np.sort(C.mean_matrix(k.astype(np.float64), g, v), axis=1)
        assert len(k) == 0 or float((m[:, 1] - m[:, 0]).min()) > 1e-6
    assert len(want[0]["mpjpe"]) >= 4 and want[1] == 10
    got = post.evaluator.eval_list()
    _assert_list(got, want, "graph")
    st = post.evaluator.state()
    assert st["frames"] == 4 and st["kept_rows"] == sum(len(k) for k in kept)
    # eager() takes the same path: the same list, bit for bit
    post.evaluator.reset()
    for i, c in enumerate(cases * 2):
        post.set_cameras(c.meta)
        post.load(src_views=c.src_views, tgt=c.tgt, query_pos=c.query_pos, reference_points=c.reference_points, ground_truth=gts_dev[i % 2])
        post.eager()
    again = post.evaluator.eval_list()
    assert again[1] == got[1] and all(np.array_equal(again[0][k], got[0][k], equal_nan=k == "mpjpe") for k in got[0])
    # DeviceEvaluator.update on its own, under the same mode
    ev = E.DeviceEvaluator("panoptic", capacity=64, max_persons=4, device=DEV)
    dets, count = _dev(*C.pad_rows(kept[0], 8, 15))
    torch.cuda.synchronize()
    checked = _sync_debug("error")
    try:
        ev.update(dets, count, *gts_dev[0])
    finally:
        _sync_debug("default")
    print("update under sync debug mode 'error':", checked)
    _assert_list(ev.eval_list(), E.match_predictions(kept[:1], want_gt[:1], want_vis[:1]), "update alone")


def test_evaluation_needs_postprocess_and_known_keys():
    from mvgformer_amd.factory import build_decoder_for_case, case_to_device
    from mvgformer_amd.serving import GraphedDecoder
    c = case_to_device(build_case("mini5", seed=4, layers=2, with_features=False), DEV)
    dec = build_decoder_for_case(c, DEV, dtype=torch.bfloat16)
    args = (dec, c.meta, c.spatial_shapes, c.level_start_index, 1, c.NQ, 0.1)
    with pytest.raises(ValueError, match="requires postprocess"):
        GraphedDecoder(*args, evaluation=dict(kind="panoptic"))
    with pytest.raises(TypeError, match="unknown evaluation keys"):
        GraphedDecoder(*args, postprocess=dict(), evaluation=dict(kind="panoptic", threshold=25))
    with pytest.raises(ValueError, match="kind"):
        GraphedDecoder(*args, postprocess=dict(), evaluation=dict(kind="coco"))
    with pytest.raises(ValueError, match="evaluation"):
        GraphedDecoder(*args, postprocess=dict()).load(ground_truth=(None, None, None))


# ---- 8: validate.main --------------------------------------------------------------------------------------------------------------
YAMLS = {"panoptic": "configs/panoptic/knn5-lr4-q1024-g8.yaml", "shelf": "configs/shelf_campus/shelf_knn5-lr4-q1024.yaml"}


@functools.lru_cache(maxsize=None)
def _validate_rig(dataset, tmp):
    """a small configuration of the dataset's YAML (128 queries, 2 layers, 3 views of 320 x 192), two synthetic frames as a
    --frames-npz file, ground truth = kept poses of a first run moved a little, and the host report (--device-eval 0)"""
    import yaml
    from mvgformer_amd import validate
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "mvgformer_amd", "data", "yaml_extract.json")) as f:
        val = json.load(f)[YAMLS[dataset]]
    raw = {"DECODER": dict(val["DECODER"], num_instance=128, num_decoder_layers=2), "NETWORK": {"IMAGE_SIZE": [320, 192]},
           "MULTI_PERSON": {"SPACE_SIZE": val["SPACE_SIZE"], "SPACE_CENTER": val["SPACE_CENTER"]}, "DATASET": {"CAMERA_NUM": 3}}
    os.makedirs(tmp, exist_ok=True)
    cfg_path, npz, out = os.path.join(tmp, "small.yaml"), os.path.join(tmp, "frames.npz"), os.path.join(tmp, "pred")

    def write_cfg():
        with open(cfg_path, "w") as f:
            yaml.safe_dump(raw, f)
    write_cfg()
    frames = list(validate.synthetic_frames(validate.load_config(cfg_path), 2, seed=5))
    arrays = {}
    for l in range(len(frames[0][0])):
        arrays["feat%d" % l] = np.stack([fr[0][l].numpy() for fr in frames])
    for k in ("R", "T", "fx", "fy", "cx", "cy", "k", "p"):
        arrays["camera_" + k] = np.stack([np.stack([m["camera"][k][0].numpy() for m in fr[1]]) for fr in frames])
    for k in ("center", "scale", "inv_affine_trans"):
        arrays[k] = np.stack([np.stack([m[k][0].numpy() for m in fr[1]]) for fr in frames])
    np.savez(npz, **arrays)
    args = ["--cfg", cfg_path, "--frames-npz", npz, "--dtype", "fp32"]
    validate.main(args + ["--pred-out", out])
    pred = np.load("%s-%s.npy" % (out, raw["DECODER"]["inference_conf_thr"][0]))
    if dataset == "panoptic":        # untrained weights: put the threshold where about a quarter of the queries are candidates
        raw["DECODER"]["inference_conf_thr"] = [float(np.quantile(pred[:, :, 0, 4], 0.75))]
        write_cfg()
        pred[:, :, :, 3] = (pred[:, :, :, 4] > raw["DECODER"]["inference_conf_thr"][0]) - 1.0
    kept = [E.filter_and_nms(torch.from_numpy(p)).numpy() for p in pred]
    G = min(3, min(len(k) for k in kept))
    assert G >= 2, [len(k) for k in kept]
    J = pred.shape[2]
    rs = np.random.RandomState(0)
    gt = np.stack([k[:G, :, :3] + rs.standard_normal((G, J, 3)) * 15.0 for k in kept]).astype(np.float32)
    vis = np.ones((2, G, J, 3), np.float32)
    vis[1, G - 1] = 0                # shelf: the last actor is not annotated in frame 1; panoptic: a person without visible joint
    vis[0, 0, 2:5] = 0
    np.savez(npz, joints_3d=gt, joints_3d_vis=vis, **arrays)
    return args, validate.main(args + ["--device-nms", "1"])


@pytest.mark.parametrize("graph", [1, 0])
@pytest.mark.parametrize("dataset", ["panoptic", "shelf"])
def test_validate_reports_are_equal_with_and_without_device_eval(dataset, graph, tmp_path_factory):
    from mvgformer_amd import validate
    args, host = _validate_rig(dataset, str(tmp_path_factory.getbasetemp() / ("eval_" + dataset)))
    dev = validate.main(args + ["--device-nms", "1", "--device-eval", "1", "--graph", str(graph)])
    assert host["device_eval"] is False and dev["device_eval"] is True and dev["results"][0]["hip_graph"] is bool(graph)
    drop = lambda rep: ({k: v for k, v in rep.items() if k not in ("device_eval", "results")},
                        [{k: v for k, v in r.items() if k not in ("decoder_ms_per_frame",) + (() if graph else ("hip_graph",))}
                         for r in rep["results"]])
    print(dev["results"][0])
    assert drop(host) == drop(dev)
    row = dev["results"][0]
    assert row["frames"] == 2 and 4 <= row["poses_after_nms"] <= row["candidates_above_thr"]
    if dataset == "shelf":
        assert row["PCP"]["recall500"] > 99 and len(row["PCP"]["actor"]) >= 2 and "AP" not in row
    else:
        assert row["recall500"] > 60 and row["MPJPE"] < 50 and row["AP"]["150"] > 0 and "PCP" not in row
