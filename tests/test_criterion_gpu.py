"""GPU checks of the fused training criterion (csrc/criterion.hip): mvg_knn_match and mvg_criterion against the reference's
fixture (tests/golden/criterion.npz) and the fp64 restatement tests/criterion_ref.py.

Tolerance of a loss / a gradient tensor: 4 x the reference's own fp32-against-fp64 error stored in the fixture, floored at 1e-6
relative (gradients: max abs error over max abs value).  The reference's fp32 errors are 5e-9 .. 5e-7, so nearly every bar is the
1e-6 floor.  Measured on MI355X, maximum over all fixture cases, the empty-element case and all layers: loss_ce 2.7e-8,
loss_pose_perjoint 4.7e-8, loss_pose_perprojection_2d 6.1e-8 relative (the crop affine is an fp32 record); grad_logits 5.3e-8,
grad_poses 2.4e-8, grad_poses_2d 2.4e-8 (the fp32 rounding of the stored gradient).  Metrics are counts and compare equal after
rounding to fp32.
"""
import os

import numpy as np
import pytest
import torch

from tests import criterion_ref as R
from tests.golden import criterion_cases as cc
from tests.test_criterion_cpu import FIX, restate

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cfg(NQ):
    from types import SimpleNamespace as NS
    return NS(MULTI_PERSON=NS(SPACE_SIZE=list(cc.SPACE_SIZE), SPACE_CENTER=list(cc.SPACE_CENTER)), NETWORK=NS(IMAGE_SIZE=list(cc.IMG_WH)),
              DECODER=NS(pred_conf_threshold=cc.PRED_CONF_THRESHOLD, num_instance=NQ))


def _criterion(name):
    from mvgformer_amd.criterion import KNNMatcher, SetCriterion
    c = cc.EMPTY_CASE if name == "empty" else cc.CASES[name]
    m = KNNMatcher("abs", "norm", cost_class=2.0, cost_pose=5.0, method=c["method"], method_value=c["value"])
    return SetCriterion(2, m, {}, ["joints", "labels", "cardinality"], _cfg(c["NQ"]))


def _device_case(name):
    from mvgformer_amd import ops
    inp = cc.make_inputs(name)
    meta = cc.make_meta(inp, DEV)
    t = {k: torch.from_numpy(inp[k]).to(DEV) for k in ("init_poses", "logits", "poses", "poses_2d")}
    cams = ops.pack_cameras(meta, list(cc.IMG_WH), DEV)
    return inp, meta, t, cams


def _fused(name, decay="none"):
    """pairs, table (L, 8), the three gradients of sum(loss_ce + loss_pose_perjoint + loss_pose_perprojection_2d over layers)"""
    from mvgformer_amd.criterion import criterion_all_layers
    inp, meta, t, cams = _device_case(name)
    crit = _criterion(name)
    lg, ps, p2 = (t[k].clone().requires_grad_(True) for k in ("logits", "poses", "poses_2d"))
    ld, pairs = criterion_all_layers(crit, lg, ps, p2, meta, t["init_poses"], decay, cams)
    (ld["loss_ce"] + ld["loss_pose_perjoint"] + ld["loss_pose_perprojection_2d"]).backward()
    rows = torch.stack([torch.stack([d[k] for k in R.KEYS]) for d in ld["dict_losses_layers"]]).detach()
    return pairs, rows, (lg.grad, ps.grad, p2.grad), ld


def _pairs_per_person(pq, pg, pc, b):
    n = int(pc[b])
    q, g = pq[b, :n].tolist(), pg[b, :n].tolist()
    return q, g


@pytest.mark.parametrize("name", list(cc.CASES))
def test_knn_match_equals_the_fixture(name):
    pairs, _, _, _ = _fused(name)
    pq, pg, pc, matched = (x.cpu() for x in pairs)
    for b in range(cc.CASES[name]["B"]):
        q, g = _pairs_per_person(pq, pg, pc, b)
        assert q == FIX["%s/pairs/%d/query" % (name, b)].tolist() and g == FIX["%s/pairs/%d/gt" % (name, b)].tolist(), (name, b)
        union = torch.zeros(cc.CASES[name]["NQ"], dtype=torch.uint8)
        union[torch.tensor(q, dtype=torch.long)] = 1
        assert torch.equal(matched[b], union)
        assert torch.all(pq[b, int(pc[b]):] == -1)


@pytest.mark.parametrize("NQ,Gmax,nump,K", [(1024, 10, [10, 7], 5), (1024, 10, [1, 0], 1), (1024, 10, [4, 10], 3), (1024, 10, [10, 3], 16),
                                            (1024, 64, [64, 37], 5), (200, 64, [64, 0], 16)])
def test_knn_match_random_cases_against_the_restatement(NQ, Gmax, nump, K):
    from mvgformer_amd import ops
    g = torch.Generator().manual_seed(NQ + Gmax + K)
    B, J = len(nump), 15
    size, cen = torch.tensor(cc.SPACE_SIZE, dtype=torch.float64), torch.tensor(cc.SPACE_CENTER, dtype=torch.float64)
    poses = ((torch.rand((B, NQ, 1, 3), generator=g, dtype=torch.float64) - 0.5) * size + cen
             + torch.randn((B, NQ, J, 3), generator=g, dtype=torch.float64) * 200).float().reshape(B, NQ * J, 3)
    gt = ((torch.rand((B, Gmax, 1, 3), generator=g, dtype=torch.float64) - 0.5) * size * 0.8 + cen
          + torch.randn((B, Gmax, J, 3), generator=g, dtype=torch.float64) * 200).float()
    num = torch.tensor(nump, dtype=torch.int32)
    pq, pg, pc, matched = (x.cpu() for x in ops.knn_match(poses.to(DEV), gt.to(DEV), num.to(DEV), cc.SPACE_SIZE, cc.SPACE_CENTER, "KNN", K))
    C = R.costs(poses.double(), gt.double(), size, cen)
    want = R.match(poses.double(), gt.double(), num, size, cen, "KNN", K)
    assert pc.tolist() == [n * K for n in nump]
    for b in range(B):
        q, gg = _pairs_per_person(pq, pg, pc, b)
        assert gg == want[b][1].tolist()
        for person in range(nump[b]):
            mine, ref = q[person * K:(person + 1) * K], want[b][0][person * K:(person + 1) * K].tolist()
            assert set(mine) == set(ref), (b, person)
            col = C[b, :, person]
            gaps = (col[ref][1:] - col[ref][:-1]).abs()
            if K == 1 or float(gaps.min()) > 1e-3:           # costs ~1e2 .. 1e3: fp32 rounding of the sum ~1e-4
                assert mine == ref, (b, person)
        union = torch.zeros(NQ, dtype=torch.uint8)
        union[torch.tensor(q, dtype=torch.long)] = 1
        assert torch.equal(matched[b], union)


def test_knn_match_without_persons_and_bad_arguments():
    from mvgformer_amd import _lib, ops
    poses = torch.randn((2, 32 * 15, 3), device=DEV) * 1000
    gt = torch.randn((2, 3, 15, 3), device=DEV) * 1000
    zero = torch.zeros(2, dtype=torch.int64, device=DEV)
    pq, pg, pc, matched = ops.knn_match(poses, gt, zero, cc.SPACE_SIZE, cc.SPACE_CENTER, "KNN", 5)
    assert pc.tolist() == [0, 0] and int(matched.sum()) == 0 and bool((pq == -1).all())

    def bad(**kw):
        a = dict(poses=poses, gt=gt, num=zero, K=5, method="KNN")
        a.update(kw)
        with pytest.raises(_lib.MvgError, match="10001"):
            ops.knn_match(a["poses"], a["gt"], a["num"], cc.SPACE_SIZE, cc.SPACE_CENTER, a["method"], a["K"])
    bad(gt=torch.zeros((2, 65, 15, 3), device=DEV))                                     # Gmax > 64
    bad(K=17)                                                                           # K > 16
    bad(poses=poses[:, :4 * 15], K=5)                                                   # K > NQ
    bad(poses=torch.zeros((2, 2 * 65, 3), device=DEV), gt=torch.zeros((2, 3, 65, 3), device=DEV), K=1)   # J > 64
    bad(K=0)
    bad(method="multiple", K=-1.0)                                                      # threshold <= 0


def _bars(name):
    f32, f64 = FIX[name + "/table/f32"].astype(np.float64), FIX[name + "/table/f64"]
    ref_err = np.abs(f32 - f64) / np.maximum(np.abs(f64), 1e-30)
    return np.maximum(4 * ref_err, 1e-6)


@pytest.mark.parametrize("name", list(cc.CASES) + ["empty"])
def test_losses_metrics_and_gradients_against_the_fp64_restatement(name):
    _, want, wgrads = restate(name)
    _, got, grads, _ = _fused(name)
    got, want = got.cpu().double().numpy(), want.numpy()
    bars = _bars(name) if name in cc.CASES else np.full(want.shape, 1e-6)
    for i, k in enumerate(R.KEYS):
        if k in R.METRICS:
            print(name, k, got[:, i], want[:, i])
            assert np.array_equal(got[:, i].astype(np.float32), want[:, i].astype(np.float32)), (name, k, got[:, i], want[:, i])
        else:
            err = np.abs(got[:, i] - want[:, i]) / np.maximum(np.abs(want[:, i]), 1e-30)
            err = np.where(want[:, i] == 0, np.abs(got[:, i]), err)
            print(name, k, "rel err", err, "bar", bars[:, i])
            assert np.all(err <= bars[:, i]), (name, k, err, bars[:, i])
    for key, g, w in zip(("grad_logits", "grad_poses", "grad_poses_2d"), grads, wgrads):
        bar = 1e-6
        if name in cc.CASES:
            f32, f64 = FIX["%s/%s/f32" % (name, key)].astype(np.float64), FIX["%s/%s/f64" % (name, key)]
            bar = max(4 * np.abs(f32 - f64).max() / max(np.abs(f64).max(), 1e-30), 1e-6)
        scale = float(w.abs().max())
        err = float((g.cpu().double() - w).abs().max()) / max(scale, 1e-30) if scale > 0 else float(g.abs().max())
        print(name, key, "err", err, "bar", bar)
        assert err <= bar, (name, key, err, bar)


def test_shared_query_gets_the_summed_gradient_and_the_guard_zeroes_the_2d_gradient():
    pairs, _, grads, _ = _fused("b2")
    pq, pg, pc, _ = (x.cpu() for x in pairs)
    q0, g0 = _pairs_per_person(pq, pg, pc, 0)
    shared = [q for q in set(q0) if q0.count(q) > 1]
    assert shared, "case b2 must hold a query among the K nearest of two persons"
    _, _, wgrads = restate("b2")
    J = cc.J
    rows = slice(shared[0] * J, (shared[0] + 1) * J)
    got, want = grads[1][:, 0, rows].cpu().double(), wgrads[1][:, 0, rows]
    single = 1.0 / float(sum(cc.CASES["b2"]["num_person"])) / (J * 3)                   # |gradient| of one pair's term
    assert float(want.abs().max()) > 1.5 * single                                       # two terms add up somewhere
    assert float((got - want).abs().max()) <= 1e-6 * float(want.abs().max())
    _, table, g, ld = _fused("guard")
    assert float(g[2].abs().max()) == 0.0 and bool((table[:, 6] == 0).all())
    assert float(g[1].abs().max()) > 0 and float(g[0].abs().max()) > 0


def test_two_runs_are_bit_identical():
    for name in ("vis", "q1024"):
        a, b = _fused(name), _fused(name)
        assert torch.equal(a[1], b[1])
        for x, y in zip(a[2], b[2]):
            assert torch.equal(x, y)
        for x, y in zip(a[0], b[0]):
            assert torch.equal(x, y)


def _device_kernels(fn):
    """names of every device activity (kernels, copies, memsets) enqueued while fn() runs, from the profiler"""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == DeviceType.CUDA]


@pytest.mark.parametrize("L", [4, 6])
def test_no_host_synchronisation_and_launch_counts(L):
    """match + criterion forward + backward under sync debug mode 'error'; then the device activities of the two library calls as the
    profiler sees them: exactly one kernel for the match and three for the criterion (no memset, no copy), at L = 4 and L = 6."""
    from mvgformer_amd import ops
    from mvgformer_amd.criterion import criterion_all_layers
    inp, meta, t, cams = _device_case("b2")
    crit = _criterion("b2")
    rep = lambda x: x[:1].expand(L, *x.shape[1:]).clone().requires_grad_(True)     # noqa: E731
    lg, ps, p2 = rep(t["logits"]), rep(t["poses"]), rep(t["poses_2d"])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ld, _ = criterion_all_layers(crit, lg, ps, p2, meta, t["init_poses"], "linear", cams)
        (ld["loss_ce"] + ld["loss_pose_perjoint"] + ld["loss_pose_perprojection_2d"]).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(ld["dict_losses_layers"]) == L and torch.isfinite(lg.grad).all()

    m0 = meta[0]
    vis2d = torch.stack([m["joints_vis"] for m in meta]).float()
    box = (cc.SPACE_SIZE, cc.SPACE_CENTER)
    holder = {}

    def run_match():
        holder["pairs"] = ops.knn_match(t["init_poses"], m0["joints_3d"], m0["num_person"], *box, "KNN", 5)

    def run_criterion():
        pq, pg, pc, _ = holder["pairs"]
        ops.criterion(lg.detach(), ps.detach(), p2.detach(), pq, pg, pc, m0["joints_3d"], m0["joints_3d_vis"], vis2d, m0["num_person"],
                      cams, *box, cc.PRED_CONF_THRESHOLD)
    match_events = _device_kernels(run_match)
    crit_events = _device_kernels(run_criterion)
    print("match:", match_events, "criterion:", crit_events)
    assert len(match_events) == 1 and "knn_match_kernel" in match_events[0], match_events
    assert len(crit_events) == 3 and all("crit_" in n for n in crit_events), crit_events


@pytest.mark.parametrize("decay", ["none", "linear", "exp", "last"])
def test_summed_dict_applies_the_decay_weights_on_the_device(decay):
    """the step's dict against the restatement: loss keys = sum_l w_l * layer loss, metric keys = mean over layers, loss_init = 0;
    and the gradients are the layer gradients scaled by w_l"""
    name = "vis"
    _, want, wgrads = restate(name)
    _, rows, grads, ld = _fused(name, decay)
    w = R.layer_weights(decay, want.shape[0]).double()
    for i, k in enumerate(R.KEYS):
        ref = float(want[:, i].mean()) if k in R.METRICS else float((w * want[:, i]).sum())
        got = float(ld[k])
        assert abs(got - ref) <= 2e-6 * max(abs(ref), 1e-30) + (1e-30 if ref else 1e-12), (decay, k, got, ref)
    assert ld["loss_init"].shape == (1,) and float(ld["loss_init"]) == 0.0
    for g, wg in zip(grads, wgrads):
        ref = wg * w.view(-1, *([1] * (wg.dim() - 1)))
        scale = float(wg.abs().max())
        assert float((g.cpu().double() - ref).abs().max()) <= 1e-6 * scale, decay


def test_graph_capture_and_replay_on_new_ground_truth():
    from mvgformer_amd.criterion import criterion_all_layers
    inp, meta, t, cams = _device_case("b2")
    other = cc.make_inputs("vis")                                                       # same B / Gmax / J: another ground truth
    crit = _criterion("b2")
    lg, ps, p2 = (t[k].clone().requires_grad_(True) for k in ("logits", "poses", "poses_2d"))

    def step():
        ld, _ = criterion_all_layers(crit, lg, ps, p2, meta, t["init_poses"], "none", cams)
        total = ld["loss_ce"] + ld["loss_pose_perjoint"] + ld["loss_pose_perprojection_2d"]
        return (total,) + torch.autograd.grad(total, [lg, ps, p2])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                                                          # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    meta[0]["joints_3d"].copy_(torch.from_numpy(other["joints_3d"]))
    meta[0]["joints_3d_vis"].copy_(torch.from_numpy(other["joints_3d_vis"]))
    graph.replay()
    torch.cuda.synchronize()
    replayed = [x.clone() for x in captured]
    eager = step()
    for a, b in zip(replayed, eager):
        assert torch.equal(a, b)


def _mask_case():
    from mvgformer_amd.factory import build_decoder_for_case, case_to_device
    from mvgformer_amd.synthetic import build_case
    from tests.golden.cases import LAYER_CASES
    spec = LAYER_CASES["mini5_half"]
    case = build_case(spec["config"], B=spec.get("B", 1), seed=spec["seed"], NQ=spec.get("NQ"), layers=spec.get("layers", 1),
                      valid_fraction=spec.get("valid_fraction"))
    return build_decoder_for_case(case, DEV), case_to_device(case, DEV), case


@pytest.mark.parametrize("train", [False, True])
def test_indices_as_a_mask_tensor_equal_the_list_of_index_tensors(train):
    dec, gc, case = _mask_case()
    layer = dec.layers[0]
    layer.eval()
    B, NQ = gc.tgt.shape[0], gc.tgt.shape[1] // 15
    g = torch.Generator().manual_seed(5)
    mask = (torch.rand((B, NQ), generator=g) < 0.3)
    mask[:, 1] = True
    idx = [torch.nonzero(mask[b]).flatten().to(DEV) for b in range(B)]
    outs = []
    for indices in (idx, mask.to(DEV).to(torch.uint8), mask.to(DEV)):
        tgt = gc.tgt.clone().requires_grad_(train)
        with torch.set_grad_enabled(train):
            out = layer(tgt, gc.query_pos, gc.reference_points[:, :, None], gc.src_views, gc.spatial_shapes, gc.level_start_index,
                        gc.meta, indices=indices, threshold=0.1)
        outs.append([o.detach().clone() for o in out if torch.is_tensor(o)])
    for other in outs[1:]:
        assert len(other) == len(outs[0]) and all(torch.equal(a, b) for a, b in zip(outs[0], other))
    with pytest.raises(RuntimeError, match="indices as a tensor"):
        layer(gc.tgt, gc.query_pos, gc.reference_points[:, :, None], gc.src_views, gc.spatial_shapes, gc.level_start_index,
              gc.meta, indices=torch.zeros((B, NQ + 1), dtype=torch.uint8, device=DEV), threshold=0.1)


def test_set_criterion_and_matcher_have_the_reference_interface():
    from mvgformer_amd.criterion import total_loss
    inp, meta, t, cams = _device_case("b1")
    crit = _criterion("b1")
    origin = {"pred_logits": torch.ones((1, 128, 2), device=DEV), "pred_poses": {"outputs_coord": t["init_poses"]}}
    out = {"pred_logits": t["logits"][1].clone().requires_grad_(True), "pred_poses": {"outputs_coord": t["poses"][1]},
           "pred_poses_2d": {"outputs_coord_2d": t["poses_2d"][1]}}
    losses, indices = crit(out, meta, origin)
    assert set(losses) == set(R.KEYS)
    assert indices[0][0].dtype == torch.int64 and indices[0][0].is_cuda
    assert indices[0][0].tolist() == FIX["b1/pairs/0/query"].tolist() and indices[0][1].tolist() == FIX["b1/pairs/0/gt"].tolist()
    want = FIX["b1/table/f64"][1]
    got = np.array([float(losses[k]) for k in R.KEYS])
    assert np.all(np.abs(got - want) <= 1e-6 * np.abs(want) + 1e-6)
    total_loss(losses, {"loss_ce": 2.0, "loss_pose_perjoint": 5.0}).backward()
    assert float(out["pred_logits"].grad.abs().max()) > 0
    assert [tuple(map(lambda x: x.tolist(), p)) for p in crit.matcher(origin, meta)] == [tuple(map(lambda x: x.tolist(), p)) for p in indices]
    meta[1]["padding"] = True
    with pytest.raises(NotImplementedError, match="padding"):
        crit(out, meta, origin)


@pytest.mark.parametrize("tdt", [torch.float32, torch.bfloat16])
def test_forward_train_end_to_end(tdt):
    """DecoderHead.forward_train on a 5-view, NQ = 128, 2-layer synthetic case: the reference's keys, finite gradients on every
    decoder parameter the training-step probe reports, and losses equal to the restatement applied to the same decoder outputs."""
    from types import SimpleNamespace as NS
    from mvgformer_amd.caller import DecoderHead, sample_space_reference_points, total_loss
    from mvgformer_amd.factory import build_criterion_from_cfg, build_decoder_for_case, case_to_device
    from mvgformer_amd.synthetic import add_ground_truth, build_case
    case = build_case("mini5", seed=4, NQ=128, layers=2)
    dec = build_decoder_for_case(case, DEV, torch.float32)
    dec.set_training_dtype(tdt)
    g = add_ground_truth(case_to_device(case, DEV), [3], Gmax=4, seed=1)
    cfg = NS(DECODER=NS(match_method="KNN", match_method_value=5, decay_method="linear"), NETWORK=NS(IMAGE_SIZE=list(case.img_size)),
             MULTI_PERSON=NS(SPACE_SIZE=list(case.space_size), SPACE_CENTER=list(case.space_center)))
    criterion, weight_dict, decay = build_criterion_from_cfg(cfg)
    assert weight_dict == {"loss_ce": 2.0, "loss_pose_perjoint": 5.0, "loss_pose_perprojection_2d": 5.0, "loss_init": 0.0}
    torch.manual_seed(0)
    head = DecoderHead(dec, case.NQ, 15, 256, case.space_size, case.space_center).to(DEV).set_criterion(criterion, decay)
    head.train()
    for p in head.parameters():
        p.requires_grad_(True)
    # the parameters tools/train_step_probe.py reports: those its default step (made-up loss on the decoder's outputs) reaches
    dec_params = dict(dec.named_parameters())
    o = dec(g.tgt, g.reference_points, g.src_views, g.meta, g.spatial_shapes, g.level_start_index, None, query_pos=g.query_pos,
            threshold=0.1)
    (o[0].float().pow(2).mean() + 1e-6 * o[1].float().pow(2).mean() + sum(c.float().sum() for c in o[4]) * 1e-3).backward()
    reported = [n for n, p in dec_params.items() if p.grad is not None]
    assert len(reported) >= 50, len(reported)
    for p in head.parameters():
        p.grad = None
    out, ld = head.forward_train(g.src_views, g.meta, g.spatial_shapes, g.level_start_index, threshold=0.1)
    assert set(ld) == set(R.KEYS) | {"dict_losses_layers", "loss_init"}
    assert len(ld["dict_losses_layers"]) == 2 and set(ld["dict_losses_layers"][0]) == set(R.KEYS)
    assert set(out) >= {"pred_logits", "pred_poses", "pred_poses_2d", "pred_poses_2d_proj"}
    total = total_loss(ld, weight_dict)
    total.backward()
    assert torch.isfinite(total)
    missing = [n for n in reported if dec_params[n].grad is None or not bool(torch.isfinite(dec_params[n].grad).all())]
    assert not missing, missing
    assert head.joint_embedding.weight.grad is not None and bool(torch.isfinite(head.instance_embedding.weight.grad).all())

    # the restatement (fp64) on the same decoder outputs
    f64 = torch.float64
    size, cen = torch.tensor(case.space_size, dtype=f64), torch.tensor(case.space_center, dtype=f64)
    ref = sample_space_reference_points(case.NQ, case.space_size, case.space_center, case.B, "cpu").double()
    m0 = g.meta[0]
    gt, vis3, nump = m0["joints_3d"].cpu().double(), m0["joints_3d_vis"].cpu().double(), m0["num_person"].cpu()
    vis2 = torch.stack([m["joints_vis"] for m in g.meta]).cpu().double()
    pairs = R.match(ref, gt, nump, size, cen, "KNN", 5)
    cam = {k: torch.stack([m["camera"][k] for m in g.meta]).cpu().double() for k in ("R", "T", "fx", "fy", "cx", "cy", "k", "p")}
    from mvgformer_amd.synthetic import crop_affine
    aff = torch.from_numpy(crop_affine(m0["center"][0].cpu().numpy(), m0["scale"][0].cpu().numpy(), case.img_size)).double()
    logits = torch.stack(out["all_logits"]).detach().cpu().double()
    poses = torch.stack([c["outputs_coord"] for c in out["all_poses"]]).detach().cpu().double()
    poses2d = torch.stack([c["outputs_coord_2d"] for c in out["all_poses_2d"]]).detach().cpu().double()
    w = R.layer_weights("linear", 2).double()
    rows = []
    for l in range(2):
        o = R.criterion_layer(logits[l], poses[l], poses2d[l], pairs, gt, vis3, vis2, nump, cam, aff, size, cen, 0.5)
        rows.append(torch.stack([torch.as_tensor(o[k], dtype=f64).reshape(()) for k in R.KEYS]))
        for i, k in enumerate(R.KEYS):
            got, want = float(ld["dict_losses_layers"][l][k]), float(rows[-1][i])
            print(tdt, l, k, got, want)
            if k in R.METRICS:
                assert np.float32(got) == np.float32(want), (l, k, got, want)
            else:
                assert abs(got - want) <= 1e-6 * abs(want), (l, k, got, want)
    rows = torch.stack(rows)
    for i, k in enumerate(R.KEYS):
        want = float(rows[:, i].mean()) if k in R.METRICS else float((w * rows[:, i]).sum())
        assert abs(float(ld[k]) - want) <= 2e-6 * abs(want) + 1e-12, (k, float(ld[k]), want)
    # the matched mask was the decoder's filter: unmatched queries were not triangulated (zero poses), matched ones were
    matched = torch.zeros(case.NQ, dtype=torch.bool)
    matched[pairs[0][0]] = True
    nz = poses[-1][0].view(case.NQ, -1).abs().sum(1) > 0
    assert bool((nz[~matched] == False).all()) and bool(nz[matched].any())      # noqa: E712
