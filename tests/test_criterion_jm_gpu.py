"""GPU checks of the joint map of the training criterion (Shelf / Campus joint format): mvg_knn_match_jm / mvg_criterion_jm
against the reference's fixture (tests/golden/criterion_jm.npz), the fp64 restatement on gathered predictions, and -- exactly --
against the map-less entry points on predictions gathered with torch; then the layers above them: DecoderHead.forward_train,
training.GraphedTrainStep from the Shelf YAML, validate's PCP row.

Tolerances against the fixture: the rule of tests/test_criterion_gpu.py (4 x the reference's own fp32-against-fp64 error, floored
at 1e-6 relative; gradients: max abs error over max abs value), computed from criterion_jm.npz.  Everything else is equality."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import criterion_ref as R
from tests.golden import criterion_cases as cc
from tests.golden import criterion_jm_cases as jc
from tests.test_criterion_jm_cpu import FIX, SHELF_YAML, restate

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOX = (jc.SPACE_SIZE, jc.SPACE_CENTER)
E_BADARG = 10001


def _criterion(c):
    from types import SimpleNamespace as NS
    from mvgformer_amd.criterion import KNNMatcher, SetCriterion
    cfg = NS(MULTI_PERSON=NS(SPACE_SIZE=list(jc.SPACE_SIZE), SPACE_CENTER=list(jc.SPACE_CENTER)), NETWORK=NS(IMAGE_SIZE=list(jc.IMG_WH)),
             DECODER=NS(pred_conf_threshold=jc.PRED_CONF_THRESHOLD, num_instance=c["NQ"]))
    m = KNNMatcher("abs", "norm", cost_class=2.0, cost_pose=5.0, method=c["method"], method_value=c["value"])
    return SetCriterion(2, m, {}, ["joints", "labels", "cardinality"], cfg)


def _device_case(inp):
    from mvgformer_amd import ops
    meta = jc.make_meta(inp, DEV)
    t = {k: torch.from_numpy(inp[k]).to(DEV) for k in ("init_poses", "logits", "poses", "poses_2d")}
    t["vis2d"] = torch.stack([m["joints_vis"] for m in meta]).float()
    return meta, t, ops.pack_cameras(meta, list(jc.IMG_WH), DEV)


def _fused(name):
    """pairs, table rows (L, 7), the three gradients (15-joint shape) through criterion_all_layers with the case's map"""
    from mvgformer_amd.criterion import criterion_all_layers
    c = jc.CASES[name]
    meta, t, cams = _device_case(jc.make_inputs(name))
    lg, ps, p2 = (t[k].clone().requires_grad_(True) for k in ("logits", "poses", "poses_2d"))
    ld, pairs = criterion_all_layers(_criterion(c), lg, ps, p2, meta, t["init_poses"], "none", cams, joint_map=c["joint_map"])
    (ld["loss_ce"] + ld["loss_pose_perjoint"] + ld["loss_pose_perprojection_2d"]).backward()
    rows = torch.stack([torch.stack([d[k] for k in R.KEYS]) for d in ld["dict_losses_layers"]]).detach()
    return pairs, rows, (lg.grad, ps.grad, p2.grad)


def _ops_calls(inp, c, joint_map, gathered=False):
    """ops.knn_match + ops.criterion -> (pq, pg, pc, matched, table, gl, gp, gp2).  gathered: the predictions indexed with torch and
    the map-less calls (J = Jc), the two pose gradients scattered back into zero tensors of the 15-joint shape"""
    from mvgformer_amd import ops
    meta, t, cams = _device_case(inp)
    m0, NQ = meta[0], c["NQ"]
    init, ps, p2 = t["init_poses"], t["poses"], t["poses_2d"]
    kw, kwm = {}, {}
    if gathered:
        init, ps, p2 = (jc.gather(x, joint_map, NQ).contiguous() for x in (init, ps, p2))
    elif joint_map is not None:
        kw, kwm = dict(joint_map=joint_map), dict(joint_map=joint_map, num_joints=jc.JP)
    pq, pg, pc, matched = ops.knn_match(init, m0["joints_3d"], m0["num_person"], *BOX, c["method"], c["value"], **kwm)
    table, gl, gp, gp2 = ops.criterion(t["logits"], ps, p2, pq, pg, pc, m0["joints_3d"], m0["joints_3d_vis"], t["vis2d"],
                                       m0["num_person"], cams, *BOX, jc.PRED_CONF_THRESHOLD, **kw)
    if gathered:
        gp, gp2 = jc.scatter(gp, joint_map, NQ), jc.scatter(gp2, joint_map, NQ)
    return pq, pg, pc, matched, table, gl, gp, gp2


# ---- 1: the matcher against the fixture ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(jc.CASES))
def test_knn_match_with_a_joint_map_equals_the_fixture(name):
    c = jc.CASES[name]
    pq, pg, pc, matched = (x.cpu() for x in _ops_calls(jc.make_inputs(name), c, c["joint_map"])[:4])
    for b in range(c["B"]):
        n = int(pc[b])
        q, g = pq[b, :n].tolist(), pg[b, :n].tolist()
        assert q == FIX["%s/pairs/%d/query" % (name, b)].tolist() and g == FIX["%s/pairs/%d/gt" % (name, b)].tolist(), (name, b)
        union = torch.zeros(c["NQ"], dtype=torch.uint8)
        union[torch.tensor(q, dtype=torch.long)] = 1
        assert torch.equal(matched[b], union)
        assert torch.all(pq[b, n:] == -1) and torch.all(pg[b, n:] == -1)


# ---- 2: table and gradients against the fp64 column ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(jc.CASES))
def test_losses_metrics_and_gradients_against_the_fp64_fixture(name):
    _, want, wgrads = restate(name)                              # pinned to the fixture's fp64 column at 1e-10 by the CPU tests
    want = want.numpy()
    assert np.abs(want - FIX[name + "/table/f64"]).max() <= 1e-10 * np.abs(want).max()
    _, got, grads = _fused(name)
    got = got.cpu().double().numpy()
    f32, f64 = FIX[name + "/table/f32"].astype(np.float64), FIX[name + "/table/f64"]
    bars = np.maximum(4 * np.abs(f32 - f64) / np.maximum(np.abs(f64), 1e-30), 1e-6)
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
        f32, f64 = FIX["%s/%s/f32" % (name, key)].astype(np.float64), FIX["%s/%s/f64" % (name, key)]
        bar = max(4 * np.abs(f32 - f64).max() / max(np.abs(f64).max(), 1e-30), 1e-6)
        assert g.shape == w.shape
        scale = float(w.abs().max())
        err = float((g.cpu().double() - w).abs().max()) / max(scale, 1e-30) if scale > 0 else float(g.abs().max())
        print(name, key, "err", err, "bar", bar)
        assert err <= bar, (name, key, err, bar)


# ---- 3: the gather oracle, exact ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(jc.CASES))
def test_mapped_call_equals_the_map_less_call_on_gathered_predictions_bit_for_bit(name):
    c = jc.CASES[name]
    inp = jc.make_inputs(name)
    mapped = _ops_calls(inp, c, c["joint_map"])
    oracle = _ops_calls(inp, c, c["joint_map"], gathered=True)
    for what, a, b in zip(("pair_query", "pair_gt", "pair_count", "matched", "table", "grad_logits", "grad_poses", "grad_poses_2d"),
                          mapped, oracle):
        assert a.shape == b.shape and torch.equal(a, b), (name, what, float((a.double() - b.double()).abs().max()))
    assert int(mapped[2].sum()) > 0 and float(mapped[6].abs().max()) > 0


# ---- the C ABI directly ----------------------------------------------------------------------------------------------------------
def _host3(x):
    return (C.c_float * 3)(*(float(v) for v in x))


def _int_array(jm):
    return None if jm is None else (C.c_int * len(jm))(*[int(v) for v in jm])


def _guarded(shape, pad=4096):
    """a float32 tensor of `shape` in the middle of a NaN-filled buffer -> (whole buffer, view, pad)"""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * pad,), float("nan"), dtype=torch.float32, device=DEV)
    return whole, whole[pad:pad + n].view(shape), pad


def _raw_match(inp, c, Jp, Jc, jm):
    """mvg_knn_match_jm through ctypes on sentinel-filled outputs -> rc, (pq, pg, pc, matched)"""
    from mvgformer_amd import _lib as L
    lib = L.load()
    meta, t, _ = _device_case(inp)
    m0 = meta[0]
    B, Gmax = m0["joints_3d"].shape[:2]
    NQ = c["NQ"]
    knn = c["method"] == "KNN"
    K = int(c["value"]) if knn else 0
    Pmax = Gmax * K if knn else NQ
    pq = torch.full((B, Pmax), -7, dtype=torch.int32, device=DEV)
    pg, pc = pq.clone(), torch.full((B,), -7, dtype=torch.int32, device=DEV)
    matched = torch.full((B, NQ), 7, dtype=torch.uint8, device=DEV)
    nbytes = lib.mvg_knn_match_workspace(B, NQ, Gmax)
    ws = torch.empty((max(nbytes, 8),), dtype=torch.uint8, device=DEV)
    rc = lib.mvg_knn_match_jm(L.ptr(t["init_poses"]), L.ptr(m0["joints_3d"]), L.ptr(m0["num_person"]), 1, _host3(BOX[0]),
                              _host3(BOX[1]), {"KNN": 0, "multiple": 1}[c["method"]], K, float(c["value"]), B, NQ, Gmax, Jp, Jc,
                              _int_array(jm), Pmax, L.ptr(ws), nbytes, L.ptr(pq), L.ptr(pg), L.ptr(pc), L.ptr(matched), L.stream_ptr())
    torch.cuda.synchronize()
    return rc, (pq, pg, pc, matched)


def _raw_criterion(inp, c, pairs, Jp, Jc, jm):
    """mvg_criterion_jm through ctypes, every output inside a NaN-filled buffer -> rc, dict of (whole, view, pad)"""
    from mvgformer_amd import _lib as L
    lib = L.load()
    meta, t, cams = _device_case(inp)
    m0 = meta[0]
    Ln, B, NQ = t["logits"].shape[:3]
    Gmax, V = m0["joints_3d"].shape[1], t["poses_2d"].shape[2]
    out = dict(table=_guarded((Ln, 8)), gl=_guarded(tuple(t["logits"].shape)), gp=_guarded(tuple(t["poses"].shape)),
               gp2=_guarded(tuple(t["poses_2d"].shape)))
    nbytes = lib.mvg_criterion_workspace(Ln, B, Gmax, V, max(1, min(Jc, 64)))
    ws = torch.empty((nbytes // 8 + 1,), dtype=torch.float64, device=DEV)
    pq, pg, pc = pairs
    rc = lib.mvg_criterion_jm(L.ptr(t["logits"]), L.ptr(t["poses"]), L.ptr(t["poses_2d"]), L.ptr(pq), L.ptr(pg), L.ptr(pc),
                              L.ptr(m0["joints_3d"]), L.ptr(m0["joints_3d_vis"]), L.ptr(t["vis2d"]), L.ptr(m0["num_person"]), 1, None,
                              L.ptr(cams), _host3(BOX[0]), _host3(BOX[1]), float(jc.PRED_CONF_THRESHOLD), 0.25, 2.0, Ln, B, NQ, Jp, Jc,
                              _int_array(jm), V, Gmax, pq.shape[1], L.ptr(ws), ws.numel() * 8, L.ptr(out["table"][1]), L.ptr(out["gl"][1]),
                              L.ptr(out["gp"][1]), L.ptr(out["gp2"][1]), L.stream_ptr())
    torch.cuda.synchronize()
    return rc, out


# ---- 4: identity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cc.CASES))
def test_null_map_and_identity_map_equal_the_existing_entry_points(name):
    c = cc.CASES[name]
    inp = cc.make_inputs(name)
    want = _ops_calls(inp, c, None)                              # mvg_knn_match / mvg_criterion
    ident = _ops_calls(inp, c, list(range(15)))                  # the mapped kernels with the identity written out
    for a, b in zip(ident, want):
        assert torch.equal(a, b), name
    rc, raw = _raw_match(inp, c, 15, 15, None)                   # the new symbols with NULL
    assert rc == 0 and all(torch.equal(a, b) for a, b in zip(raw, want[:4]))
    rc, out = _raw_criterion(inp, c, want[:3], 15, 15, None)
    assert rc == 0
    for key, b in zip(("table", "gl", "gp", "gp2"), want[4:]):
        assert torch.equal(out[key][1], b), (name, key)


# ---- 5: dense writes -------------------------------------------------------------------------------------------------------------
def test_gradients_are_written_densely_and_unnamed_joints_get_zeros():
    c = jc.CASES["shelf"]
    inp = jc.make_inputs("shelf")
    rc, pairs = _raw_match(inp, c, 15, 14, c["joint_map"])
    assert rc == 0
    rc, out = _raw_criterion(inp, c, pairs[:3], 15, 14, c["joint_map"])
    assert rc == 0
    for key in ("table", "gl", "gp", "gp2"):
        whole, view, pad = out[key]
        assert bool(torch.isnan(whole[:pad]).all()) and bool(torch.isnan(whole[pad + view.numel():]).all()), key   # guards untouched
        assert not bool(torch.isnan(view).any()), key                                                            # every element written
    NQ = c["NQ"]
    gp = out["gp"][1].view(c["L"], c["B"], NQ, 15, 3)
    gp2 = out["gp2"][1].view(c["L"], c["B"], c["V"], NQ, 15, 2)
    assert 2 not in c["joint_map"]
    assert float(gp[..., 2, :].abs().max()) == 0.0 and float(gp2[..., 2, :].abs().max()) == 0.0
    assert float(gp.abs().max()) > 0 and float(gp2.abs().max()) > 0
    unmatched = pairs[3] == 0
    assert float(gp[:, unmatched].abs().max()) == 0.0


# ---- 6: bad arguments ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Jp,Jc,jm", [(15, 14, [14, 13, 12, 6, 7, 8, 11, 10, 9, 3, 4, 5, 0, 0]),          # a repeated entry
                                      (15, 14, [14, 13, 12, 6, 7, 8, 11, 10, 9, 3, 4, 5, 0, 15]),         # an entry equal to Jp
                                      (15, 65, list(range(65))),                                          # Jc = 65
                                      (15, 0, [0]),                                                       # Jc = 0
                                      (15, 14, None)],                                                    # NULL with Jc != Jp
                         ids=["repeated", "entry=Jp", "Jc=65", "Jc=0", "null"])
def test_bad_maps_give_badarg_and_nothing_is_written(Jp, Jc, jm):
    c = jc.CASES["shelf"]
    inp = jc.make_inputs("shelf")
    rc, outs = _raw_match(inp, c, Jp, Jc, jm)
    assert rc == E_BADARG
    assert all(bool((x == -7).all()) for x in outs[:3]) and bool((outs[3] == 7).all())
    rc, good = _raw_match(inp, c, 15, 14, c["joint_map"])
    assert rc == 0
    rc, out = _raw_criterion(inp, c, good[:3], Jp, Jc, jm)
    assert rc == E_BADARG
    assert all(bool(torch.isnan(out[k][0]).all()) for k in out)


# ---- 7: determinism, launch counts, no host synchronisation ----------------------------------------------------------------------
def test_two_runs_are_bit_identical():
    for name in ("shelf", "q1024g11"):
        a, b = _fused(name), _fused(name)
        assert torch.equal(a[1], b[1])
        assert all(torch.equal(x, y) for x, y in zip(a[2], b[2])) and all(torch.equal(x, y) for x, y in zip(a[0], b[0]))


@pytest.mark.parametrize("L", [4, 6])
def test_no_host_synchronisation_and_the_launch_counts_of_the_map_less_calls(L):
    from mvgformer_amd import ops
    from mvgformer_amd.criterion import criterion_all_layers
    from tests.test_criterion_gpu import _device_kernels
    c = jc.CASES["shelf"]
    jm = list(c["joint_map"])
    meta, t, cams = _device_case(jc.make_inputs("shelf"))
    crit = _criterion(c)
    rep = lambda x: x[:1].expand(L, *x.shape[1:]).clone().requires_grad_(True)     # noqa: E731
    lg, ps, p2 = rep(t["logits"]), rep(t["poses"]), rep(t["poses_2d"])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ld, _ = criterion_all_layers(crit, lg, ps, p2, meta, t["init_poses"], "linear", cams, joint_map=jm)
        (ld["loss_ce"] + ld["loss_pose_perjoint"] + ld["loss_pose_perprojection_2d"]).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(ld["dict_losses_layers"]) == L and torch.isfinite(ps.grad).all() and ps.grad.shape == ps.shape
    m0, holder = meta[0], {}

    def run_match():
        holder["pairs"] = ops.knn_match(t["init_poses"], m0["joints_3d"], m0["num_person"], *BOX, "KNN", 5, joint_map=jm, num_joints=15)

    def run_criterion():
        pq, pg, pc, _ = holder["pairs"]
        ops.criterion(lg.detach(), ps.detach(), p2.detach(), pq, pg, pc, m0["joints_3d"], m0["joints_3d_vis"], t["vis2d"],
                      m0["num_person"], cams, *BOX, jc.PRED_CONF_THRESHOLD, joint_map=jm)
    match_events = _device_kernels(run_match)
    crit_events = _device_kernels(run_criterion)
    print("match:", match_events, "criterion:", crit_events)
    assert len(match_events) == 1 and "knn_match_kernel" in match_events[0], match_events
    assert len(crit_events) == 3 and all("crit_" in n for n in crit_events), crit_events


# ---- 8: forward_train ------------------------------------------------------------------------------------------------------------
def _shelf_data(case_seed=4, persons=3, gt_seed=1):
    from mvgformer_amd.factory import case_to_device
    from mvgformer_amd.synthetic import add_ground_truth, build_case, convert_ground_truth
    case = build_case("mini5", seed=case_seed, NQ=128, layers=2)
    g = add_ground_truth(case_to_device(case, DEV), [persons], Gmax=4, seed=gt_seed)
    return case, convert_ground_truth(g, jc.SHELF_MAP)


def _shelf_cfg(case):
    """the Shelf YAML's extract at mini5's shapes: the case's space, image and query count"""
    from types import SimpleNamespace as NS
    from mvgformer_amd import validate
    cfg = validate.load_config("extract:" + SHELF_YAML)
    cfg.DECODER = NS(**dict(vars(cfg.DECODER), num_instance=case.NQ, num_decoder_layers=case.layers))
    cfg.NETWORK = NS(IMAGE_SIZE=list(case.img_size))
    cfg.MULTI_PERSON = NS(SPACE_SIZE=list(case.space_size), SPACE_CENTER=list(case.space_center))
    return cfg


def _shelf_head(case, tdt, weights_case=None):
    from mvgformer_amd.factory import build_decoder_for_case, build_training_head
    dec = build_decoder_for_case(weights_case or case, DEV, torch.float32)
    dec.set_training_dtype(tdt)
    torch.manual_seed(0)
    head, weight_dict = build_training_head(_shelf_cfg(case), decoder=dec)
    head = head.to(DEV)
    head.train()
    for layer in dec.layers:
        layer.dropout2.p = layer.dropout3.p = layer.dropout4.p = 0.0           # bits are compared
    for p in head.parameters():
        p.requires_grad_(True)
    return head, weight_dict


@pytest.mark.parametrize("tdt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_forward_train_in_the_shelf_joint_format_equals_the_gather_formulation(tdt):
    from mvgformer_amd import caller
    from mvgformer_amd.criterion import criterion_all_layers, total_loss
    from mvgformer_amd.decoder import DecoderContext
    case, g = _shelf_data()
    jm = list(jc.SHELF_MAP)
    assert g.meta[0]["joints_3d"].shape == (1, 4, 14, 3) and g.meta[2]["joints_vis"].shape == (1, 4, 14, 2)
    head, weight_dict = _shelf_head(case, tdt)
    assert head.convert_joint_format_indices == jm and weight_dict["loss_ce"] == 0.0
    out, ld = head.forward_train(g.src_views, g.meta, g.spatial_shapes, g.level_start_index, threshold=0.1)
    total = total_loss(ld, weight_dict)
    total.backward()
    named = dict(head.named_parameters())
    assert torch.isfinite(total) and float(total) > 0
    got = {n: p.grad.clone() for n, p in named.items() if p.grad is not None}
    assert len(got) >= 50 and all(bool(torch.isfinite(v).all()) for v in got.values())
    assert "joint_embedding.weight" in got and "instance_embedding.weight" in got
    assert out["pred_poses"]["outputs_coord"].shape == (1, case.NQ * 14, 3)
    assert out["pred_poses_2d"]["outputs_coord_2d"].shape == (1, case.V, case.NQ * 14, 2)

    # the gather formulation: the same forward, predictions indexed with torch, the map-less criterion on 14-joint tensors
    for p in head.parameters():
        p.grad = None
    layer0 = head.decoder.layers[0]
    query_pos, tgt = caller.person_joint_queries(head.joint_embedding.weight, head.instance_embedding.weight, 1)
    ctx = DecoderContext.prepare(g.spatial_shapes, g.level_start_index, g.meta, layer0.img_size, layer0.compute_dtype, 1, torch.device(DEV))
    ref = caller.sample_space_reference_points(head.num_instance, head.space_size, head.space_center, 1, torch.device(DEV), t_pose=head.t_pose)
    ref_conv = jc.gather(ref, jm, case.NQ).contiguous()
    pairs = head.criterion.matcher.match(ref_conv, g.meta)
    outs = head.decoder(tgt.contiguous(), ref, g.src_views, g.meta, g.spatial_shapes, g.level_start_index, None,
                        query_pos=query_pos.contiguous(), indices=pairs[3], threshold=0.1, context=ctx)
    want_out = caller.decoder_outputs_to_dict(*outs, head.num_instance, head.num_joints, jm)
    for k in ("pred_logits",):
        assert torch.equal(out[k], want_out[k])
    for k, kk in (("pred_poses", "outputs_coord"), ("pred_poses_2d", "outputs_coord_2d"), ("pred_poses_2d_proj", "outputs_coord_2d_proj")):
        assert torch.equal(out[k][kk], want_out[k][kk]), k
    ld2, _ = criterion_all_layers(head.criterion, torch.stack(want_out["all_logits"]),
                                  torch.stack([c["outputs_coord"] for c in want_out["all_poses"]]),
                                  torch.stack([c["outputs_coord_2d"] for c in want_out["all_poses_2d"]]), g.meta, ref_conv,
                                  head.decay_method, cams=ctx.cams, pairs=pairs)
    total2 = total_loss(ld2, weight_dict)
    total2.backward()
    assert torch.equal(total2.detach(), total.detach())
    for k in R.KEYS:
        assert torch.equal(ld2[k].detach(), ld[k].detach()), k
    want = {n: p.grad for n, p in named.items() if p.grad is not None}
    assert sorted(want) == sorted(got)
    for n in want:
        assert torch.equal(got[n], want[n]), n


# ---- 9: the graphed step from the Shelf YAML -------------------------------------------------------------------------------------
def _shelf_rig(tdt, data=None):
    from mvgformer_amd.factory import build_graphed_train_step, build_optimizer_from_cfg
    from mvgformer_amd.synthetic import build_case
    from tests.test_train_graph_gpu import Rig

    class ShelfRig(Rig):
        def __init__(self):
            case, self.g = data if data is not None else _shelf_data()
            wcase = case if data is None else build_case("mini5", seed=4, NQ=128, layers=2)     # always the standard weights
            self.head, self.weight_dict = _shelf_head(case, tdt, wcase)
            self.dec = self.head.decoder
            self.opt = build_optimizer_from_cfg(self.head, _shelf_cfg(case))
            self.runner = build_graphed_train_step(self.head, self.opt, self.g, capture=False)
            self.ops16 = self.runner.operands
            self.start = {n: p.detach().clone() for n, p in self.head.named_parameters()}
    return ShelfRig()


@pytest.mark.parametrize("tdt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_graphed_shelf_step_replays_equal_eager_steps_bit_for_bit(tdt):
    from tests.test_train_graph_gpu import _assert_same, _run
    rig0 = _shelf_rig(tdt)
    assert rig0.opt.defaults["decoupled_weight_decay"] and rig0.weight_dict["loss_ce"] == 0.0         # AdamW, loss_ce weight 0
    assert rig0.runner.meta[0]["joints_3d"].shape[2] == 14
    e1 = _run(rig0, 3, replay=False)
    rig = _shelf_rig(tdt).captured()
    got = _run(rig, 3, replay=True)
    _assert_same(got, e1, "replay vs eager")
    losses = [float(m[0]) for m in got[0]]
    assert len(set(losses)) == 3 and all(torch.isfinite(m[0]) and float(m[1]) > 0 for m in got[0])
    assert rig.opt.step_count() == 3
    # other 14-joint ground truth between replays
    other = _shelf_data(case_seed=4, persons=2, gt_seed=3)
    assert not torch.equal(other[1].meta[0]["joints_3d"], rig.runner.meta[0]["joints_3d"])
    rig.restore()
    rig.runner.load(meta=other[1].meta)
    got = _run(rig, 1, replay=True)
    want = _run(_shelf_rig(tdt, data=other), 1, replay=False)
    _assert_same(got, want, "replay after load() vs eager")


# ---- 10: PCP in validate ---------------------------------------------------------------------------------------------------------
def test_validate_reports_pcp_for_shelf_frames_with_ground_truth(tmp_path):
    import yaml
    from mvgformer_amd import evaluate as E
    from mvgformer_amd import validate
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mvgformer_amd", "data", "yaml_extract.json")) as f:
        val = json.load(f)[SHELF_YAML]
    raw = {"DECODER": dict(val["DECODER"], num_instance=128, num_decoder_layers=2), "NETWORK": {"IMAGE_SIZE": [320, 192]},
           "MULTI_PERSON": {"SPACE_SIZE": val["SPACE_SIZE"], "SPACE_CENTER": val["SPACE_CENTER"]}, "DATASET": {"CAMERA_NUM": 3}}
    cfg_path = str(tmp_path / "shelf_small.yaml")
    with open(cfg_path, "w") as f:
        yaml.safe_dump(raw, f)
    cfg = validate.load_config(cfg_path)
    frames = list(validate.synthetic_frames(cfg, 2, seed=5))
    arrays = {}
    for l in range(len(frames[0][0])):
        arrays["feat%d" % l] = np.stack([fr[0][l].numpy() for fr in frames])
    for k in ("R", "T", "fx", "fy", "cx", "cy", "k", "p"):
        arrays["camera_" + k] = np.stack([np.stack([m["camera"][k][0].numpy() for m in fr[1]]) for fr in frames])
    for k in ("center", "scale", "inv_affine_trans"):
        arrays[k] = np.stack([np.stack([m[k][0].numpy() for m in fr[1]]) for fr in frames])
    npz, out = str(tmp_path / "frames.npz"), str(tmp_path / "pred")
    np.savez(npz, **arrays)
    args = ["--cfg", cfg_path, "--frames-npz", npz, "--dtype", "fp32", "--pred-out", out]
    first = validate.main(args)["results"][0]
    assert "PCP" not in first and "AP" not in first and first["frames"] == 2           # no ground truth: the row as before
    thr = first["inference_conf_thr"]

    def kept_of():
        pred = np.load("%s-%s.npy" % (out, thr))
        assert pred.shape == (2, 128, 14, 5)
        return [E.filter_and_nms(torch.from_numpy(p).to(DEV)) for p in pred]
    kept = kept_of()
    G = min(3, min(len(k) for k in kept))
    assert G >= 1
    # ground truth: up to three kept poses of each frame, moved a little; the last actor is not annotated in frame 1
    rs = np.random.RandomState(0)
    gt = np.stack([k[:G, :, :3].cpu().numpy() + rs.standard_normal((G, 14, 3)) * 15.0 for k in kept]).astype(np.float32)
    vis = np.ones((2, G, 14, 3), np.float32)
    if G > 1:
        vis[1, G - 1] = 0
    np.savez(npz, joints_3d=gt, joints_3d_vis=vis, **arrays)
    row = validate.main(args)["results"][0]
    kept = kept_of()
    actors = [[gt[f, a].astype(np.float64) if vis[f, a].any() else None for f in range(2)] for a in range(G)]
    actor, avg, bones, recall = E.evaluate_pcp(kept, actors)
    pcp = row["PCP"]
    assert pcp["actor"] == [round(100 * float(a), 2) for a in actor] and pcp["average"] == round(100 * float(avg), 2)
    assert pcp["bones"] == {k: [round(100 * float(x), 2) for x in v] for k, v in bones.items()}
    assert pcp["recall500"] == round(100 * float(recall), 2)
    assert len(pcp["actor"]) == G and pcp["recall500"] > 99 and "AP" not in row     # every annotated actor has its pose within 500 mm
    assert {k: v for k, v in row.items() if k not in ("PCP", "decoder_ms_per_frame")} == \
           {k: v for k, v in first.items() if k != "decoder_ms_per_frame"}
