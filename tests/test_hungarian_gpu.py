"""GPU checks of the one-to-one ground-truth matcher (csrc/hungarian.hip, mvg_hungarian_match) against the numpy restatement
tests/hungarian_ref.py, the reference's recorded pairs (tests/golden/hungarian.npz) and the dual certificate of optimality; and of
what is built on it: criterion.HungarianMatcher, SetCriterion.forward on the layer's own logits, per-layer matching in
criterion_all_layers, DecoderHead.forward_train and the captured training step.

Pairs, counts and masks compare exactly.  The certificate runs on the DEVICE's potentials against the restated cost matrix with
tol = 1e-9 * max|C| (hungarian_ref.check_certificate): the device's exp / log may differ from numpy's in the last bits (1e-16
relative), far below it."""
import ctypes as C
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import criterion_ref as R
from tests import hungarian_cases as HC
from tests import hungarian_ref as H
from tests.golden import criterion_cases as cc
from tests.test_hungarian_cpu import golden, restated

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = 0xA5
BADARG = 10001


def _dev(inp):
    return {k: torch.from_numpy(v).to(DEV) for k, v in inp.items()}


def _poisoned(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(torch.uint8).fill_(POISON)
    return t


def _still_poisoned(*tensors):
    return all(bool((t.view(torch.uint8) == POISON).all()) for t in tensors)


def raw_call(poses, gt, num, logits=None, method=2, cost_class=2.0, cost_pose=5.0, size=HC.SPACE_SIZE, center=HC.SPACE_CENTER,
             joint_map=None, duals=True, null=(), **dims):
    """mvg_hungarian_match itself on output buffers filled with a poison byte.  Dimensions come from the tensors unless given in
    `dims` (the refused-argument checks pass wrong ones); `null`: argument names passed as NULL.  -> (return code, outputs)"""
    from mvgformer_amd import _lib
    lib = _lib.load()
    lead = poses.dim() == 4
    B, Gmax, Jc = gt.shape[:3]
    Jp = dims.get("Jp", Jc)
    d = dict(P=(poses.shape[0] if lead else 1) * B, B=B, Gmax=Gmax, Jc=Jc, Jp=Jp)
    d.update(dims)
    if "NQ" not in d:
        d["NQ"] = poses.shape[-2] // Jp
    P, NQ = max(d["P"], 1), d["NQ"]
    out = dict(pair_query=_poisoned((P, d["Gmax"]), torch.int32), pair_gt=_poisoned((P, d["Gmax"]), torch.int32),
               pair_count=_poisoned((P,), torch.int32), matched=_poisoned((P, NQ), torch.uint8))
    uv = _poisoned((P * (d["Gmax"] + NQ) + 1,), torch.float64) if duals else None       # one guard element behind the last row
    nbytes = lib.mvg_hungarian_match_workspace(P, NQ, d["Gmax"])
    ws = torch.empty((max(nbytes, 4) // 4,), dtype=torch.float32, device=DEV)
    ws_bytes = dims.get("ws_bytes", nbytes)
    is64 = int(num.dtype == torch.int64)
    jm = None if joint_map is None else (C.c_int * len(joint_map))(*joint_map)
    ptr = {k: _lib.ptr(t) for k, t in dict(logits=logits, poses=poses, gt=gt, num=num, ws=ws if nbytes else None, **out).items()}
    ptr["duals"] = None if uv is None else C.c_void_p(uv.data_ptr() + dims.get("duals_offset", 0))
    sz, cn = (C.c_float * 3)(*size), (C.c_float * 3)(*center)
    for k in null:
        if k == "size":
            sz = None
        elif k == "center":
            cn = None
        else:
            ptr[k] = None
    rc = lib.mvg_hungarian_match(ptr["logits"], ptr["poses"], ptr["gt"], ptr["num"], is64, sz, cn, method, cost_class, cost_pose, d["P"],
                                 d["B"], NQ, d["Gmax"], d["Jp"], d["Jc"], jm, ptr["ws"], ws_bytes, ptr["pair_query"], ptr["pair_gt"],
                                 ptr["pair_count"], ptr["matched"], ptr["duals"], _lib.stream_ptr())
    torch.cuda.synchronize()
    if uv is not None:
        rows = uv[:-1].view(P, d["Gmax"] + NQ)
        out["u"], out["v"], out["uv"] = rows[:, :d["Gmax"]].contiguous(), rows[:, d["Gmax"]:].contiguous(), uv
    return rc, out


def _assert_equals_restatement(out, r, what, certificate=True):
    """out: device tensors with the problems flattened; r: hungarian_ref.hungarian_match's dict"""
    flat = {k: np.asarray(v).reshape((-1,) + np.asarray(v).shape[(2 if r["pair_count"].ndim == 2 else 1):]) for k, v in r.items()}
    for k in ("pair_query", "pair_gt", "pair_count", "matched"):
        got = out[k].cpu().numpy().reshape(flat[k].shape)
        assert np.array_equal(got, flat[k]), (what, k, got, flat[k])
    if certificate and "u" in out:
        u, v = (out[k].cpu().numpy().reshape(-1, out[k].shape[-1]) for k in ("u", "v"))
        assert np.isfinite(u).all() and np.isfinite(v).all()
        for p in range(flat["C"].shape[0]):
            H.check_certificate(flat["C"][p], int(flat["pair_count"][p]), flat["pair_query"][p], flat["pair_gt"][p], u[p], v[p], (what, p))


@pytest.mark.parametrize("name", sorted(HC.CASES))
def test_device_equals_the_restatement_and_writes_every_slot(name):
    inp, r = restated(name)
    t = _dev(inp)
    c = HC.CASES[name]
    kw = dict(method={"hungarian": 2, "hungarian-dis": 3}[c["method"]], joint_map=c["joint_map"])
    if c["Jp"] is not None:
        kw["Jp"] = c["Jp"]
    rc, out = raw_call(t["poses"], t["joints_3d"], t["num_person"], t["logits"], **kw)
    assert rc == 0
    uv = out["uv"]
    assert not bool((out["pair_query"].view(torch.uint8).reshape(-1, 4) == POISON).all(-1).any())     # no int32 is 0xA5A5A5A5 any more
    assert not bool((out["pair_gt"].view(torch.uint8).reshape(-1, 4) == POISON).all(-1).any())
    assert not bool((out["pair_count"].view(torch.uint8).reshape(-1, 4) == POISON).all(-1).any())
    assert not bool((out["matched"] == POISON).any())
    assert not bool((uv[:-1].view(torch.uint8).reshape(-1, 8) == POISON).all(-1).any())
    assert _still_poisoned(uv[-1:])                                                      # and nothing behind the last slot
    _assert_equals_restatement(out, r, name)
    # the wrapper: same launch, same bits, a leading Lm kept
    from mvgformer_amd import ops
    got = ops.hungarian_match(t["poses"], t["joints_3d"], t["num_person"], HC.SPACE_SIZE, HC.SPACE_CENTER, logits=t["logits"], duals=True,
                              **HC.match_kwargs(name))
    assert got[0].shape == (c["Lm"], c["B"], c["Gmax"]) and got[3].shape == (c["Lm"], c["B"], c["NQ"]) and got[5].shape[-1] == c["NQ"]
    for g, k in zip(got, ("pair_query", "pair_gt", "pair_count", "matched", "u", "v")):
        assert torch.equal(g.reshape(out[k].shape), out[k]), (name, k)


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
def test_person_counts_in_both_integer_types(dtype):
    for name in ("counts", "clamp"):
        inp, r = restated(name)
        t = _dev(inp)
        rc, out = raw_call(t["poses"], t["joints_3d"], t["num_person"].to(dtype), t["logits"])
        assert rc == 0
        _assert_equals_restatement(out, r, (name, dtype))
    assert out["pair_count"].tolist() == [6, 6]                                          # 9 and 1000 persons clamp to Gmax


@pytest.mark.parametrize("name", sorted(HC.TIE_CASES))
def test_tie_rule_on_the_device(name):
    from mvgformer_amd import ops
    tie = HC.TIE_CASES[name]
    t = _dev(HC.tie_inputs(name))
    pq, pg, pc, matched = ops.hungarian_match(t["poses"], t["joints_3d"], t["num_person"], *HC.TIE_SPACE, method="hungarian-dis")
    G = len(tie["persons"])
    assert pc.tolist() == [G] and list(zip(pq[0, :G].tolist(), pg[0, :G].tolist())) == tie["pairs"]
    assert matched[0].nonzero().flatten().tolist() == [q for q, _ in tie["pairs"]]


def test_logits_none_is_logit_one_and_dis_ignores_logits():
    from mvgformer_amd import ops
    inp, r = restated("nq257")
    t = _dev(inp)
    args = (t["poses"][0], t["joints_3d"], t["num_person"], HC.SPACE_SIZE, HC.SPACE_CENTER)
    none = ops.hungarian_match(*args, logits=None, cost_class=2.0, cost_pose=5.0, duals=True)
    ones = ops.hungarian_match(*args, logits=torch.ones_like(t["logits"][0]), cost_class=2.0, cost_pose=5.0, duals=True)
    for a, b in zip(none, ones):
        assert torch.equal(a, b)
    want = H.hungarian_match(inp["poses"][0], inp["joints_3d"], inp["num_person"], HC.SPACE_SIZE, HC.SPACE_CENTER, logits=None,
                             cost_class=2.0, cost_pose=5.0)
    _assert_equals_restatement(dict(zip(("pair_query", "pair_gt", "pair_count", "matched", "u", "v"), none)), want, "logits=None")
    with_logits = ops.hungarian_match(*args, logits=t["logits"][0], method="hungarian-dis", duals=True)
    without = ops.hungarian_match(*args, logits=None, method="hungarian-dis", duals=True)
    for a, b in zip(with_logits, without):
        assert torch.equal(a, b)
    assert not torch.equal(with_logits[0], none[0]) or not torch.equal(with_logits[4], none[4])


def test_nan_and_inf_queries_are_never_chosen():
    from mvgformer_amd import ops
    inp = {k: v.copy() for k, v in HC.make_inputs("nq70").items()}
    poses = inp["poses"].reshape(1, 1, 70, 15, 3)
    poses[0, 0, 0, 3, 1] = np.nan                      # queries 0 and 4 start near persons 0 and 1
    poses[0, 0, 4, 0, 0] = np.inf
    poses[0, 0, 69, 14, 2] = -np.inf
    t = _dev(inp)
    for method in ("hungarian", "hungarian-dis"):
        got = ops.hungarian_match(t["poses"], t["joints_3d"], t["num_person"], HC.SPACE_SIZE, HC.SPACE_CENTER, logits=t["logits"],
                                  method=method, cost_class=2.0, cost_pose=5.0, duals=True)
        torch.cuda.synchronize()                       # the call returns
        want = H.hungarian_match(inp["poses"], inp["joints_3d"], inp["num_person"], HC.SPACE_SIZE, HC.SPACE_CENTER, logits=inp["logits"],
                                 method=method, cost_class=2.0, cost_pose=5.0)
        assert np.all(want["C"][0, 0][:, [0, 4, 69]] == H.LAP_BIG)
        _assert_equals_restatement(dict(zip(("pair_query", "pair_gt", "pair_count", "matched", "u", "v"), got)), want, method)
        assert got[2].tolist() == [[10]] and not set(got[0].flatten().tolist()) & {0, 4, 69}


def test_identity_joint_map_equals_no_map():
    from mvgformer_amd import ops
    inp, _ = restated("nq257")
    t = _dev(inp)
    args = (t["poses"], t["joints_3d"], t["num_person"], HC.SPACE_SIZE, HC.SPACE_CENTER)
    a = ops.hungarian_match(*args, logits=t["logits"], cost_class=2.0, cost_pose=5.0, duals=True)
    b = ops.hungarian_match(*args, logits=t["logits"], cost_class=2.0, cost_pose=5.0, duals=True, joint_map=list(range(15)), num_joints=15)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_four_layers_in_one_launch_equal_four_launches():
    from mvgformer_amd import ops
    inp, _ = restated("lm4")
    t = _dev(inp)
    kw = dict(cost_class=2.0, cost_pose=5.0, duals=True)
    one = ops.hungarian_match(t["poses"], t["joints_3d"], t["num_person"], HC.SPACE_SIZE, HC.SPACE_CENTER, logits=t["logits"], **kw)
    for l in range(4):
        single = ops.hungarian_match(t["poses"][l], t["joints_3d"], t["num_person"], HC.SPACE_SIZE, HC.SPACE_CENTER, logits=t["logits"][l], **kw)
        for a, b in zip(one, single):
            assert torch.equal(a[l], b), l
    assert not torch.equal(one[0][0], one[0][1])                                         # the layers' problems do differ


def test_two_calls_are_bit_equal_and_a_captured_launch_replays_on_new_inputs():
    from mvgformer_amd import ops
    inp, r = restated("train")
    other = HC.make_inputs({**HC.CASES["train"], "seed": 206, "num_person": [7, 10]})
    want_other = H.hungarian_match(other["poses"], other["joints_3d"], other["num_person"], HC.SPACE_SIZE, HC.SPACE_CENTER,
                                   logits=other["logits"], cost_class=2.0, cost_pose=5.0)
    t, o = _dev(inp), _dev(other)
    call = lambda: ops.hungarian_match(t["poses"], t["joints_3d"], t["num_person"], HC.SPACE_SIZE, HC.SPACE_CENTER, logits=t["logits"],  # noqa: E731
                                       cost_class=2.0, cost_pose=5.0, duals=True)
    a, b = call(), call()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    keys = ("pair_query", "pair_gt", "pair_count", "matched", "u", "v")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = call()
    for k in t:
        t[k].copy_(o[k])
    graph.replay()
    torch.cuda.synchronize()
    _assert_equals_restatement(dict(zip(keys, static)), want_other, "replay on new inputs")
    assert static[2].tolist() == [[7, 10]] and not np.array_equal(want_other["pair_query"], r["pair_query"])


@pytest.mark.parametrize("name", HC.GOLDEN)
def test_device_pairs_equal_the_references(name):
    from mvgformer_amd import ops
    z = golden()
    t = _dev(HC.make_inputs(name))
    pq, pg, pc, _ = ops.hungarian_match(t["poses"], t["joints_3d"], t["num_person"], HC.SPACE_SIZE, HC.SPACE_CENTER, logits=t["logits"],
                                        **HC.match_kwargs(name))
    pq, pg, pc = pq.cpu(), pg.cpu(), pc.cpu()
    for l in range(pq.shape[0]):
        for b in range(pq.shape[1]):
            n = int(pc[l, b])
            assert pq[l, b, :n].tolist() == z["%s/%d/%d/query" % (name, l, b)].tolist(), (name, l, b)
            assert pg[l, b, :n].tolist() == z["%s/%d/%d/gt" % (name, l, b)].tolist(), (name, l, b)


def test_matcher_forward_returns_the_references_lists():
    from mvgformer_amd.criterion import HungarianMatcher
    z = golden()
    for name in ("train", "dis"):
        c = HC.CASES[name]
        t = _dev(HC.make_inputs(name))
        m = HungarianMatcher("abs", "norm", cost_class=c["cost_class"], cost_pose=c["cost_pose"], method=c["method"])
        m.grid_size, m.grid_center = torch.tensor(HC.SPACE_SIZE), torch.tensor(HC.SPACE_CENTER)
        meta = [dict(joints_3d=t["joints_3d"], num_person=t["num_person"])]
        got = m({"pred_logits": t["logits"][0], "pred_poses": {"outputs_coord": t["poses"][0]}}, meta)
        assert len(got) == c["B"]
        for b, (q, g) in enumerate(got):
            assert q.dtype == torch.int64 and g.dtype == torch.int64 and q.is_cuda
            assert q.tolist() == z["%s/0/%d/query" % (name, b)].tolist() and g.tolist() == z["%s/0/%d/gt" % (name, b)].tolist()
    # the reference's class in full: KNN through the same object
    pq, pg, pc, _ = m.match(t["poses"][0], meta, method="KNN", value=3)
    assert pq.shape == (2, 30) and pc.tolist() == [30, 12]


# ---- criterion ----------------------------------------------------------------------------------------------------------------
def _criterion(NQ):
    from mvgformer_amd.criterion import HungarianMatcher, SetCriterion
    cfg = NS(MULTI_PERSON=NS(SPACE_SIZE=list(cc.SPACE_SIZE), SPACE_CENTER=list(cc.SPACE_CENTER)), NETWORK=NS(IMAGE_SIZE=list(cc.IMG_WH)),
             DECODER=NS(pred_conf_threshold=cc.PRED_CONF_THRESHOLD, num_instance=NQ))
    return SetCriterion(2, HungarianMatcher("abs", "norm", cost_class=2.0, cost_pose=5.0), {}, ["joints", "labels", "cardinality"], cfg)


def _criterion_case(name="b2"):
    from mvgformer_amd import ops
    inp = cc.make_inputs(name)
    meta = cc.make_meta(inp, DEV)
    t = {k: torch.from_numpy(inp[k]).to(DEV) for k in ("logits", "poses", "poses_2d")}
    return inp, meta, t, ops.pack_cameras(meta, list(cc.IMG_WH), DEV)


def test_set_criterion_matches_on_the_layers_own_logits_and_equals_the_fp64_restatement():
    """the bars of tests/test_criterion_gpu.py for a case without fixture columns: 1e-6 relative on the losses, the metrics equal
    after rounding to fp32"""
    inp, meta, t, _ = _criterion_case()
    crit = _criterion(cc.CASES["b2"]["NQ"])
    t64, cam, aff = R.tensors_of(inp, torch.float64)
    size, cen = torch.tensor(cc.SPACE_SIZE, dtype=torch.float64), torch.tensor(cc.SPACE_CENTER, dtype=torch.float64)
    seen = []
    for l in range(cc.CASES["b2"]["L"]):
        out = {"pred_logits": t["logits"][l], "pred_poses": {"outputs_coord": t["poses"][l]},
               "pred_poses_2d": {"outputs_coord_2d": t["poses_2d"][l]}}
        losses, indices = crit(out, meta)
        r = H.hungarian_match(inp["poses"][l], inp["joints_3d"], inp["num_person"], cc.SPACE_SIZE, cc.SPACE_CENTER, logits=inp["logits"][l],
                              cost_class=2.0, cost_pose=5.0)
        pairs = []
        for b, (q, g) in enumerate(indices):
            n = int(r["pair_count"][b])
            assert q.tolist() == r["pair_query"][b, :n].tolist() and g.tolist() == r["pair_gt"][b, :n].tolist(), (l, b)
            pairs.append((torch.from_numpy(r["pair_query"][b, :n].astype(np.int64)), torch.from_numpy(r["pair_gt"][b, :n].astype(np.int64))))
        # the class term took part: without the logits another assignment comes out somewhere in this case's two layers
        blind = H.hungarian_match(inp["poses"][l], inp["joints_3d"], inp["num_person"], cc.SPACE_SIZE, cc.SPACE_CENTER, logits=None,
                                  cost_class=2.0, cost_pose=5.0)
        seen.append(not np.array_equal(blind["pair_query"], r["pair_query"]))
        want = R.criterion_layer(t64["logits"][l], t64["poses"][l], t64["poses_2d"][l], pairs, t64["joints_3d"], t64["joints_3d_vis"],
                                 t64["joints_vis"], t64["num_person"], cam, aff, size, cen, cc.PRED_CONF_THRESHOLD)
        for k in R.KEYS:
            g_, w_ = float(losses[k]), float(want[k])
            print(l, k, g_, w_)
            if k in R.METRICS:
                assert np.float32(g_) == np.float32(w_), (l, k, g_, w_)
            else:
                assert abs(g_ - w_) <= 1e-6 * abs(w_), (l, k, g_, w_)
    print("layers whose assignment depends on the logits:", seen)


def test_per_layer_matching_in_one_launch_equals_the_per_layer_loop():
    from mvgformer_amd.criterion import criterion_all_layers
    from mvgformer_amd import ops
    inp, meta, t, cams = _criterion_case()
    crit = _criterion(cc.CASES["b2"]["NQ"])
    lg, ps, p2 = (t[k].clone().requires_grad_(True) for k in ("logits", "poses", "poses_2d"))
    launches = []
    orig = ops.hungarian_match
    try:
        ops.hungarian_match = lambda *a, **k: (launches.append(1), orig(*a, **k))[1]
        ld, pairs = criterion_all_layers(crit, lg, ps, p2, meta, None, "linear", cams)
    finally:
        ops.hungarian_match = orig
    assert len(launches) == 1 and pairs[0].shape == (2, 2, 4)                 # ONE matcher call over the L * B problems
    (ld["loss_ce"] + ld["loss_pose_perjoint"] + ld["loss_pose_perprojection_2d"]).backward()
    assert sorted(ld) == sorted(list(R.KEYS) + ["dict_losses_layers", "loss_init"])
    w = R.layer_weights("linear", 2).to(DEV)
    lg2, ps2, p22 = (t[k].clone().requires_grad_(True) for k in ("logits", "poses", "poses_2d"))
    total = 0
    for l in range(2):
        out = {"pred_logits": lg2[l], "pred_poses": {"outputs_coord": ps2[l]}, "pred_poses_2d": {"outputs_coord_2d": p22[l]}}
        losses, indices = crit(out, meta)
        for k in R.KEYS:
            assert torch.equal(ld["dict_losses_layers"][l][k], losses[k]), (l, k)
        for b, (q, g) in enumerate(indices):
            n = int(pairs[2][l, b])
            assert q.tolist() == pairs[0][l, b, :n].tolist() and g.tolist() == pairs[1][l, b, :n].tolist()
        total = total + w[l] * (losses["loss_ce"] + losses["loss_pose_perjoint"] + losses["loss_pose_perprojection_2d"])
    total.backward()
    for a, b in ((lg, lg2), (ps, ps2), (p2, p22)):
        assert float(a.grad.abs().max()) > 0
        assert float((a.grad - b.grad).abs().max()) <= 1e-6 * float(b.grad.abs().max())
    for k in ("loss_ce", "loss_pose_perjoint"):
        want = sum(w[l] * ld["dict_losses_layers"][l][k] for l in range(2))
        assert abs(float(ld[k].detach()) - float(want.detach())) <= 1e-6 * abs(float(want.detach()))


# ---- training -----------------------------------------------------------------------------------------------------------------
def _hungarian_rig():
    """tests/test_train_graph_gpu.py's Rig on its standard (smallest) case, with the head built by
    build_training_head(cfg, matcher=build_matcher_from_cfg(cfg)) for a cfg whose match_method is 'hungarian'"""
    from mvgformer_amd.factory import (build_decoder_for_case, build_matcher_from_cfg, build_optimizer_from_cfg, build_training_head)
    from mvgformer_amd.training import GraphedTrainStep
    from tests import test_train_graph_gpu as TG

    class HRig(TG.Rig):
        def __init__(self):
            case, self.g = TG._data()
            self.dec = build_decoder_for_case(case, DEV, torch.float32)
            self.dec.set_training_dtype(torch.float32)
            cfg = NS(DECODER=NS(match_method="hungarian", decay_method="none", optimizer="adam", lr_linear_proj_mult=0.1,
                                num_instance=case.NQ, num_keypoints=15, d_model=256),
                     NETWORK=NS(IMAGE_SIZE=list(case.img_size)), TRAIN=NS(LR=0.0004, clip_max_norm=0.1),
                     MULTI_PERSON=NS(SPACE_SIZE=list(case.space_size), SPACE_CENTER=list(case.space_center)))
            torch.manual_seed(0)
            self.head, self.weight_dict = build_training_head(cfg, decoder=self.dec, matcher=build_matcher_from_cfg(cfg))
            self.head.to(DEV).train()
            for layer in self.dec.layers:
                layer.dropout2.p = layer.dropout3.p = layer.dropout4.p = 0.0
            for p in self.head.parameters():
                p.requires_grad_(True)
            self.opt = build_optimizer_from_cfg(self.head, cfg)
            self.ops16 = None
            self.runner = GraphedTrainStep(self.head, self.opt, self.weight_dict, self.g.src_views, self.g.meta, self.g.spatial_shapes,
                                           self.g.level_start_index, threshold=0.1)
            self.start = {n: p.detach().clone() for n, p in self.head.named_parameters()}
    return HRig(), TG


def test_forward_train_and_the_captured_step_with_the_hungarian_matcher():
    from mvgformer_amd.criterion import HungarianMatcher
    rig, TG = _hungarian_rig()
    assert isinstance(rig.head.criterion.matcher, HungarianMatcher) and rig.head.criterion.matcher.method == "hungarian"
    other = TG._data(persons=2, gt_seed=3)[1]

    def swap(r, s):
        if s == 1:
            r.runner.load(meta=other.meta)
    want = TG._run(rig, 2, replay=False, before_step=swap)
    rig2, _ = _hungarian_rig()
    rig2.captured()
    got = TG._run(rig2, 2, replay=True, before_step=swap)
    TG._assert_same(got, want, "hungarian: replay vs eager, new ground truth before the second step")
    losses = [float(m[0]) for m in got[0]]
    assert len(set(losses)) == 2 and all(np.isfinite(losses)) and all(float(m[1]) > 0 for m in got[0])
    unchanged, _ = _hungarian_rig()
    same_gt = TG._run(unchanged, 2, replay=False)
    assert not torch.equal(same_gt[0][1][0], got[0][1][0])                    # the new ground truth did reach the graph
    g = unchanged.g
    out, loss_dict = unchanged.head.forward_train(g.src_views, g.meta, g.spatial_shapes, g.level_start_index, threshold=0.1)
    assert len(loss_dict["dict_losses_layers"]) == 2 and all(bool(torch.isfinite(loss_dict[k]).all()) for k in R.KEYS)
    assert len(out["all_logits"]) == 2


# ---- refused arguments ----------------------------------------------------------------------------------------------------------
def test_refused_arguments_launch_nothing():
    NQ, Gmax = 4100, 65                                 # buffers large enough for every dimension claimed below
    poses = torch.zeros((2, NQ * 1, 3), device=DEV)
    gt = torch.zeros((2, Gmax, 1, 3), device=DEV)
    num = torch.zeros(2, dtype=torch.int32, device=DEV)
    logits = torch.zeros((2, NQ, 2), device=DEV)
    ok = dict(NQ=100, Gmax=10, P=2, B=2)

    def refused(what, **kw):
        a = {**ok, **kw}
        rc, out = raw_call(poses, gt, num, a.pop("logits", logits), **a)
        assert rc == BADARG, (what, rc)
        assert _still_poisoned(out["pair_query"], out["pair_gt"], out["pair_count"], out["matched"]), what
        assert "uv" not in out or _still_poisoned(out["uv"]), what
    rc, out = raw_call(poses, gt, num, logits, **ok)    # the base call is fine
    assert rc == 0 and out["pair_count"].tolist() == [0, 0]
    refused("Gmax > 64", Gmax=65, NQ=100)
    refused("NQ > 4096", NQ=4097)
    refused("NQ < Gmax", NQ=9)
    refused("P < 1", P=0)
    refused("P % B", P=3)
    refused("B < 1", B=0, P=0)
    refused("Jp = 0", Jp=0, Jc=0)
    refused("Jc = 65", Jp=65, Jc=65)
    refused("Jp != Jc without a map", Jp=2, Jc=1)
    refused("map repeats", Jp=3, Jc=2, joint_map=[1, 1])
    refused("map out of range", Jp=3, Jc=2, joint_map=[0, 3])
    refused("map negative", Jp=3, Jc=2, joint_map=[-1, 0])
    refused("method 0", method=0)
    refused("method 4", method=4)
    for name in ("poses", "gt", "num", "size", "center", "pair_query", "pair_gt", "pair_count", "matched"):
        refused("NULL " + name, null=(name,))
    refused("misaligned duals", duals_offset=4)
    refused("workspace too small", NQ=4096, Gmax=64, ws_bytes=4096 * 64 * 4 * 2 - 1)
    refused("workspace NULL", NQ=4096, Gmax=64, null=("ws",))
    rc, _ = raw_call(poses, gt, num, None, **ok)        # logits and duals may be NULL
    assert rc == 0
    rc, _ = raw_call(poses, gt, num, logits, duals=False, **ok)
    assert rc == 0
