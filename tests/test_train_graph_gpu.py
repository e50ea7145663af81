"""GPU checks of training.GraphedTrainStep: the whole training step (forward_train -> total_loss -> backward -> FusedAdam.step) as
one HIP graph, against the identical step run eagerly from the same initial state, bit for bit; and of training.TrainOperands, the
bf16 operands that the device rewrites inside the step.

The case is tests/test_criterion_gpu.py::test_forward_train_end_to_end's: mini5, seed 4, NQ = 128, 2 layers, 3 persons in 4
ground-truth slots, KNN 5.  Dropout is 0 wherever bits are compared.  capture() itself takes optimizer steps (its warm-up), so a
rig that is to be compared with an eager run restores its initial state in place after the capture -- parameters, moments, step
count -- and calls refresh_operands(), the documented route for a write to the parameters outside the graph."""
from types import SimpleNamespace as NS

import pytest
import torch

from mvgformer_amd.caller import DecoderHead
from mvgformer_amd.factory import (build_criterion_from_cfg, build_decoder_for_case, build_graphed_train_step,
                                   build_optimizer_from_cfg, case_to_device)
from mvgformer_amd.synthetic import add_ground_truth, build_case
from mvgformer_amd.training import GraphedTrainStep, TrainOperands

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16


def _data(case_seed=4, persons=3, gt_seed=1):
    case = build_case("mini5", seed=case_seed, NQ=128, layers=2)
    return case, add_ground_truth(case_to_device(case, DEV), [persons], Gmax=4, seed=gt_seed)


class Rig:
    """head + optimizer (+ operands) on the standard case, always from the same initial state (seeded weights and embeddings)"""

    def __init__(self, tdt, dropout=0.0, attach=True, zero_grad=True, data=None):
        case, self.g = data if data is not None else _data()
        # the weights are ALWAYS the standard case's: another batch (data=) changes inputs, ground truth and cameras only
        wcase = case if data is None else build_case("mini5", seed=4, NQ=128, layers=2)
        self.dec = build_decoder_for_case(wcase, DEV, F32)
        self.dec.set_training_dtype(tdt)
        cfg = NS(DECODER=NS(match_method="KNN", match_method_value=5, decay_method="none", optimizer="adam", lr_linear_proj_mult=0.1),
                 NETWORK=NS(IMAGE_SIZE=list(case.img_size)), TRAIN=NS(LR=0.0004, clip_max_norm=0.1),
                 MULTI_PERSON=NS(SPACE_SIZE=list(case.space_size), SPACE_CENTER=list(case.space_center)))
        criterion, self.weight_dict, decay = build_criterion_from_cfg(cfg)
        torch.manual_seed(0)
        self.head = DecoderHead(self.dec, case.NQ, 15, 256, case.space_size, case.space_center).to(DEV).set_criterion(criterion, decay)
        self.head.train()
        for layer in self.dec.layers:
            layer.dropout2.p = layer.dropout3.p = layer.dropout4.p = dropout
        for p in self.head.parameters():
            p.requires_grad_(True)
        self.opt = build_optimizer_from_cfg(self.head, cfg)
        if not zero_grad:
            self.opt.zero_grad_after_step = False
        self.ops16 = None
        if tdt == BF16 and attach:
            self.ops16 = TrainOperands(self.head)
            self.opt.attach_operands(self.ops16)
        self.runner = GraphedTrainStep(self.head, self.opt, self.weight_dict, self.g.src_views, self.g.meta, self.g.spatial_shapes,
                                       self.g.level_start_index, threshold=0.1, operands=self.ops16)
        self.start = {n: p.detach().clone() for n, p in self.head.named_parameters()}

    def captured(self):
        """capture, then back to the initial state in place"""
        self.runner.capture()
        return self.restore()

    def restore(self):
        with torch.no_grad():
            for n, p in self.head.named_parameters():
                p.copy_(self.start[n])
            for st in self.opt.state.values():
                st["exp_avg"].zero_()
                st["exp_avg_sq"].zero_()
        self.opt._set_step(0)
        self.runner.refresh_operands()
        return self

    def state(self):
        torch.cuda.synchronize()
        named = dict(self.head.named_parameters())
        out = {"p/" + n: p.detach().clone() for n, p in named.items()}
        for n, p in named.items():
            st = self.opt.state.get(p, {})
            if "exp_avg" in st:
                out["m/" + n], out["v/" + n] = st["exp_avg"].clone(), st["exp_avg_sq"].clone()
        return out


def _run(rig, n, replay, before_step=None):
    """n steps -> (per-step [loss, norm] as host floats' bit patterns, final state)"""
    marks = []
    for s in range(n):
        if before_step is not None:
            before_step(rig, s)
        total, _, norm, _ = rig.runner.replay() if replay else rig.runner.eager()
        marks.append((total.detach().clone(), norm.detach().clone()))
    return marks, rig.state()


def _max_diff(a, b):
    assert sorted(a) == sorted(b)
    worst = (0.0, None)
    for k in a:
        d = float((a[k].double() - b[k].double()).abs().max()) if a[k].numel() else 0.0
        if d > worst[0]:
            worst = (d, k)
    return worst


def _assert_same(got, want, what):
    (gm, gs), (wm, ws) = got, want
    d, k = _max_diff(gs, ws)
    dl = max(abs(float(a[0]) - float(b[0])) for a, b in zip(gm, wm))
    dn = max(abs(float(a[1]) - float(b[1])) for a, b in zip(gm, wm))
    print("%s: max |state diff| %.3e (%s), max |loss diff| %.3e, max |norm diff| %.3e; losses %s"
          % (what, d, k, dl, dn, [float(a[0]) for a in gm]))
    assert all(torch.equal(gs[key], ws[key]) for key in ws), (what, d, k)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(gm, wm)), (what, dl, dn)


@pytest.mark.parametrize("tdt", [F32, BF16], ids=["fp32", "bf16"])
def test_three_replays_equal_three_eager_steps_bit_for_bit(tdt):
    """tests 1 and 2 of the change: first eager against eager (is the step deterministic at all?), then replay against eager.  bf16:
    after the replays every adopted W16 / W16^T is the cast of its CURRENT master weight -- the in-graph refresh; a graph that kept
    its capture-time operands would leave the eager run at the second step."""
    e1 = _run(Rig(tdt), 3, replay=False)
    e2 = _run(Rig(tdt), 3, replay=False)
    _assert_same(e2, e1, "eager vs eager")
    rig = Rig(tdt).captured()
    grads = rig.runner._grads()
    got = _run(rig, 3, replay=True)
    _assert_same(got, e1, "replay vs eager")
    assert rig.runner._grads() == grads
    losses = [float(m[0]) for m in got[0]]
    assert len(set(losses)) == 3 and all(torch.isfinite(m[0]) and float(m[1]) > 0 for m in got[0])       # the weights do move
    assert rig.opt.step_count() == 3
    if tdt == BF16:
        assert len(rig.ops16.entries) == 8 * len(rig.dec.layers)
        name_of = {id(p): n for n, p in rig.head.named_parameters()}
        moved = 0
        for cache, key, params, w16, w16t in rig.ops16.entries:
            w = torch.cat([p.detach() for p in params], 0)
            assert torch.equal(w16, w.to(BF16)) and torch.equal(w16t, w.t().contiguous().to(BF16)), key
            moved += not torch.equal(w16, torch.cat([rig.start[name_of[id(p)]] for p in params], 0).to(BF16))
            # and the caches hand out exactly these tensors for the parameters as they are now
            assert cache.get(key, params, BF16) is w16 and cache.get(key + "^T", params, BF16) is w16t
        print("operands whose bf16 bits left their initial values:", moved, "of", len(rig.ops16.entries))
        assert 2 * moved >= len(rig.ops16.entries)           # they are not the capture-time (= initial) copies


def test_bf16_eager_steps_with_device_operands_equal_those_with_torch_casts():
    """test 3: no graph.  attach_operands replaces the per-step torch casts by the refresh launch: the same rounding, so the same
    parameters; a following no-grad inference forward sees the new weights (the version bump and the re-stamp of the adopted
    entries did not hide the update from the inference path's cache keys)"""
    def infer(rig):
        g = rig.g
        with torch.no_grad():
            out = rig.dec(g.tgt, g.reference_points, g.src_views, g.meta, g.spatial_shapes, g.level_start_index, None,
                          query_pos=g.query_pos, threshold=0.1)
        return [o.clone() for o in out[:3]]
    with_ops, without = Rig(BF16, attach=True), Rig(BF16, attach=False)
    assert without.ops16 is None and without.opt._operands is None
    before = infer(with_ops)                                   # fills the inference caches with the initial weights
    infer(without)
    a = _run(with_ops, 3, replay=False)
    b = _run(without, 3, replay=False)
    _assert_same(a, b, "device operands vs torch casts")
    after, want = infer(with_ops), infer(without)
    assert all(torch.equal(x, y) for x, y in zip(after, want))
    assert not torch.equal(after[0], before[0])


def test_new_ground_truth_and_cameras_between_replays():
    """test 4: load() + set_cameras() with another batch (other maps, other ground truth, other cameras), then one replay == one
    eager step of a fresh rig built on that batch"""
    other = _data(case_seed=9, persons=2, gt_seed=3)
    rig = Rig(F32).captured()
    first = _data()[1]
    assert not torch.equal(other[1].meta[0]["joints_3d"], first.meta[0]["joints_3d"])
    assert not torch.equal(other[1].meta[1]["camera"]["T"], first.meta[1]["camera"]["T"])
    rig.runner.load(src_views=other[1].src_views, meta=other[1].meta).set_cameras(other[1].meta)
    got = _run(rig, 1, replay=True)
    want = _run(Rig(F32, data=other), 1, replay=False)
    _assert_same(got, want, "replay on a new batch vs eager")
    unchanged = _run(Rig(F32), 1, replay=False)
    assert not torch.equal(unchanged[0][0][0], got[0][0][0])                        # the new batch did reach the graph


def test_lr_change_between_replays_through_prepare():
    """test 5: a scheduler step between replays: param_groups change on the host, prepare() re-sends the group table, no re-capture"""
    def schedule(rig, s):
        if s == 2:
            for gr in rig.opt.param_groups:
                gr["lr"] *= 0.25
            rig.opt.prepare()
    want = _run(Rig(F32), 3, replay=False, before_step=schedule)
    plain = _run(Rig(F32), 3, replay=False)
    got = _run(Rig(F32).captured(), 3, replay=True, before_step=schedule)
    _assert_same(got, want, "replay vs eager, lr * 0.25 before step 3")
    assert not all(torch.equal(plain[1][k], want[1][k]) for k in want[1])


def test_guards():
    """test 6"""
    rig = Rig(BF16, attach=False)
    with pytest.raises(RuntimeError, match="TrainOperands"):
        rig.runner.capture()
    rig = Rig(BF16, attach=True)
    rig.runner.operands = None                              # attached to the optimizer, but not handed to the runner
    with pytest.raises(RuntimeError, match="TrainOperands"):
        rig.runner.capture()
    with pytest.raises(ValueError, match="zero_grad=True"):
        Rig(F32, zero_grad=False)
    rig = Rig(F32)
    with pytest.raises(TypeError, match="FusedAdam"):
        GraphedTrainStep(rig.head, torch.optim.Adam(rig.head.parameters(), lr=1e-4), rig.weight_dict, rig.g.src_views, rig.g.meta)
    rig.captured()
    ptrs = [p.grad.data_ptr() for p in rig.head.parameters() if p.grad is not None]
    assert len(ptrs) >= 50
    for _ in range(3):
        rig.runner.replay()
    torch.cuda.synchronize()
    assert [p.grad.data_ptr() for p in rig.head.parameters() if p.grad is not None] == ptrs
    assert all(not bool(p.grad.any()) for p in rig.head.parameters() if p.grad is not None)          # zeroed in place by the step
    moved = next(p for p in rig.head.parameters() if p.grad is not None)
    moved.grad = torch.zeros_like(moved.grad)
    with pytest.raises(RuntimeError, match="grad moved"):
        rig.runner.replay()


def test_dropout_stays_torchs_under_replay():
    """test 7: dropout 0.1: three replays, finite loss and parameters.  Observation printed (pytest -s), not asserted: whether two
    replays from the SAME parameters draw different masks (torch advances the Philox offset of a captured graph per replay)."""
    rig = Rig(F32, dropout=0.1).captured()
    first = float(rig.runner.replay()[0])
    rig.restore()
    again = float(rig.runner.replay()[0])
    print("dropout 0.1: loss of two replays from the same parameters: %.9g, %.9g -> masks %s"
          % (first, again, "differ" if first != again else "are the same"))
    marks, state = _run(rig, 3, replay=True)
    assert all(bool(torch.isfinite(m[0])) and bool(torch.isfinite(m[1])) for m in marks)
    assert all(bool(torch.isfinite(t).all()) for t in state.values())


def test_factory_entry_builds_attaches_and_captures():
    rig = Rig(BF16, attach=False)
    step = build_graphed_train_step(rig.head, rig.opt, rig.g)
    assert isinstance(step, GraphedTrainStep) and step.graph is not None
    assert isinstance(rig.opt._operands, TrainOperands) and step.operands is rig.opt._operands
    total, loss_dict, norm, out = step.replay()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(total)) and float(norm) > 0 and "pred_logits" in out and "loss_ce" in loss_dict
