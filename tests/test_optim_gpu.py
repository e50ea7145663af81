"""GPU checks of the fused optimizer step (csrc/optim.hip, optim.FusedAdam).

Yardstick: what run/train_3d.py runs -- torch.nn.utils.clip_grad_norm_ followed by torch.optim.Adam / AdamW(foreach=False,
fused=False) -- on the CPU in float64 from the same fp32 parameters and the same fp32 gradient sequence.  The same in float32 gives
torch's own fp32 error.  Per state tensor x (p, exp_avg, exp_avg_sq), err(x) = max|x - x64| / max|x64|; the bar of the fused path
is 4 x torch's fp32 err for that tensor, floored at 1e-6 (a different, equally valid fp32 operation order: FMA contraction is on).
The returned norm is an fp64 sum: 1e-6 relative to the fp64 value.  A tensor that is exactly zero in fp64 must be exactly zero.

Measured on MI355X, 10 steps, maximum over the tensors of the synthetic set (torch's fp32 err in brackets; bars 1e-6 .. 2.3e-6):
  adam  clip 0.1 : p 2.31e-07 (2.31e-07)  exp_avg 1.66e-07 (1.94e-07)  exp_avg_sq 2.73e-07 (3.65e-07)  norm 3.4e-08
  adam  no clip  : p 1.92e-07 (1.92e-07)  exp_avg 1.96e-07 (1.01e-07)  exp_avg_sq 2.44e-07 (3.02e-07)  norm 3.4e-08
  adamw clip 0.1 : p 5.77e-07 (5.77e-07)  exp_avg 1.66e-07 (1.94e-07)  exp_avg_sq 2.73e-07 (3.65e-07)  norm 3.4e-08
  adamw no clip  : p 5.40e-07 (5.40e-07)  exp_avg 1.96e-07 (1.01e-07)  exp_avg_sq 2.44e-07 (3.02e-07)  norm 3.4e-08
(the norm's error is the fp32 rounding of the returned scalar).  Every test prints the figures it asserts on (pytest -s).

The synthetic parameter set is the smallest that reaches every path of the kernels (C = optim.CHUNK): a tensor shorter than a
16-byte vector, tails of 1 .. 3 elements, exact chunk fits and chunk crossings, an empty tensor (no chunk), a tensor without a
gradient, one with an all-zero gradient; every p / grad / exp_avg / exp_avg_sq sits inside a larger buffer between guard values,
every third tensor at an address that is not a multiple of 16 bytes (the scalar path)."""
import copy
import functools
import math

import pytest
import torch

from mvgformer_amd.optim import CHUNK, FusedAdam

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = CHUNK
SHAPES = [(1,), (3,), (2, 256), (255,), (256, 256), (C - 1,), (C,), (C + 1,), (3 * C + 5,), (0,)]
SCALES = [1e-4, 1e-3, 1e-2, 0.0, 1e-1, 1.0, 1e1, 1e2, 1e-2, 1.0]      # 0.0: the tensor whose gradient is all zeros
NOGRAD_SHAPE = (7,)                                                      # one further tensor: grad=None
GROUP_OF = [i % 2 for i in range(len(SHAPES))]
LRS = (1e-3, 1e-2)
WDS = {"adam": (0.0, 0.0), "adamw": (1e-4, 1e-2)}
GUARD = 12345.0
STEPS = 10


@functools.lru_cache(maxsize=None)
def _data():
    """fp32 start values and the gradient sequence, on the host; made once and never modified"""
    g = torch.Generator().manual_seed(20)
    p0 = [torch.randn(s, generator=g) for s in SHAPES]
    grads = [[torch.randn(s, generator=g) * sc for s, sc in zip(SHAPES, SCALES)] for _ in range(STEPS)]
    return p0, grads, torch.randn(NOGRAD_SHAPE, generator=g)


def _norm64(gs):
    return math.sqrt(sum(float((x.double() ** 2).sum()) for x in gs))


@functools.lru_cache(maxsize=None)
def _yardstick(kind, max_norm, dtype, steps=STEPS, take=None, lr_scale_at=None):
    """clip_grad_norm_ + torch.optim.Adam / AdamW on the CPU in `dtype`.  take: the indices of the gradient sequence that are
    stepped on (the others are skipped, as the loss guard skips them).  lr_scale_at = (step, factor)."""
    p0, grads, _ = _data()
    ps = [torch.nn.Parameter(x.to(dtype).clone()) for x in p0]
    groups = [{"params": [p for p, gi in zip(ps, GROUP_OF) if gi == k], "lr": LRS[k], "weight_decay": WDS[kind][k]} for k in (0, 1)]
    cls = torch.optim.AdamW if kind == "adamw" else torch.optim.Adam
    opt = cls(groups, lr=LRS[0], foreach=False, fused=False)
    norms, left = [], None
    for s in (range(steps) if take is None else take):
        if lr_scale_at is not None and s == lr_scale_at[0]:
            for gr in opt.param_groups:
                gr["lr"] *= lr_scale_at[1]
        for p, gs in zip(ps, grads[s]):
            p.grad = gs.to(dtype).clone()
        if max_norm > 0:
            norms.append(float(torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False)))
        else:
            norms.append(_norm64(grads[s]))
        opt.step()
        left = [p.grad.clone() for p in ps]
    st = [opt.state[p] for p in ps]
    return {"p": [p.detach().clone() for p in ps], "exp_avg": [x["exp_avg"] for x in st], "exp_avg_sq": [x["exp_avg_sq"] for x in st],
            "norms": norms, "grad": left}


class Guarded:
    """a tensor inside a larger buffer between guard values; `odd`: at an address that is no multiple of 16 bytes"""

    def __init__(self, shape, odd, init=None):
        n = math.prod(shape)
        self.front = 3 if odd else 64
        self.buf = torch.full((self.front + n + 64,), GUARD, device=DEV)
        self.t = self.buf[self.front:self.front + n].view(shape)
        if init is None:
            self.t.zero_()
        else:
            self.t.copy_(init)
        assert n == 0 or (self.t.data_ptr() % 16 != 0) == bool(odd)

    def intact(self):
        n = self.t.numel()
        return bool((self.buf[:self.front] == GUARD).all()) and bool((self.buf[self.front + n:] == GUARD).all())


class Rig:
    """the synthetic parameter set on the device with a FusedAdam over it"""

    def __init__(self, kind, max_norm, zero_grad=False, reverse=False):
        p0, _, pn = _data()
        odd = [i % 3 == 2 for i in range(len(SHAPES))]
        self.P = [Guarded(s, o, x) for s, o, x in zip(SHAPES, odd, p0)]
        self.G = [Guarded(s, o) for s, o in zip(SHAPES, odd)]
        self.M = [Guarded(s, o) for s, o in zip(SHAPES, odd)]
        self.V = [Guarded(s, o) for s, o in zip(SHAPES, odd)]
        self.params = [x.t.requires_grad_(True) for x in self.P]
        for p, g in zip(self.params, self.G):
            p.grad = g.t
        self.nograd = pn.to(DEV).requires_grad_(True)
        members = [[p for p, gi in zip(self.params, GROUP_OF) if gi == k] for k in (0, 1)]
        members[1].append(self.nograd)
        if reverse:
            members = [m[::-1] for m in members]
        groups = [{"params": members[k], "lr": LRS[k], "weight_decay": WDS[kind][k]} for k in (0, 1)]
        self.opt = FusedAdam(groups, lr=LRS[0], decoupled_weight_decay=(kind == "adamw"), clip_max_norm=max_norm, zero_grad=zero_grad)
        for p, m, v in zip(self.params, self.M, self.V):
            self.opt.state[p]["exp_avg"], self.opt.state[p]["exp_avg_sq"] = m.t, v.t
        self.dev_grads = [[x.to(DEV) for x in gs] for gs in _data()[1]]

    def load(self, s):
        for g, x in zip(self.G, self.dev_grads[s]):
            g.t.copy_(x)

    def snapshot(self):
        """device-side clones (no synchronisation)"""
        return {"p": [x.t.detach().clone() for x in self.P], "exp_avg": [x.t.clone() for x in self.M],
                "exp_avg_sq": [x.t.clone() for x in self.V], "grad": [x.t.clone() for x in self.G]}

    def intact(self):
        return all(x.intact() for xs in (self.P, self.G, self.M, self.V) for x in xs)


def _cpu(snap):
    return {k: [x.cpu() for x in v] for k, v in snap.items()}


def _run(kind, max_norm, zero_grad=False, reverse=False, steps=STEPS):
    rig = Rig(kind, max_norm, zero_grad, reverse)
    norms, after_first = [], None
    for s in range(steps):
        rig.load(s)
        norms.append(rig.opt.step())
        if s == 0:
            after_first = rig.snapshot()
    out = _cpu(rig.snapshot())
    out.update(norms=[float(n) for n in norms], norm64=float(rig.opt.last_total_norm()), intact=rig.intact(), step=rig.opt.step_count(), first=_cpu(after_first),
               nograd=rig.nograd.detach().cpu(), nograd_state=dict(rig.opt.state.get(rig.nograd, {})), nograd_grad=rig.nograd.grad)
    return out


_run_cached = functools.lru_cache(maxsize=None)(_run)


def _err(x, ref):
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    diff = float((x.double() - ref).abs().max()) if ref.numel() else 0.0
    return diff / scale if scale > 0 else diff          # a tensor that is exactly zero in fp64: absolute, the bar below is 0


def _check_against_yardstick(got, kind, max_norm, label, **kw):
    y64, y32 = _yardstick(kind, max_norm, torch.float64, **kw), _yardstick(kind, max_norm, torch.float32, **kw)
    worst = {}
    for key in ("p", "exp_avg", "exp_avg_sq"):
        for i, (x, r64, r32) in enumerate(zip(got[key], y64[key], y32[key])):
            zero = r64.numel() == 0 or float(r64.abs().max()) == 0.0
            e, e32 = _err(x, r64), _err(r32, r64)
            bar = 0.0 if zero else max(4 * e32, 1e-6)
            w = worst.get(key, (0.0, 0.0))
            worst[key] = (max(w[0], e), max(w[1], e32))
            assert e <= bar, (label, key, i, SHAPES[i], e, e32, bar)
    print(label, " ".join("%s err %.2e (torch fp32 %.2e)" % (k, v[0], v[1]) for k, v in worst.items()))
    return y64


CASES = [(k, m) for k in ("adam", "adamw") for m in (0.1, 0.0, 1e9)]


@pytest.mark.parametrize("kind,max_norm", CASES)
def test_ten_steps_against_the_fp64_yardstick(kind, max_norm):
    got = _run_cached(kind, max_norm)
    y64 = _check_against_yardstick(got, kind, max_norm, "%s max_norm %g:" % (kind, max_norm))
    nerr = max(abs(a - b) / b for a, b in zip(got["norms"], y64["norms"]))
    print("norm rel err %.2e" % nerr)
    assert nerr <= 1e-6 and got["step"] == STEPS
    for i, (x, r) in enumerate(zip(got["grad"], y64["grad"])):       # the gradients left behind: clip_grad_norm_'s
        if max_norm == 0.1:
            assert _err(x, r) <= 1e-6, (i, _err(x, r))
        else:
            assert torch.equal(x, _data()[1][-1][i])                   # coefficient 1: not a bit changed
    # the tensor without a gradient and its state are untouched
    assert torch.equal(got["nograd"], _data()[2]) and got["nograd_state"] == {} and got["nograd_grad"] is None


def test_zero_grad_leaves_zeros_in_place():
    rig = Rig("adam", 0.1, zero_grad=True)
    ptrs = [p.grad.data_ptr() for p in rig.params]
    for s in range(3):
        rig.load(s)
        rig.opt.step()
    assert all(p.grad is not None and p.grad.data_ptr() == q and not bool(p.grad.any()) for p, q in zip(rig.params, ptrs))
    got = _cpu(rig.snapshot())
    _check_against_yardstick(got, "adam", 0.1, "zero_grad:", steps=3)
    assert rig.intact()


@pytest.mark.parametrize("kind,max_norm", [("adam", 0.1), ("adamw", 0.0)])
def test_guard_values_around_every_tensor_are_intact(kind, max_norm):
    assert _run_cached(kind, max_norm)["intact"]


def test_loss_guard_skips_on_the_device():
    """loss 1e-3 steps; 0, -1 and NaN change no bit of p / exp_avg / exp_avg_sq and leave the count alone; the step after them
    has the bias correction of t = 2 (the yardstick skipped the same gradients).  All under sync debug mode 'error'."""
    rig = Rig("adam", 0.1)
    losses = [torch.tensor(v, device=DEV) for v in (1e-3, 0.0, -1.0, float("nan"), 1e-3)]
    losses[2] = losses[2].reshape(1)                                    # a (1,) tensor is a scalar too
    snaps = []
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for s, loss in enumerate(losses):
            rig.load(s)
            rig.opt.step(loss=loss)
            snaps.append(rig.snapshot())
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for s in (1, 2, 3):
        for key in ("p", "exp_avg", "exp_avg_sq"):
            assert all(torch.equal(a, b) for a, b in zip(snaps[s][key], snaps[0][key])), (s, key)
        assert all(torch.equal(a, b) for a, b in zip(snaps[s]["grad"], rig.dev_grads[s]))    # skipped and zero_grad off: untouched
    assert rig.opt.step_count() == 2
    _check_against_yardstick(_cpu(snaps[4]), "adam", 0.1, "guard:", take=(0, 4))
    assert not all(torch.equal(a, b) for a, b in zip(snaps[4]["p"], snaps[0]["p"]))
    # a skipped step still zeroes the gradients if asked to
    rig = Rig("adam", 0.1, zero_grad=True)
    rig.load(0)
    before = rig.snapshot()
    rig.opt.step(loss=losses[1])
    after = rig.snapshot()
    assert all(torch.equal(a, b) for k in ("p", "exp_avg", "exp_avg_sq") for a, b in zip(before[k], after[k]))
    assert not any(bool(g.any()) for g in after["grad"]) and rig.opt.step_count() == 0 and rig.intact()


def _device_activities(fn):
    """names of every device activity (kernels, copies, memsets) enqueued while fn() runs, from the profiler"""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    events = list(prof.events())
    # a record_function range (torch wraps Optimizer.step in one) is mirrored onto the device timeline under its host name: it is
    # an annotation, not work on the device
    host = {e.name for e in events if e.device_type == DeviceType.CPU}
    return [e.name for e in events if e.device_type == DeviceType.CUDA and e.name not in host]


def test_steady_state_step_is_three_kernels_and_a_new_lr_one_copy():
    rig = Rig("adam", 0.1, zero_grad=True)
    loss = torch.tensor(1e-3, device=DEV)
    for s in range(2):
        rig.load(s)
        rig.opt.step(loss=loss)
    rig.load(2)

    def step():
        torch.cuda.set_sync_debug_mode("error")
        try:
            rig.opt.step(loss=loss)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    steady = _device_activities(step)
    print("steady:", steady)
    assert len(steady) <= 3 and all("optim_" in n for n in steady), steady
    for k in ("optim_sumsq_kernel", "optim_state_kernel", "optim_update_kernel"):      # names may come mangled
        assert sum(k in n for n in steady) == 1, (k, steady)
    rig.opt.param_groups[0]["lr"] *= 0.5
    changed = _device_activities(step)
    print("after an lr change:", changed)
    # the one copy is the group table from pinned host memory; this profiler labels a copy out of pinned (device-visible) host
    # memory 'Memcpy DtoD', so the direction is checked by what arrived: the table on the device holds the new lr
    others = [n for n in changed if "optim_" not in n]
    assert len(others) == 1 and "memcpy" in others[0].lower(), changed
    assert len(changed) == 4 and not any("memset" in n.lower() for n in changed), changed
    assert float(rig.opt._groups_dev[0, 0]) == rig.opt.param_groups[0]["lr"] == LRS[0] * 0.5
    again = _device_activities(step)
    assert len(again) == 3 and all("optim_" in n for n in again), again


def test_two_runs_are_bit_identical_and_the_table_order_does_not_matter():
    """The update of an element depends on the tables' order only through the clip coefficient, an fp32 rounding of the fp64 norm.
    The partial sums are added in chunk-table order, which follows param_groups: the order is NOT canonical, a reversed parameter
    list gives the same norm to 1e-12 relative, not necessarily the same bits."""
    a, b = _run("adamw", 0.1, steps=4), _run("adamw", 0.1, steps=4)
    r = _run("adamw", 0.1, reverse=True, steps=4)
    for key in ("p", "exp_avg", "exp_avg_sq", "grad"):
        assert all(torch.equal(x, y) for x, y in zip(a[key], b[key])), key
        assert all(torch.equal(x, y) for x, y in zip(a[key], r[key])), key
    assert a["norms"] == b["norms"] and a["norm64"] == b["norm64"]
    assert abs(a["norm64"] - r["norm64"]) <= 1e-12 * a["norm64"], (a["norm64"], r["norm64"])


def test_graph_capture_replay_and_lr_change_without_recapture():
    def fresh():
        rig = Rig("adam", 0.1, zero_grad=True)
        rig.loss = torch.tensor(1e-3, device=DEV)
        return rig
    eager = fresh()
    marks = []
    for s in range(4):
        if s == 3:
            eager.opt.param_groups[0]["lr"] *= 0.25
        eager.load(s)
        eager.opt.step(loss=eager.loss)
        marks.append(eager.snapshot())
    rig = fresh()
    rig.load(0)
    # without prepare(): the tables are not on the device, a capture must not build them
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rig.loss + 0                                                    # something to capture: the graph is not empty
        with pytest.raises(RuntimeError, match="prepare"):
            rig.opt.step(loss=rig.loss)
    versions = [p._version for p in rig.params]
    rig.opt.prepare()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        norm = rig.opt.step(loss=rig.loss)
    assert all(p._version > v for p, v in zip(rig.params, versions))
    for s in range(3):
        rig.load(s)
        graph.replay()
    torch.cuda.synchronize()
    got = rig.snapshot()
    for key in ("p", "exp_avg", "exp_avg_sq", "grad"):
        assert all(torch.equal(a, b) for a, b in zip(got[key], marks[2][key])), key
    assert rig.opt.step_count() == 3 and abs(float(norm) - _norm64(_data()[1][2])) <= 1e-6 * float(norm)
    rig.opt.param_groups[0]["lr"] *= 0.25                               # a scheduler step between replays
    rig.opt.prepare()
    rig.load(3)
    graph.replay()
    torch.cuda.synchronize()
    got = rig.snapshot()
    for key in ("p", "exp_avg", "exp_avg_sq"):
        assert all(torch.equal(a, b) for a, b in zip(got[key], marks[3][key])), key
    assert rig.intact()


def _plain_groups(ps):
    return [{"params": [p for p, gi in zip(ps, GROUP_OF) if gi == k], "lr": LRS[k]} for k in (0, 1)]


def _three_steps(ps, opt, first, fused):
    grads = _data()[1]
    for s in range(first, first + 3):
        for p, g in zip(ps, grads[s]):
            if p.grad is None:
                p.grad = g.to(DEV)
            else:
                p.grad.copy_(g)
        if fused:
            opt.step()
        else:
            torch.nn.utils.clip_grad_norm_(ps, 0.1)
            opt.step()


@pytest.mark.parametrize("torch_first", [True, False])
def test_state_dict_interchange_with_torch_adam(torch_first):
    ps = [torch.nn.Parameter(x.to(DEV)) for x in _data()[0]]
    make_torch = lambda: torch.optim.Adam(_plain_groups(ps), lr=LRS[0])                        # noqa: E731
    make_fused = lambda: FusedAdam(_plain_groups(ps), lr=LRS[0], clip_max_norm=0.1)            # noqa: E731
    a = make_torch() if torch_first else make_fused()
    _three_steps(ps, a, 0, fused=not torch_first)
    sd = a.state_dict()
    b = make_fused() if torch_first else make_torch()
    b.load_state_dict(sd)
    _three_steps(ps, b, 3, fused=torch_first)
    st = [b.state[p] for p in ps]
    got = {"p": [p.detach().cpu() for p in ps], "exp_avg": [x["exp_avg"].cpu() for x in st],
           "exp_avg_sq": [x["exp_avg_sq"].cpu() for x in st]}
    _check_against_yardstick(got, "adam", 0.1, "torch -> fused:" if torch_first else "fused -> torch:", steps=6)
    if torch_first:
        assert b.step_count() == 6
    else:
        assert all(float(x["step"]) == 6.0 for x in st if x["exp_avg"].numel())


def test_multistep_lr_changes_the_step_size_at_its_milestone():
    """a constant gradient makes Adam's update lr * g / (|g| + eps): the size of a step is the learning rate"""
    p = torch.nn.Parameter(torch.zeros(1000, device=DEV))
    p.grad = torch.full((1000,), 0.5, device=DEV)
    opt = FusedAdam([p], lr=1e-2)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[2], gamma=0.1)
    deltas = []
    for _ in range(4):
        before = p.detach().clone()
        opt.step()
        sched.step()
        deltas.append(float((p.detach() - before).abs().max()))
    print("step sizes", deltas)
    assert all(abs(d - 1e-2) <= 1e-5 * 1e-2 for d in deltas[:2]) and all(abs(d - 1e-3) <= 1e-5 * 1e-3 for d in deltas[2:]), deltas
    cos = torch.optim.lr_scheduler.CosineAnnealingLR(FusedAdam([p], lr=1e-2), T_max=10)
    cos.optimizer.step()
    cos.step()
    assert cos.optimizer.param_groups[0]["lr"] < 1e-2


def _training_case():
    from types import SimpleNamespace as NS
    from mvgformer_amd.caller import DecoderHead
    from mvgformer_amd.factory import build_criterion_from_cfg, build_decoder_for_case, case_to_device
    from mvgformer_amd.synthetic import add_ground_truth, build_case
    case = build_case("mini5", seed=4, NQ=128, layers=2)
    dec = build_decoder_for_case(case, DEV, torch.float32)
    g = add_ground_truth(case_to_device(case, DEV), [3], Gmax=4, seed=1)
    cfg = NS(DECODER=NS(match_method="KNN", match_method_value=5, decay_method="none", optimizer="adam", lr_linear_proj_mult=0.1),
             NETWORK=NS(IMAGE_SIZE=list(case.img_size)), TRAIN=NS(LR=0.0004, clip_max_norm=0.1),
             MULTI_PERSON=NS(SPACE_SIZE=list(case.space_size), SPACE_CENTER=list(case.space_center)))
    criterion, weight_dict, decay = build_criterion_from_cfg(cfg)
    torch.manual_seed(0)
    head = DecoderHead(dec, case.NQ, 15, 256, case.space_size, case.space_center).to(DEV).set_criterion(criterion, decay)
    # eval(): the autograd path runs because gradients are enabled, without dropout, so a loss is a function of the weights alone
    head.eval()
    for p in head.parameters():
        p.requires_grad_(True)
    return head, dec, g, cfg, weight_dict


def _train_loss(head, g, weight_dict):
    from mvgformer_amd.caller import total_loss
    _, ld = head.forward_train(g.src_views, g.meta, g.spatial_shapes, g.level_start_index, threshold=0.1)
    return total_loss(ld, weight_dict)


def _infer(dec, g):
    with torch.no_grad():
        out = dec(g.tgt, g.reference_points, g.src_views, g.meta, g.spatial_shapes, g.level_start_index, None, query_pos=g.query_pos,
                  threshold=0.1)
    return [o.clone() for o in out[:3]]


def test_a_step_invalidates_the_decoders_operand_caches():
    """The kernels write the parameters through raw pointers; WeightCache is keyed on Parameter._version.  Without the version bump
    in FusedAdam.step the forward after the step is the forward before it."""
    from mvgformer_amd.factory import build_optimizer_from_cfg
    head, dec, g, cfg, weight_dict = _training_case()
    before = _infer(dec, g)                                             # fills the inference caches
    twin = copy.deepcopy(dec)                                           # old values, caches empty
    opt = build_optimizer_from_cfg(head, cfg, lr=1e-2)
    loss1 = _train_loss(head, g, weight_dict)
    loss1.backward()
    opt.step(loss=loss1)
    after = _infer(dec, g)
    with torch.no_grad():
        for a, b in zip(twin.parameters(), dec.parameters()):
            a.copy_(b)
    want = _infer(twin, g)
    assert all(torch.equal(a, b) for a, b in zip(after, want))
    assert not torch.equal(after[0], before[0])
    # the bf16 training copies of the weights are cached the same way
    dec.set_training_dtype(torch.bfloat16)
    la = _train_loss(head, g, weight_dict)
    la.backward()
    opt.step(loss=la)
    lb = _train_loss(head, g, weight_dict)
    print("bf16 losses", float(la), float(lb))
    assert float(la) != float(lb)


def test_twenty_training_steps_end_to_end():
    """forward_train -> total_loss -> backward -> step(loss=total), fp32, on the mini5 head with the reference's two groups.
    forward_train itself synchronises today (caller.sample_space_reference_points uploads the space box and the T-pose from
    pageable host memory on every call), so sync debug mode 'error' is restricted to step()."""
    from mvgformer_amd.factory import build_optimizer_from_cfg
    head, dec, g, cfg, weight_dict = _training_case()
    opt = build_optimizer_from_cfg(head, cfg)
    assert [gr["lr"] for gr in opt.param_groups] == [0.0004, 0.0004 * 0.1] and opt.clip_max_norm == 0.1
    start = {n: p.detach().clone() for n, p in head.named_parameters()}
    losses = []
    for s in range(20):
        total = _train_loss(head, g, weight_dict)
        total.backward()
        if s >= 2:
            torch.cuda.set_sync_debug_mode("error")
        try:
            opt.step(loss=total)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        losses.append(total.detach())
    losses = [float(x) for x in losses]
    had_grad = {n for n, p in head.named_parameters() if p.grad is not None}       # zeroed in place, never dropped
    print("losses", losses[0], losses[-1])
    assert losses[-1] < losses[0], losses
    assert len(had_grad) >= 50 and opt.step_count() == 20
    for n, p in head.named_parameters():
        assert bool(torch.isfinite(p).all()), n
        assert (not torch.equal(p.detach(), start[n])) == (n in had_grad), n
        assert p.grad is None or not bool(p.grad.any()), n              # zero_grad=True: zeroed in place
