"""The live-view table (DecoderContext.set_live_views, DQDecoder.forward(view_live=...)): a forward with some views masked out
gives, bit for bit, what the same decoder object gives when it is run on the live views alone -- all five outputs of all layers,
with zeros in the 2D slots of the dead views -- on the bf16 fused, the fp32 fused and the unfused fp32 path.  Cases: mini5 (V = 5,
NQ = 12, 2 layers) and mini9 (V = 9, NQ = 8: the one shape where a problem's views wrap onto a second round of the eight lanes
of the triangulation, and where the 5-view subset run takes chain B's V <= 5 path while the masked run walks groups of 8)."""
import contextlib

import pytest
import torch

from mvgformer_amd.synthetic import build_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ["bf16", "f32", "unfused"]
_CACHE = {}


@contextlib.contextmanager
def _mode(mode):
    """the compute dtype of a path; "unfused" is fp32 with the library's f32_split knob off (reference-arithmetic GEMMs, one launch
    per GEMM / row op), restored afterwards"""
    from mvgformer_amd import _lib
    _lib.load()
    if mode == "unfused":
        with _lib.tuning(f32_split=0):
            yield torch.float32
    else:
        yield torch.bfloat16 if mode == "bf16" else torch.float32


def _rig(name, mode, B=1, NQ=None, valid_fraction=None, seed=3):
    """(decoder, case on the device), built once per configuration and left unchanged"""
    from mvgformer_amd.factory import build_decoder_for_case, case_to_device
    key = (name, mode == "bf16", B, NQ, valid_fraction, seed)
    if key not in _CACHE:
        case = build_case(name, B=B, seed=seed, NQ=NQ, layers=2, valid_fraction=valid_fraction)
        dec = build_decoder_for_case(case, DEV, dtype=torch.bfloat16 if mode == "bf16" else torch.float32)
        _CACHE[key] = (dec, case_to_device(case, DEV))
    return _CACHE[key]


def _forward(dec, g, src_views=None, meta=None, thr=0.1, **kw):
    with torch.no_grad():
        hs, refs, r2d, p2d, cls = dec(g.tgt, g.reference_points, g.src_views if src_views is None else src_views,
                                      g.meta if meta is None else meta, g.spatial_shapes, g.level_start_index, None,
                                      query_pos=g.query_pos, threshold=thr, **kw)
    torch.cuda.synchronize()
    return [hs.clone(), refs.clone(), r2d.clone(), p2d.clone(), torch.stack(list(cls)).clone()]


def _subset(g, views):
    """the rig of the live views alone: src_views is view-major (image v * B + b), meta a list over views"""
    B = g.tgt.shape[0]
    idx = torch.tensor([v * B + b for v in views for b in range(B)], device=DEV)
    return [s.index_select(0, idx).contiguous() for s in g.src_views], [g.meta[v] for v in views]


def _mask(V, views):
    return [v in views for v in range(V)]


def _check(masked, sub, views, V, streams=None):
    """masked: outputs on all V slots with a table; sub: outputs of the run on `views` alone.  streams: compare these batch elements only"""
    views = list(views)
    dead = [v for v in range(V) if v not in views]
    b = slice(None) if streams is None else streams
    for k in (0, 1):
        assert torch.equal(masked[k][:, b], sub[k][:, b]), ("hs", "refs")[k]
    assert torch.equal(masked[4][:, b], sub[4][:, b]), "class_prob"
    for k in (2, 3):
        assert torch.equal(masked[k][:, b][:, :, views], sub[k][:, b]), ("ref2d", "proj2d")[k - 2]
        if dead:
            assert not bool(masked[k][:, b][:, :, dead].any()), "dead slots must be exactly zero"
    for t in masked:
        assert bool(torch.isfinite(t[:, b]).all())


@pytest.mark.parametrize("mode", MODES)
def test_all_views_live_equals_no_table(mode):
    with _mode(mode):
        dec, g = _rig("mini5", mode)
        plain = _forward(dec, g)
        masked = _forward(dec, g, view_live=[True] * 5)
    for a, b in zip(plain, masked):
        assert torch.equal(a, b)


@pytest.mark.parametrize("views", [(0, 2, 4), (1, 2, 3), (3, 4), (2,)], ids=lambda v: "".join(map(str, v)))
@pytest.mark.parametrize("mode", MODES)
def test_mini5_subsets(mode, views):
    """(1, 2, 3) is the case a zero-weight mask over all views gets wrong: lanes 1..3 instead of 0..2 feed max8 / add8 and the
    eight-way Gram sum, and the DPP trees group by lane."""
    with _mode(mode):
        dec, g = _rig("mini5", mode)
        src, meta = _subset(g, views)
        sub = _forward(dec, g, src, meta)
        masked = _forward(dec, g, view_live=_mask(5, views))
    _check(masked, sub, views, 5)


@pytest.mark.parametrize("views,thr", [((0, 1, 3, 4, 6), 0.1), ((0, 1, 2, 4, 5, 6, 7, 8), 0.1), (tuple(range(9)), 0.1),
                                       ((0, 1, 3, 4, 6), 1.5)], ids=["5of9", "8of9", "9of9", "5of9_none_valid"])
@pytest.mark.parametrize("mode", MODES)
def test_mini9_subsets(mode, views, thr):
    """valid_fraction 0.5; the last case runs at a threshold no probability reaches, so the forced query (0, 0) rule decides"""
    with _mode(mode):
        dec, g = _rig("mini9", mode, valid_fraction=0.5)
        src, meta = _subset(g, views)
        sub = _forward(dec, g, src, meta, thr=thr)
        masked = _forward(dec, g, thr=thr, view_live=_mask(9, views))
    passed = sub[4][..., 1] > thr
    if thr > 1.0:
        assert not bool(passed.any())
        assert bool(sub[1][:, 0, :15].any()) and not bool(sub[1][:, 0, 15:].any())        # query (0, 0) alone was triangulated
    else:
        assert bool(passed.any()) and not bool(passed.all())
    _check(masked, sub, views, 9)


@pytest.mark.parametrize("mode", MODES)
def test_two_streams(mode):
    """B = 2, NQ = 13: NQ * 15 = 195 rows per stream is no multiple of the chain-B tiles (30 / 60 rows of 2 / 4 queries), so one tile
    holds rows of both streams and divides by both counts.  Same subset in both streams: the B = 2 subset run.  A subset per stream:
    stream b equals stream b of the B = 2 run in which both streams carry subset b (both streams have valid queries in every layer,
    so the batch-wide any-valid rule is not in play)."""
    subsets, thr = [(0, 2, 4), (1, 3)], 0.01       # (the second layer's probabilities of this rig lie between 0.0006 and 0.04)
    with _mode(mode):
        dec, g = _rig("mini5", mode, B=2, NQ=13, valid_fraction=0.5)
        subs = [_forward(dec, g, *_subset(g, views), thr=thr) for views in subsets]
        same = _forward(dec, g, thr=thr, view_live=_mask(5, subsets[0]))
        mixed = _forward(dec, g, thr=thr, view_live=[_mask(5, views) for views in subsets])
    for s in subs:
        passed = s[4][..., 1] > thr
        assert bool(passed.any(-1).all()), "every layer of every stream needs a valid query"
    _check(same, subs[0], subsets[0], 5)
    for b, views in enumerate(subsets):
        _check(mixed, subs[b], views, 5, streams=slice(b, b + 1))


@pytest.mark.parametrize("mode", MODES)
def test_dead_views_are_not_read(mode):
    """the dead views' feature maps are NaN and their camera records zeros: still the subset run's bits, and no NaN anywhere"""
    from mvgformer_amd.decoder import DecoderContext
    views, V = (0, 2, 3), 5
    with _mode(mode) as dt:
        dec, g = _rig("mini5", mode)
        sub = _forward(dec, g, *_subset(g, views))
        src = [s.clone() for s in g.src_views]
        ctx = DecoderContext.prepare(g.spatial_shapes, g.level_start_index, g.meta, dec.layers[0].img_size, dt, 1, torch.device(DEV))
        for v in range(V):
            if v not in views:
                for s in src:
                    s[v].fill_(float("nan"))
                ctx.cams[v].zero_()
        ctx.set_live_views(_mask(V, views))
        masked = _forward(dec, g, src, context=ctx)
    _check(masked, sub, views, V)


_KNOBS = [("bf16", "auto_small", 0, False), ("bf16", "chain_rm", 64, True), ("bf16", "chain_rm", 256, False),
          ("f32", "f32h_rows", 32, True), ("f32", "f32h_rows", 64, True)]


@pytest.mark.parametrize("mode,key,value,exact", _KNOBS, ids=["%s=%d" % (k, v) for _, k, v, _ in _KNOBS])
def test_tuning_knobs_select_the_live_variants(mode, key, value, exact):
    """the knob values tests/test_hip_parity.py walks for the chains, and f32h_rows: with a table, each gives what the default
    gives with that table, under the rule that test states for the knob -- bit-identical, or for the two variants that change the
    order of an fp32 sum, its bf16 bars.  Only auto_small (chain_b_kernel's 32- / 64-row tiles) and f32h_rows (the fp32 chain B's
    two tile sizes) reach kernels with a LIVE variant -- at mini9 both variants of both are run; chain_rm selects among chain A's
    variants, which have none, and is walked because the issue lists it; the lane-parallel triangulation is not instantiated
    and has no knob."""
    from mvgformer_amd import _lib
    views = (0, 1, 3, 4, 6)
    with _mode(mode):
        dec, g = _rig("mini9", mode, valid_fraction=0.5)
        ref = _forward(dec, g, view_live=_mask(9, views))
        with _lib.tuning(**{key: value}):
            got = _forward(dec, g, view_live=_mask(9, views))
    if exact:
        for a, b in zip(ref, got):
            assert torch.equal(a, b), key
    else:
        assert float((got[0] - ref[0]).abs().max()) < 4e-2
        assert float((got[1] - ref[1]).norm(dim=-1).max()) < 6.0 and float((got[2] - ref[2]).abs().max()) < 0.5
    assert not bool(got[2][:, :, [2, 5, 7, 8]].any())


def test_init_self_attention_passes_the_table_through():
    from mvgformer_amd.factory import build_decoder_for_case
    views = (1, 2, 3)
    _, g = _rig("mini5", "bf16")
    dec = build_decoder_for_case(build_case("mini5", seed=3, layers=2), DEV, dtype=torch.bfloat16)
    for layer in dec.layers:
        layer.init_self_attention = True
    sub = _forward(dec, g, *_subset(g, views))
    masked = _forward(dec, g, view_live=_mask(5, views))
    _check(masked, sub, views, 5)
    plain, _ = _rig("mini5", "bf16")
    assert not torch.equal(masked[0], _forward(plain, g, view_live=_mask(5, views))[0])       # the block did run


def _training_rig():
    """head with a criterion, FusedAdam and a GraphedTrainStep on mini5 (the rig of tests/test_train_graph_gpu.py, fp32, NQ = 32)"""
    from types import SimpleNamespace as NS
    from mvgformer_amd.caller import DecoderHead
    from mvgformer_amd.factory import build_criterion_from_cfg, build_decoder_for_case, build_optimizer_from_cfg, case_to_device
    from mvgformer_amd.synthetic import add_ground_truth
    from mvgformer_amd.training import GraphedTrainStep
    case = build_case("mini5", seed=4, NQ=32, layers=2)
    g = add_ground_truth(case_to_device(case, DEV), [3], Gmax=4, seed=1)
    dec = build_decoder_for_case(case, DEV, torch.float32)
    cfg = NS(DECODER=NS(match_method="KNN", match_method_value=5, decay_method="none", optimizer="adam", lr_linear_proj_mult=0.1),
             NETWORK=NS(IMAGE_SIZE=list(case.img_size)), TRAIN=NS(LR=0.0004, clip_max_norm=0.1),
             MULTI_PERSON=NS(SPACE_SIZE=list(case.space_size), SPACE_CENTER=list(case.space_center)))
    criterion, weight_dict, decay = build_criterion_from_cfg(cfg)
    head = DecoderHead(dec, case.NQ, 15, 256, case.space_size, case.space_center).to(DEV).set_criterion(criterion, decay)
    head.train()
    for p in head.parameters():
        p.requires_grad_(True)
    opt = build_optimizer_from_cfg(head, cfg)
    step = GraphedTrainStep(head, opt, weight_dict, g.src_views, g.meta, g.spatial_shapes, g.level_start_index, threshold=0.1)
    return head, g, step


def test_training_refuses_a_table_before_any_launch(monkeypatch):
    """DecoderHead.forward_train and GraphedTrainStep (eager step, capture, replay) on a context with a table: NotImplementedError
    that names the caller, and not one entry point of the library was launched by then"""
    from mvgformer_amd import ops
    from mvgformer_amd.decoder import DecoderContext
    head, g, step = _training_rig()
    ctx = DecoderContext.prepare(g.spatial_shapes, g.level_start_index, g.meta, head.decoder.layers[0].img_size, torch.float32, 1,
                                 torch.device(DEV)).set_live_views([True, False, True, True, True])
    step.ctx.set_live_views([True, True, False, True, True])
    seen = []
    real = ops._launch
    monkeypatch.setattr(ops, "_launch", lambda symbol, *a, **k: (seen.append(symbol), real(symbol, *a, **k))[1])
    with pytest.raises(NotImplementedError, match="DecoderHead.forward_train"):
        head.forward_train(g.src_views, g.meta, g.spatial_shapes, g.level_start_index, threshold=0.1, context=ctx)
    for call in (step.eager, step.capture, step.replay):
        with pytest.raises(NotImplementedError, match="GraphedTrainStep"):
            call()
    assert seen == [] and step.graph is None
    # the table switched off: the step runs (and launches)
    step.ctx.set_live_views(None)
    total = step.eager()[0]
    torch.cuda.synchronize()
    assert bool(torch.isfinite(total)) and seen


def test_refusals(monkeypatch):
    from mvgformer_amd import dist as D
    from mvgformer_amd import ops
    from mvgformer_amd.decoder import DecoderContext
    dec, g = _rig("mini5", "bf16")
    ctx = DecoderContext.prepare(g.spatial_shapes, g.level_start_index, g.meta, dec.layers[0].img_size, torch.bfloat16, 1,
                                 torch.device(DEV))
    with pytest.raises(TypeError):
        ctx.set_live_views(torch.ones(5, dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError):
        ctx.set_live_views([False] * 5)
    with pytest.raises(ValueError):
        ctx.set_live_views([True] * 4)
    with pytest.raises(ValueError):
        ctx.set_live_views([[True] * 5] * 2)
    assert ctx.live is None
    ctx.set_live_views([True, False, True, True, True])
    assert all(any(t.data_ptr() == p.data_ptr() for p in ctx.tensors()) for t in ctx.live)
    seen = []
    real = ops._launch
    monkeypatch.setattr(ops, "_launch", lambda symbol, *a, **k: (seen.append(symbol), real(symbol, *a, **k))[1])
    with pytest.raises(NotImplementedError, match="forward_autograd"):
        with torch.enable_grad():
            dec(g.tgt.clone().requires_grad_(True), g.reference_points, g.src_views, g.meta, g.spatial_shapes, g.level_start_index,
                None, query_pos=g.query_pos, threshold=0.1, context=ctx)
    with pytest.raises(NotImplementedError, match="sharded_decoder_forward"):
        D.sharded_decoder_forward(dec, g.tgt, g.reference_points, g.src_views, g.meta, g.spatial_shapes, g.level_start_index,
                                  g.query_pos, 0.1, context=ctx)
    with pytest.raises(NotImplementedError, match="GraphedShardedDecoder"):
        D.GraphedShardedDecoder(dec, g.tgt, g.reference_points, g.src_views, g.query_pos, ctx, 0.1, g.NQ)
    with pytest.raises(NotImplementedError, match="ShardedDecoder"):
        D.SpeculativeShardedDecoder(dec, g.tgt, g.reference_points, g.src_views, g.query_pos, ctx, 0.1, g.NQ)
    assert seen == []                   # every refusal came before any launch
    # None switches the table off again: the launches without one; the buffers stay and the next table refills them
    held = ctx.live
    ctx.set_live_views(None)
    assert ctx.live is None and all(any(t is p for p in ctx.tensors()) for t in held)
    for a, b in zip(_forward(dec, g, context=ctx), _forward(dec, g)):
        assert torch.equal(a, b)
