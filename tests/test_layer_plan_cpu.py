"""DQDecoderLayer.plan: the one place where a layer's sampler form, its fused chains, the pair binning, the masked-tile skipping
and the hand-offs to its neighbours are decided -- as a table over the switches (no GPU: the plan is host logic)."""
import pytest
import torch

from mvgformer_amd import ops

BF16, F32 = torch.bfloat16, torch.float32
LQ = 150
LEVELS = ops.Levels([[20, 20], [10, 10], [5, 5]], [0, 400, 500])        # S = 525 > LQ * L = 450
SMALL = ops.Levels([[8, 8], [4, 4], [2, 2]], [0, 64, 80])               # S = 84 <= 450


def _layer(dt, attrs=(), **kw):
    from tests.test_selfattn_cpu import _layer as build
    layer = build(**kw).set_compute_dtype(dt)
    for name, value in dict(attrs).items():
        obj, _, attr = ("layer." + name).rpartition(".")
        setattr(layer if obj == "layer" else layer.proj_attn, attr, value)
    return layer


def _f32_split(value):
    """the library's f32_split knob (bench.py --f32-gemm exact sets 0), restored on the way out; None = as it is"""
    from mvgformer_amd import _lib
    return _lib.tuning(**({} if value is None else {"f32_split": value}))


# (id, dtype, layer arguments, attributes set afterwards, f32_split knob, levels) ->
#     (sampler, chain A, chain B, pyramid products ahead on the side stream, ... in a grouped launch)
TABLE = [
    ("bf16-defaults", BF16, {}, {}, None, LEVELS, ("gsamp", "bf16", "bf16", True, True)),
    ("bf16-chains-off", BF16, {}, {"use_fused_chains": False}, None, LEVELS, ("gsamp", None, None, False, True)),
    ("bf16-fast-path-off", BF16, {}, {"proj_attn.use_fast_path": False}, None, LEVELS, ("gather", "bf16", "bf16", False, False)),
    ("bf16-ffn-512", BF16, {"open_forward_ffn": True, "d_ffn": 512}, {}, None, LEVELS, ("gsamp", "bf16", None, True, True)),
    ("fp32-defaults", F32, {}, {}, None, LEVELS, ("gfused_f32h", "f32h", "f32h", True, False)),
    ("fp32-chains-off", F32, {}, {"use_fused_chains_f32": False}, None, LEVELS, ("gfused_f32h", None, None, True, False)),
    ("fp32-split-0", F32, {}, {}, 0, LEVELS, ("gather", None, None, False, False)),
    ("fp32-split-0-few-pyramid-rows", F32, {}, {}, 0, SMALL, ("gfused_f32", None, None, True, False)),
    ("fp32-g-sampling-off", F32, {}, {"proj_attn.g_sampling_f32": False}, None, LEVELS, ("gather", None, "f32h", False, False)),
    ("fp32-33-joints", F32, {"num_joints": 33}, {}, None, LEVELS, ("gfused_f32h", "f32h", None, True, False)),
]


@pytest.mark.parametrize("dt, kw, attrs, knob, levels, want", [row[1:] for row in TABLE], ids=[row[0] for row in TABLE])
def test_plan_table(dt, kw, attrs, knob, levels, want):
    layer = _layer(dt, attrs, **kw)
    # the environment's switches are not what is under test
    layer.proj_attn.g_sampling_f32 = attrs.get("proj_attn.g_sampling_f32", "auto")
    with _f32_split(knob):
        plan = layer.plan(dt, LQ, levels)
        assert (plan.sampler, plan.chain_a, plan.chain_b, plan.products_ahead, plan.grouped) == want
        assert layer.plan(dt, LQ, (levels.L, levels.S)) == plan            # the levels as (L, S)
        assert plan.dt == dt
        # the names other code and the tools ask keep their meaning
        pa = layer.proj_attn
        assert pa.uses_fast_path(dt) == (plan.sampler == "gsamp")
        if dt == F32:
            assert pa.f32_g_form(LQ, levels.L, levels.S) == plan.sampler.startswith("gfused")
            assert pa.f32_fused_active() == (knob != 0)
        assert pa.sampler_form(dt, LQ, levels.L, levels.S) == plan.sampler
        assert plan.sampler in pa.sampler_forms(dt)


def test_plan_is_not_cached():
    layer = _layer(BF16)
    assert layer.plan(BF16, LQ, LEVELS).chain_a == "bf16"
    layer.use_fused_chains = False
    assert layer.plan(BF16, LQ, LEVELS).chain_a is None
    layer32 = _layer(F32)
    with _f32_split(0):
        assert layer32.plan(F32, LQ, LEVELS).chain_b is None
    assert layer32.plan(F32, LQ, LEVELS).chain_b == "f32h"


@pytest.mark.parametrize("dt", [BF16, F32])
def test_pair_binning(dt):
    layer = _layer(dt)
    layer.proj_attn.sort_pairs = "layer"
    assert layer.plan(dt, LQ, LEVELS).binning == "layer"                # per layer by default
    assert layer.plan(dt, 65536, LEVELS).binning == "layer"
    assert layer.plan(dt, 65537, LEVELS).binning is None                # no order above 65536 queries
    layer.proj_attn.sort_pairs = "first"
    assert layer.plan(dt, LQ, LEVELS).binning == ("first" if dt == BF16 else "layer")   # once per forward: the bf16 fused path
    assert layer.plan(dt, 65537, LEVELS).binning is None
    layer.use_fused_chains = layer.use_fused_chains_f32 = False
    assert layer.plan(dt, LQ, LEVELS).binning == "layer"                # the G-sampler alone bins per layer
    layer.use_fused_chains = layer.use_fused_chains_f32 = True
    layer.proj_attn.sort_pairs = False
    assert layer.plan(dt, LQ, LEVELS).binning is None
    # gather form without a fused chain A and without masked-tile skipping: nothing reads an order
    layer.proj_attn.sort_pairs = "layer"
    layer.proj_attn.use_fast_path, layer.proj_attn.g_sampling_f32 = False, False
    layer.use_fused_chains = False
    assert layer.plan(dt, LQ, LEVELS).binning is None
    assert layer.plan(dt, 8192, LEVELS).binning == (None if dt == BF16 else "layer")    # fp32: the masked-tile skipping reads one


def test_masked_tiles_are_skipped_only_on_the_unfused_fp32_path_inside_its_window():
    unfused = _layer(F32, {"use_fused_chains_f32": False})
    unfused.proj_attn.sort_pairs = "layer"
    assert [unfused.plan(F32, Lq, LEVELS).skip_masked for Lq in (LQ, 8191, 8192, 65536, 65537)] == [False, False, True, True, False]
    with _f32_split(0):
        assert _layer(F32).plan(F32, 8192, LEVELS).skip_masked
    gather = _layer(F32, {"proj_attn.g_sampling_f32": False})           # chain A unfused, chain B fused
    gather.proj_attn.sort_pairs = "layer"
    assert gather.plan(F32, 8192, LEVELS).skip_masked
    unfused.skip_masked_f32 = False
    assert not unfused.plan(F32, 8192, LEVELS).skip_masked
    unfused.skip_masked_f32 = True
    unfused.proj_attn.sort_pairs = False
    assert not unfused.plan(F32, 8192, LEVELS).skip_masked
    fused = _layer(F32)
    fused.proj_attn.sort_pairs = "layer"
    assert fused.plan(F32, 8192, LEVELS).chain_a == "f32h" and not fused.plan(F32, 8192, LEVELS).skip_masked
    for attrs in ({}, {"use_fused_chains": False}):
        assert not _layer(BF16, attrs).plan(BF16, 8192, LEVELS).skip_masked


def test_query_term_of_the_next_layer():
    tgt = torch.zeros(1, LQ, 256)
    for dt, path in ((BF16, "bf16"), (F32, "f32h")):
        a, b = _layer(dt), _layer(dt)
        b.proj_attn.g_sampling_f32 = "auto"
        assert b.plan(dt, LQ, LEVELS).query_term == path
        # taken: the position term as rows + the next layer's operands for this path (stand-ins: the real ones need the device)
        b.proj_attn.query_term_weights = lambda dtype, p: ("operands", dtype, p)
        qp, *rest = a._next_query_term(b, path, tgt, tgt + 1, LEVELS)
        assert qp.shape == (LQ, 256) and bool((qp == 1).all()) and rest == ["operands", dt, path]
        assert a._next_query_term(b, path, tgt, None, LEVELS) == (None, "operands", dt, path)
        if dt == BF16:      # (building the operand itself needs the device: ops.gsamp_column_order)
            assert _layer(dt, init_self_attention=True).plan(dt, LQ, LEVELS).query_term is None
        # refused: a layer that attends first, a layer on another dtype, no next layer, a query_pos of another shape
        assert a._next_query_term(_layer(dt, init_self_attention=True), path, tgt, tgt, LEVELS) is None
        assert a._next_query_term(_layer(F32 if dt == BF16 else BF16), path, tgt, tgt, LEVELS) is None
        assert a._next_query_term(None, path, tgt, tgt, LEVELS) is None
        assert a._next_query_term(b, path, tgt, tgt[:, :1], LEVELS) is None
        # refused: the next layer's chain A is not the matching path
        assert a._next_query_term(_layer(dt, {"use_fused_chains": False, "use_fused_chains_f32": False}), path, tgt, tgt, LEVELS) is None
        assert a._next_query_term(b, "f32h" if path == "bf16" else "bf16", tgt, tgt, LEVELS) is None
    gather = _layer(F32, {"proj_attn.g_sampling_f32": False})
    assert gather.plan(F32, LQ, LEVELS).chain_b == "f32h" and gather.plan(F32, LQ, LEVELS).query_term is None
    assert gather._next_query_term(gather, "f32h", tgt, tgt, LEVELS) is None


def test_fp32_without_a_shape():
    """the shape is read where it decides, and only there: g_sampling_f32 = "auto" without the fused fp32 kernels"""
    layer = _layer(F32)
    layer.proj_attn.g_sampling_f32 = "auto"
    assert layer.plan(F32).sampler == "gfused_f32h" and layer.proj_attn.sampler_forms(F32) == ("gfused_f32h",)
    with _f32_split(0):
        assert layer.proj_attn.sampler_forms(F32) == ("gfused_f32", "gather")
        with pytest.raises(ValueError, match="decides by the shape"):
            layer.plan(F32)
        assert [layer.plan(F32, sampler=form).sampler for form in layer.proj_attn.sampler_forms(F32)] == ["gfused_f32", "gather"]
        layer.proj_attn.g_sampling_f32 = False
        assert layer.plan(F32).sampler == "gather" and layer.proj_attn.sampler_forms(F32) == ("gather",)
    assert _layer(BF16).proj_attn.sampler_forms(BF16) == ("gsamp",)
