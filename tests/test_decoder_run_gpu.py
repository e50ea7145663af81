"""A forward that ends in an exception leaves nothing behind (mvgformer_amd.decoder.DecoderRun).

The per-forward hand-offs between the layers -- the just-in-time hook that issues the next layer's pyramid products, the query term
computed by the previous layer's chain B, the projections written by its triangulation launch -- live in one run object that is
detached from every layer however the forward ends.  Here an ordinary Python exception is raised on the host between two launches
(nothing is provoked on the device), at a point where such a hand-off is installed and not consumed yet; the next forward must be
bit-identical to an untouched one (the decoder is bit-reproducible: test_bf16_decoder_is_deterministic_and_order_independent).
Two layers is the smallest decoder that has a hook, a query-term hand-off and a projection hand-off at all."""
import pytest
import torch

from mvgformer_amd.synthetic import build_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_SETUPS = {}


def _setup(dtype):
    """(decoder, forward, reference outputs of an untouched forward) of the smallest synthetic case, built once per dtype"""
    if dtype not in _SETUPS:
        from mvgformer_amd.decoder import DecoderContext
        from mvgformer_amd.factory import build_decoder_for_case, case_to_device
        case = build_case("cfg1", seed=0, layers=2)
        dec = build_decoder_for_case(case, DEV, dtype=dtype)
        dec.pyramid_jit = "1"
        gc = case_to_device(case, DEV)
        ctx = DecoderContext.build(gc.src_views, gc.spatial_shapes, gc.level_start_index, gc.meta, case.img_size, dtype, 1)
        f32_shape = (gc.tgt.shape[1], ctx.levels.L, ctx.levels.S)
        with torch.no_grad():
            if dtype == torch.bfloat16:
                # the just-in-time schedule with a hook on layer 0 is really in use
                assert dec.fork_side_stream(torch.device(DEV)) is not None
                assert [(len(g), s) for g, s in dec.pyramid_launches(ctx)] == [(1, dec.pyramid_jit_slots)] * len(dec.layers)
            elif dec.layers[0].proj_attn.f32_g_form(*f32_shape):
                print("fp32: the case takes the G form -- side stream without just-in-time hooks")
                assert dec.fork_side_stream(torch.device(DEV), f32_shape) is not None
                assert dec.pyramid_launches(ctx) is None
            else:
                print("fp32: the case does not take the G form -- the pyramid products run inline")
        torch.cuda.synchronize()

        def forward(dec=dec):
            with torch.no_grad():
                out = dec(gc.tgt, gc.reference_points, gc.src_views, gc.meta, gc.spatial_shapes, gc.level_start_index, None,
                          query_pos=gc.query_pos, threshold=0.1)
            torch.cuda.synchronize()
            return out
        _SETUPS[dtype] = (dec, forward, [t.clone() for t in forward()[:4]])
    return _SETUPS[dtype]


@pytest.mark.parametrize("dtype, where", [(torch.bfloat16, "sampler"), (torch.bfloat16, "triangulation"),
                                          (torch.float32, "triangulation")])
def test_forward_that_raises_leaves_no_state_behind(dtype, where):
    """sampler: layer 0 raises in front of its sampler -- the hook that issues layer 1's pyramid products is installed and never
    fires.  triangulation: layer 0 raises behind its triangulation launch -- layer 1's query term and projections are handed over
    and never consumed (fp32: the f32h chain B's hand-off, a side stream without hooks)."""
    dec, forward, ref = _setup(dtype)
    layer0 = dec.layers[0]

    def raise_at_once(*args, **kwargs):
        raise RuntimeError("injected")

    def triangulate_then_raise(st, ctx, real=layer0.forward_triangulate):
        real(st, ctx)
        raise RuntimeError("injected")
    obj, name, wrapper = ((layer0.proj_attn, "native_sample", raise_at_once) if where == "sampler" else
                          (layer0, "forward_triangulate", triangulate_then_raise))
    setattr(obj, name, wrapper)         # shadows the method on this instance only
    try:
        with pytest.raises(RuntimeError, match="injected"):
            forward()
    finally:
        delattr(obj, name)
    torch.cuda.synchronize()
    assert all(l._run is None for l in dec.layers)
    assert not dec.products.pending() and all(l.proj_attn.products is dec.products for l in dec.layers)
    got = forward()
    for x, y in zip(ref, got[:4]):
        assert torch.equal(x, y)


def test_fp32_ahead_products_never_alias_the_inline_pair():
    """fp32 forwards with the products inline (ONE pair per stream for all layers), then ahead on the side stream (one pair per layer,
    all alive at once), then inline again, on a decoder whose owner starts empty -- so the inline pair exists first and an ahead
    buffer that reused it would be shared by both layers.  Each forward is bit-identical to the first of its kind, nothing is pending
    afterwards, and the ahead buffers are other tensors than the inline pair, which survives them."""
    import copy
    dec0, forward, ref = _setup(torch.float32)
    dec = copy.deepcopy(dec0)       # the same weights, a fresh and empty owner
    assert dec.products.tensors() == [] and dec.overlap_pyramid and dec.overlap_pyramid_f32
    outs, held = [], []
    try:
        for overlap in (False, True, False):
            dec.overlap_pyramid = overlap
            outs.append([t.clone() for t in forward(dec)[:4]])
            assert not dec.products.pending()
            held.append(dec.products.tensors())
    finally:
        dec.overlap_pyramid = True
    inline, both = held[0], held[1]
    assert len(inline) == 2 and len(both) == 2 + 2 * len(dec.layers)        # (the case takes the G-sampling form: there are products)
    ids = lambda ts: {id(t) for t in ts}
    assert ids(inline) < ids(both) and ids(held[2]) == ids(both)            # the pair survives; the third forward allocates nothing
    assert len(ids(both)) == len(both) == len({t.data_ptr() for t in both})     # ahead buffers: other tensors, other memory
    for x, y in zip(outs[0], outs[2]):
        assert torch.equal(x, y)
    for x, y in zip(ref, outs[1]):          # ahead is what the shared decoder's untouched forward ran
        assert torch.equal(x, y)
