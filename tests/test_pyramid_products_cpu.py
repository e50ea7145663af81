"""mvgformer_amd.projattn.PyramidProducts -- the one owner of the per-layer pyramid products (value planes and G): host logic only,
on CPU tensors.  Reuse policy of the buffers, the two tables that never share a tensor, the ready state machine, what a captured
graph pins and compares; and DecoderContext, which declares every field it carries."""
import os
import re

import torch

from mvgformer_amd.decoder import DecoderContext
from mvgformer_amd.projattn import ProjAttn, PyramidProducts, WeightCache

CPU = torch.device("cpu")
F32, BF16 = torch.float32, torch.bfloat16
N, S, C = 2, 24, 256


def _layers(n=2):
    return [ProjAttn(256, 1, 8, 8, "ablation_not_use_rayconv") for _ in range(n)]


def _same(a, b):
    return all(x is y and x.data_ptr() == y.data_ptr() for x, y in zip(a, b))


def _disjoint(a, b):
    return not ({id(t) for t in a} & {id(t) for t in b}) and not ({t.data_ptr() for t in a} & {t.data_ptr() for t in b})


def test_same_key_and_shape_return_the_same_tensors():
    P, (pa, pb) = PyramidProducts(), _layers()
    for dtype, ahead, shape in ((BF16, False, (N, 8, S, 32)), (BF16, True, (N, 8, S, 32)), (F32, True, (N, S, C)), (F32, False, (N, S, C))):
        P = PyramidProducts()
        first = P.buffers(pa, dtype, N, S, C, CPU, ahead=ahead, stream=7)
        assert tuple(first[0].shape) == shape and tuple(first[1].shape) == (N * S, 192)
        assert first[0].dtype == first[1].dtype == dtype and first[0].device == first[1].device == CPU
        sig = P.signature()
        assert _same(first, P.buffers(pa, dtype, N, S, C, CPU, ahead=ahead, stream=7)) and P.signature() == sig
        # another shape, dtype or device under the same key: new tensors, the old ones leave the tables
        other = P.buffers(pa, dtype, N, S + 8, C, CPU, ahead=ahead, stream=7)
        assert _disjoint(first, other) and tuple(other[1].shape) == (N * (S + 8), 192) and P.signature() != sig
        assert P.tensors() == list(other)
        moved = P.buffers(pa, dtype, N, S + 8, C, torch.device("meta"), ahead=ahead, stream=7)
        assert moved[0] is not other[0] and moved[1] is not other[1] and moved[0].device.type == "meta"
    # the per-layer slot holds ONE pair: the other dtype replaces it
    P = PyramidProducts()
    b16 = P.buffers(pa, BF16, N, S, C, CPU)
    f32 = P.buffers(pa, F32, N, S, C, CPU, ahead=True)
    assert _disjoint(b16, f32) and f32[0].dtype == F32 and P.tensors() == list(f32)
    assert not _same(b16, P.buffers(pa, BF16, N, S, C, CPU))
    # another layer has its own
    assert _disjoint(P.buffers(pa, BF16, N, S, C, CPU), P.buffers(pb, BF16, N, S, C, CPU)) and len(P.tensors()) == 4


def test_inline_fp32_pair_is_shared_per_stream():
    P, (pa, pb) = PyramidProducts(), _layers()
    one = P.buffers(pa, F32, N, S, C, CPU, ahead=False, stream=1)
    assert _same(one, P.buffers(pb, F32, N, S, C, CPU, ahead=False, stream=1))          # two layers, one stream: one pair
    two = P.buffers(pa, F32, N, S, C, CPU, ahead=False, stream=2)                       # another stream: another pair
    assert _disjoint(one, two) and _same(one, P.buffers(pb, F32, N, S, C, CPU, ahead=False, stream=1))
    assert len(P.tensors()) == 4
    # bf16 products are per layer, inline or not
    assert _disjoint(P.buffers(pa, BF16, N, S, C, CPU, ahead=False, stream=1), P.buffers(pb, BF16, N, S, C, CPU, ahead=False, stream=1))


def test_an_ahead_pair_is_never_an_inline_pair():
    P, layers = PyramidProducts(), _layers(3)
    inline = P.buffers(layers[0], F32, N, S, C, CPU, ahead=False, stream=1)     # the inline table first ...
    ahead = [P.buffers(pa, F32, N, S, C, CPU, ahead=True) for pa in layers]      # ... then ahead buffers of the same shape
    for i, pair in enumerate(ahead):
        assert _disjoint(pair, inline) and all(_disjoint(pair, other) for other in ahead[:i])
    assert _same(inline, P.buffers(layers[1], F32, N, S, C, CPU, ahead=False, stream=1))
    assert all(_same(pair, P.buffers(pa, F32, N, S, C, CPU, ahead=True)) for pa, pair in zip(layers, ahead))
    live = P.tensors()
    assert len(live) == 8 and len({id(t) for t in live}) == 8 and len({t.data_ptr() for t in live}) == 8    # every live buffer, once


class _Event:
    def __init__(self):
        self.waits = 0

    def wait(self, stream=None):
        self.waits += 1


def test_ready_state_machine():
    P, (pa, pb) = PyramidProducts(), _layers()
    bufs = {l: P.buffers(l, BF16, N, S, C, CPU) for l in (pa, pb)}
    assert P.take(pa) is None and not P.pending() and not P.pending(pa)            # not produced: the layer computes inline
    ev = _Event()
    P.produced([pa], ev)
    assert P.pending() and P.pending(pa) and not P.pending(pb) and P.take(pb) is None
    assert _same(P.take(pa), bufs[pa]) and ev.waits == 1
    assert _same(P.take(pa), bufs[pa]) and ev.waits == 2                           # armed until the join
    P.join(None, keep=False)
    assert P.take(pa) is None and not P.pending() and ev.waits == 2                 # dropped
    P.produced([pa, pb], ev)                                                        # one event for a group of layers
    P.join(None, keep=True)
    assert P.pending() and _same(P.take(pa), bufs[pa]) and _same(P.take(pb), bufs[pb]) and ev.waits == 2   # joined: no event wait
    P.join(None, keep=True)
    assert P.pending(pa) and P.pending(pb)
    P.join(None)
    assert not P.pending() and P.take(pa) is None and P.take(pb) is None
    P.join(None, keep=True)                                                         # keeps what is there: nothing
    assert not P.pending()
    assert P.signature() == tuple((t.data_ptr(), t.dtype, tuple(t.shape)) for pair in bufs.values() for t in pair)   # state is not buffers


def test_deepcopy_is_a_fresh_empty_owner():
    import copy
    P, (pa, pb) = PyramidProducts(), _layers()
    pa.products = pb.products = P
    P.buffers(pa, F32, N, S, C, CPU, ahead=False, stream=1)
    P.buffers(pa, BF16, N, S, C, CPU)
    P.produced([pa], _Event())
    ca, cb = copy.deepcopy([pa, pb])
    assert ca.products is cb.products and ca.products is not P
    assert ca.products.tensors() == [] and ca.products.signature() == () and not ca.products.pending()
    assert len(P.tensors()) == 4 and P.pending(pa)


def test_weight_cache_lists_its_operand_tensors():
    wc, w = WeightCache(), torch.nn.Parameter(torch.ones(4, 4))
    a = wc.get("a", (w,), F32)
    b = wc.get("b", (w,), torch.float16, lambda t: (t * 2, 0.5))      # (tensor, host-side scalar)
    assert b[1] == 0.5 and [id(t) for t in wc.tensors()] == [id(a), id(b[0])]


def test_decoder_context_declares_every_field():
    ctx = DecoderContext()
    declared = {"levels", "cams", "V", "B", "dtype", "feat", "_buffer", "packed_event", "train_Pm", "train_key", "train_ref"}
    assert set(vars(ctx)) == declared
    assert all(getattr(ctx, k) is None for k in declared - {"V", "B", "dtype"}) and ctx.tensors() == []
    ctx.cams, ctx.train_ref = torch.zeros(3), torch.zeros(2)
    assert [id(t) for t in ctx.tensors()] == [id(ctx.cams), id(ctx.train_ref)]


def test_no_reach_in_for_private_state_from_the_runners():
    """decoder.py, training.py, caller.py and serving.py read no underscore attribute of a context or a ProjAttn through getattr,
    give a context no attribute from outside, and the names of the scattered state are gone from the package"""
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mvgformer_amd")
    reach = re.compile(r"""getattr\(\s*(?:[\w.]*ctx|[\w.]*context|[\w.]*proj_attn|[\w.]*\bpa|self)\s*,\s*["']_""")
    gone = re.compile(r"\b_vp\b|\b_G\b|_vp_event|_f32_pool|_packed_feat|(?<!fork)_side_stream|_share_f32_pool|_buffer_ptrs|_train_cache|_train_ref"
                      r"|_packed_event|_plane_buffer|_g_buffer|_wait_pyramid")
    declared = set(vars(DecoderContext()))
    for name in ("decoder.py", "training.py", "caller.py", "serving.py", "projattn.py"):
        with open(os.path.join(root, name)) as f:
            src = f.read()
        assert not reach.findall(src), (name, reach.findall(src))
        assert not gone.findall(src), (name, gone.findall(src))
        assigned = set(re.findall(r"\b(?:self\.)?ctx\.(\w+)\s*=[^=]", src))
        assert assigned <= declared, (name, assigned - declared)
