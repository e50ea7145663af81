"""Host side of the live-view table: the table builder (ordering, padding, counts, refusals), the option checks of the
post-processing pipeline around it, and validate's --view-subsets parser."""
import numpy as np
import pytest
import torch

from mvgformer_amd.decoder import DecoderContext, live_view_table, refuse_live_views


def test_table_ordering_padding_and_counts():
    idx, n = live_view_table([True, False, True, True, False], 2, 5)
    assert idx.dtype == np.int32 and n.dtype == np.int32 and idx.shape == (2, 5) and n.shape == (2,)
    assert idx.tolist() == [[0, 2, 3, -1, -1]] * 2 and n.tolist() == [3, 3]
    mask = np.array([[0, 0, 0, 1, 0, 0, 0, 0, 0], [1, 1, 0, 1, 1, 0, 1, 0, 1]], dtype=bool)
    idx, n = live_view_table(mask, 2, 9)
    assert idx.tolist() == [[3] + [-1] * 8, [0, 1, 3, 4, 6, 8, -1, -1, -1]] and n.tolist() == [1, 6]
    for same in (torch.from_numpy(mask), mask.astype(np.int64), mask.tolist()):
        i2, n2 = live_view_table(same, 2, 9)
        assert np.array_equal(i2, idx) and np.array_equal(n2, n)
    idx, n = live_view_table([True] * 4, 3, 4)
    assert idx.tolist() == [[0, 1, 2, 3]] * 3 and n.tolist() == [4, 4, 4]


def test_table_refusals():
    with pytest.raises(ValueError, match="stream 1 has no live view"):
        live_view_table([[True, False], [False, False]], 2, 2)
    for bad in ([True] * 3, [[True] * 4] * 3, [[[True] * 4]]):
        with pytest.raises(ValueError, match="shape"):
            live_view_table(bad, 2, 4)
    with pytest.raises(ValueError, match="bool"):
        live_view_table([0.5, 1.0, 0.0, 1.0], 1, 4)
    with pytest.raises(ValueError, match="bool"):
        live_view_table([2, 1, 0, 1], 1, 4)
    with pytest.raises(TypeError, match="host"):
        live_view_table(torch.ones(4, dtype=torch.bool, device="meta"), 1, 4)


def test_context_keeps_one_pair_of_buffers():
    ctx = DecoderContext(None, torch.zeros(6, 40), V=3, B=2)
    assert ctx.live is None and len(ctx.tensors()) == 1
    refuse_live_views(ctx, "x")
    refuse_live_views(None, "x")
    ctx.set_live_views([True, False, True])
    view_idx, n_live = ctx.live
    assert view_idx.dtype == torch.int32 and view_idx.tolist() == [[0, 2, -1]] * 2 and n_live.tolist() == [2, 2]
    assert len(ctx.tensors()) == 3
    ctx.set_live_views([[False, True, False], [True, True, True]])
    assert ctx.live[0] is view_idx and ctx.live[1] is n_live            # refilled in place: a captured graph addresses them
    assert view_idx.tolist() == [[1, -1, -1], [0, 1, 2]] and n_live.tolist() == [1, 3]
    with pytest.raises(ValueError):
        ctx.set_live_views([False] * 3)
    assert view_idx.tolist() == [[1, -1, -1], [0, 1, 2]]                 # a refused mask leaves the table as it was
    with pytest.raises(NotImplementedError, match="somebody"):
        refuse_live_views(ctx, "somebody")
    assert ctx.set_live_views(None).live is None
    assert len(ctx.tensors()) == 3                                       # off: the buffers stay pinned ...
    ctx.set_live_views([True, True, False])
    assert ctx.live[0] is view_idx and ctx.live[1] is n_live and view_idx.tolist() == [[0, 1, -1]] * 2       # ... and come back


def test_postprocess_view_weights_and_checks():
    from mvgformer_amd.postprocess import PostProcess
    post = PostProcess.__new__(PostProcess)         # the two methods read nothing but the table
    post.live = None
    refs2d = torch.zeros(2, 4, 30, 2)
    assert post.view_weights(refs2d) is None
    view_idx = torch.tensor([[0, 2, 3, -1], [1, -1, -1, -1]], dtype=torch.int32)
    n_live = torch.tensor([3, 1], dtype=torch.int32)
    assert post.set_live_views((view_idx, n_live)) is post
    w = post.view_weights(refs2d)
    third = (torch.ones(()) / torch.full((), 3.0)).item()
    assert w.dtype == torch.float32 and tuple(w.shape) == (2, 4, 30) and w.is_contiguous()
    assert w[0, :, 0].tolist() == [third, 0.0, third, third] and w[1, :, 7].tolist() == [0.0, 1.0, 0.0, 0.0]
    assert bool((w == w[:, :, :1]).all())
    with pytest.raises(ValueError):
        post.set_live_views((view_idx.long(), n_live))
    with pytest.raises(ValueError):
        post.set_live_views((view_idx, n_live[:1]))
    with pytest.raises(ValueError):
        post.view_weights(torch.zeros(2, 5, 30, 2))
    assert post.set_live_views(None).view_weights(refs2d) is None


def test_view_subsets_parser():
    from mvgformer_amd.validate import parse_view_subsets
    assert parse_view_subsets("0,1,2;0,2,4;0,1,2,3,4", 5) == [(0, 1, 2), (0, 2, 4), (0, 1, 2, 3, 4)]
    assert parse_view_subsets(" 4, 0 ;2", 5) == [(0, 4), (2,)]
    for bad in ("0,1;", "0,0,1", "0,5", "-1,2", "a,b", ""):
        with pytest.raises(ValueError, match="view-subsets"):
            parse_view_subsets(bad, 5)
