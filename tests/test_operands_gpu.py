"""GPU checks of mvg_refresh_operands (csrc/operands.hip): the bf16 copy and the transposed bf16 copy of fp32 matrices, bit for bit
against torch's own casts w.to(bfloat16) and w.t().contiguous().to(bfloat16) -- the casts projattn.WeightCache runs and this
kernel replaces.  Shapes: the smallest at which each path of the kernel can go wrong (one tile; many tiles in both aspect ratios;
two records into one buffer with row / column offsets; edge tiles with leading dimensions that are no multiple of 8; a single
element; a source that is not 16-byte aligned; a record with only one of the destinations).  Every destination sits inside a
larger buffer between guard values."""
import ctypes

import pytest
import torch

from mvgformer_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 0x5A5A                      # bf16 bits of the guard value
PAD = 64                            # guard elements in front of and behind every destination

F32_MAX = 3.4028234663852886e38
HALF_DOWN = 1.0 + 2.0 ** -8         # exactly between the bf16 values 1.0 and 1.0078125: ties to even -> 1.0
HALF_UP = 1.0 + 3.0 * 2.0 ** -8     # exactly between 1.0078125 and 1.015625: ties to even -> 1.015625
SPECIALS = [0.0, -0.0, float("inf"), float("-inf"), F32_MAX, -F32_MAX, 1e-40, -1e-40, HALF_DOWN, HALF_UP, -HALF_DOWN,
            3.3895313892515355e38]  # the last: bf16 max + half an ulp, the smallest value that rounds up to Inf


def _values(shape, seed, offset=0):
    """random normal values over 20 binades with the special values planted where the matrix has room; a view that starts `offset`
    elements into its storage"""
    g = torch.Generator().manual_seed(seed)
    n = shape[0] * shape[1]
    flat = torch.randn(n, generator=g) * torch.exp2(torch.randint(-10, 11, (n,), generator=g).float())
    if n >= 4 * len(SPECIALS):
        where = torch.randperm(n, generator=g)[:len(SPECIALS)]
        flat[where] = torch.tensor(SPECIALS, dtype=torch.float32)
    store = torch.zeros(n + offset, dtype=torch.float32)
    store[offset:] = flat
    return store.to(DEV)[offset:].view(shape)


def _guarded(rows, cols):
    """a (rows, cols) bf16 destination inside a buffer of guard values -> (buffer as int16 bits, the view)"""
    buf = torch.full((rows * cols + 2 * PAD,), GUARD, dtype=torch.int16, device=DEV)
    return buf, buf[PAD:PAD + rows * cols].view(torch.bfloat16).view(rows, cols)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _launch(records):
    """records: [(src, dst or None, dst_ld, dstT or None, dstT_ld)] with dst / dstT given as (tensor whose data_ptr is the record's
    pointer).  Builds both tables as the header lays them out and launches once."""
    rows, tiles = [], []
    for i, (src, dst, dst_ld, dstT, dstT_ld) in enumerate(records):
        N, K = src.shape
        rows.append((src.data_ptr(), N, K, src.stride(0), 0 if dst is None else dst.data_ptr(), dst_ld,
                     0 if dstT is None else dstT.data_ptr(), dstT_ld))
        tiles += [(i, t) for t in range(-(-N // 64) * -(-K // 64))]
    rec = torch.tensor(rows, dtype=torch.int64).to(DEV)
    til = torch.tensor(tiles, dtype=torch.int32).to(DEV)
    ops.refresh_operands(rec, til)
    torch.cuda.synchronize()
    return rec, til


def _check(src, got, got_t):
    want = src.to(torch.bfloat16)
    want_t = src.t().contiguous().to(torch.bfloat16)
    if got is not None:
        assert torch.equal(got, want) and torch.equal(_bits(got), _bits(want))          # the second: -0 and +0 apart
    if got_t is not None:
        assert torch.equal(got_t, want_t) and torch.equal(_bits(got_t), _bits(want_t))


def _guards_intact(buf, n):
    return bool((buf[:PAD] == GUARD).all()) and bool((buf[PAD + n:] == GUARD).all())


@pytest.mark.parametrize("shape,offset", [((64, 64), 0), ((1024, 256), 0), ((256, 1024), 0), ((70, 100), 0), ((1, 1), 0),
                                          ((64, 64), 1), ((128, 192), 3), ((65, 8), 0), ((8, 65), 0)])
def test_copy_and_transposed_copy_are_torchs_bits(shape, offset):
    """one record.  offset: the source starts that many elements into its storage (not 16-byte aligned: the element path)"""
    N, K = shape
    src = _values(shape, seed=N * 131 + K + offset, offset=offset)
    assert (src.data_ptr() % 16 != 0) == (offset % 4 != 0)
    buf, dst = _guarded(N, K)
    buf_t, dst_t = _guarded(K, N)
    _launch([(src, dst, K, dst_t, N)])
    _check(src, dst, dst_t)
    assert _guards_intact(buf, N * K) and _guards_intact(buf_t, N * K)
    first, first_t = dst.clone(), dst_t.clone()
    dst.zero_()
    dst_t.zero_()
    _launch([(src, dst, K, dst_t, N)])                                          # two runs: the same bits
    assert torch.equal(_bits(dst), _bits(first)) and torch.equal(_bits(dst_t), _bits(first_t))


def test_destinations_that_are_not_16_byte_aligned_take_the_element_path():
    """full tiles and friendly leading dimensions, but destination pointers 2 bytes off a 16-byte boundary"""
    src = _values((128, 64), seed=9)
    buf = torch.full((128 * 64 + 2 * PAD + 1,), GUARD, dtype=torch.int16, device=DEV)
    buf_t = buf.clone()
    dst = buf[PAD + 1:PAD + 1 + 128 * 64].view(torch.bfloat16).view(128, 64)
    dst_t = buf_t[PAD + 1:PAD + 1 + 128 * 64].view(torch.bfloat16).view(64, 128)
    assert dst.data_ptr() % 16 == 2 and dst_t.data_ptr() % 16 == 2
    _launch([(src, dst, 64, dst_t, 128)])
    _check(src, dst, dst_t)
    for b in (buf, buf_t):
        assert bool((b[:PAD + 1] == GUARD).all()) and bool((b[PAD + 1 + 128 * 64:] == GUARD).all())


def test_two_records_into_one_buffer():
    """ProjAttn's [sampling_offsets; attention_weights]: (128, 256) + (64, 256) -> one (192, 256) / (256, 192) pair; the second record's
    dst starts at row 128, its dstT at column 128 with dstT_ld = 192 != N"""
    a, b = _values((128, 256), seed=1), _values((64, 256), seed=2)
    buf, dst = _guarded(192, 256)
    buf_t, dst_t = _guarded(256, 192)
    _launch([(a, dst, 256, dst_t, 192), (b, dst[128:], 256, dst_t[:, 128:], 192)])
    _check(torch.cat([a, b], 0), dst, dst_t)
    assert _guards_intact(buf, 192 * 256) and _guards_intact(buf_t, 192 * 256)


def test_a_record_with_one_destination_only():
    src = _values((128, 128), seed=3)
    buf, dst = _guarded(128, 128)
    buf_t, dst_t = _guarded(128, 128)
    _launch([(src, dst, 128, None, 0), (src, None, 0, dst_t, 128)])
    _check(src, dst, dst_t)
    assert _guards_intact(buf, 128 * 128) and _guards_intact(buf_t, 128 * 128)
    # and each alone leaves the other buffer untouched
    buf2, only = _guarded(70, 100)
    small = _values((70, 100), seed=4)
    _launch([(small, only, 100, None, 0)])
    _check(small, only, None)
    assert _guards_intact(buf2, 7000)


def test_a_nan_stays_a_nan():
    src = _values((64, 64), seed=5)
    src[3, 5] = float("nan")
    src[40, 63] = -float("nan")
    buf, dst = _guarded(64, 64)
    buf_t, dst_t = _guarded(64, 64)
    _launch([(src, dst, 64, dst_t, 64)])
    nan = torch.isnan(src)
    assert torch.equal(torch.isnan(dst), nan) and torch.equal(torch.isnan(dst_t), nan.t())
    keep = ~nan
    want = src.to(torch.bfloat16)
    assert torch.equal(_bits(dst)[keep], _bits(want)[keep]) and torch.equal(_bits(dst_t)[keep.t()], _bits(want.t())[keep.t()])


def test_argument_errors_return_non_zero_and_launch_nothing():
    lib = _lib.load()
    src = _values((64, 64), seed=6)
    buf, dst = _guarded(64, 64)
    rec = torch.tensor([(src.data_ptr(), 64, 64, 64, dst.data_ptr(), 64, 0, 0)], dtype=torch.int64).to(DEV)
    til = torch.tensor([(0, 0)], dtype=torch.int32).to(DEV)
    stream = _lib.stream_ptr()
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)          # noqa: E731
    bad = [(None, 1, p(til), 1), (p(rec), 1, None, 1), (p(rec), 0, p(til), 1), (p(rec), -1, p(til), 1), (p(rec), 1, p(til), -1),
           (p(rec, 4), 1, p(til), 1), (p(rec), 1, p(til, 4), 1)]
    for a, n, b, m in bad:
        assert lib.mvg_refresh_operands(a, n, b, m, stream) != 0
    assert lib.mvg_refresh_operands(p(rec), 1, p(til), 0, stream) == 0                 # no tiles: nothing to do, no launch
    torch.cuda.synchronize()
    assert bool((buf == GUARD).all())                                                  # nothing was written by any of them
    with pytest.raises(RuntimeError, match="mvg_refresh_operands"):
        ops.refresh_operands(rec.to(torch.int32), til)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.refresh_operands(rec.cpu(), til.cpu())
    # table entries that point outside the tables are skipped, not followed
    til2 = torch.tensor([(5, 0), (0, 99), (-1, 0), (0, 0)], dtype=torch.int32).to(DEV)
    ops.refresh_operands(rec, til2)
    torch.cuda.synchronize()
    _check(src, dst, None)
    assert _guards_intact(buf, 64 * 64)
