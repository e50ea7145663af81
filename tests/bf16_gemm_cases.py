"""Case lists, inputs and a CPU emulation (with eight defects) for the tests of the bf16 GEMMs: mvg_pyramid_group_ws
(csrc/wreg_gemm.hip) and the bf16 paths of mvg_linear / mvg_linear_sum (csrc/gemm.hip).  Not a test module:
tests/test_bf16_gemm_ref_cpu.py checks the lists' coverage, the straddler cap and that the reference of tests/bf16_gemm_ref.py
rejects every defect; tests/test_bf16_gemm_fp64.py runs the same cases on the device.  Everything is made on the CPU from seeded
generators, so both files see the same numbers."""
import random

import torch

from tests import bf16_gemm_ref as B

BF = torch.bfloat16


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------ pyramid products
# (n_img, S, jobs, slots): M = n_img * S rows; jobs alternate value (bias, head planes) and G (N = 192, no bias, row-major).
# The (M, jobs, slots) come from B.group_tile_counts (tile counts per workgroup in the comments; test_bf16_gemm_ref_cpu asserts
# them); S in {1, 5, 31} runs the SMALL_S addressing (a tile crosses several images), 32 / 33 / 31 put an image boundary on the
# first row, the second row and the last row of a tile; M = 31, 257, 1237 are prime.
PYR_CASES = [
    (1, 1, 1, 0),          # M = 1: 0 and 1 tiles
    (1, 31, 2, 0),         # 31: 0, 1
    (1, 32, 2, 0),         # 32: 0, 1
    (1, 33, 2, 0),         # 33: 0, 1
    (33, 1, 2, 0),
    (51, 5, 2, 0),         # 255: 1
    (1, 257, 8, 0),        # 257: 0, 1
    (257, 1, 8, 0),
    (9, 31, 2, 0),         # 279: image boundaries on the last row of a tile, then walking backwards
    (9, 32, 2, 0),         # 288: on every tile's first row
    (9, 33, 2, 0),         # 297: on the second row, then walking forwards
    (289, 1, 2, 1),        # 289: 1, 2
    (17, 17, 2, 1),
    (109, 5, 2, 1),        # 545: 2, 3
    (3, 277, 2, 1),        # 831: 3, 4
    (831, 1, 1, 1),        # 831, one job: 3, 4
    (7, 151, 8, 8),        # 1057: 4, 5
    (23, 57, 6, 3),        # 1311: 5, 6
    (1, 1237, 2, 0),       # 1237 (prime, one image)
    (2, 1237, 8, 0),       # 2474: 1, 2 (S = M / 2)
    (3, 1237, 2, 32),      # 3711: 0, 1
]
# the table of the cases' (M, jobs, slots) -> tile counts per workgroup, as B.group_tile_counts gives them
PYR_TABLE = {(1, 1, 0): {0, 1}, (31, 2, 0): {0, 1}, (32, 2, 0): {0, 1}, (33, 2, 0): {0, 1}, (255, 2, 0): {1}, (257, 8, 0): {0, 1},
             (289, 2, 1): {1, 2}, (545, 2, 1): {2, 3}, (831, 2, 1): {3, 4}, (831, 1, 1): {3, 4}, (1057, 8, 8): {4, 5},
             (1311, 6, 3): {5, 6}, (2474, 8, 0): {1, 2}, (3711, 2, 32): {0, 1}}


def pyr_id(c):
    return "img%d_S%d_jobs%d_slots%d" % c


def job_is_planes(j):
    return j % 2 == 0


_PYR_W = {}


def pyr_job(j):
    """job j's plain operands: (W bf16 (256 | 192, 256), bias fp32 (256) | None, planes)."""
    if j not in _PYR_W:
        gen = _gen(40 + j)
        if job_is_planes(j):
            _PYR_W[j] = ((torch.randn(256, 256, generator=gen) / 16).to(BF), torch.randn(256, generator=gen), True)
        else:
            _PYR_W[j] = ((torch.randn(192, 256, generator=gen) / 16).to(BF), None, False)
    return _PYR_W[j]


def pyr_feat(M, seed):
    """(M, 256) bf16: randn rows times a per-row log-normal scale."""
    gen = _gen(seed)
    return (torch.randn(M, 256, generator=gen) * torch.exp(torch.randn(M, 1, generator=gen))).to(BF)


def pyr_case_feat(c):
    n_img, S, jobs, slots = c
    return pyr_feat(n_img * S, 1000 * jobs + 7 * n_img + S + slots)


def pyr_edge_rows(kind, M=289, seed=3):
    """operand rows at the edges (bf16, all within the normal range of bf16 and fp32, partial sums included)."""
    gen = _gen(seed)
    x = torch.randn(M, 256, generator=gen)
    if kind == "rows_24_decades":                    # 1e-12 .. 1e12 row by row
        x = x * 10.0 ** torch.linspace(-12, 12, M)[:, None]
    elif kind == "zero_rows":
        x[::3] = 0
    elif kind != "randn":
        raise KeyError(kind)
    return x.to(BF)


def tie_case(M=289, seed=9):
    """(feat, Wv, bv, Wg): small-integer operands, so every partial sum is an integer or a half-integer far below 2^24 and the
    fp32 accumulation is EXACT; the value bias 160.5 and the G column pair (160, 1) x (1, 0.5) put the results at k + 1/2 around 160,
    where bf16 steps by 1: exact ties, half of which round down under round-to-nearest-even."""
    gen = _gen(seed)
    feat = torch.randint(-2, 3, (M, 256), generator=gen).float()
    feat[:, 0], feat[:, 1] = 1.0, 0.5
    Wv = torch.randint(-1, 2, (256, 256), generator=gen).float()
    Wv[:, :2] = 0
    Wg = torch.randint(-1, 2, (192, 256), generator=gen).float()
    Wg[:, 0], Wg[:, 1] = 160.0, 1.0
    return feat.to(BF), Wv.to(BF), torch.full((256,), 160.5), Wg.to(BF)


# ------------------------------------------------------------------------------------------------------------------ bf16 linear
LIN_M = (1, 63, 64, 65, 127, 128, 129, 193, 257)
LIN_N = (8, 120, 128, 136, 192, 256, 576)
LIN_K = (64, 128, 256, 1024)
LIN_OPTIONS = ("relu", "mask", "bias", "strided", "a2")
DTYPES = (("bf16", "f32"), ("bf16", "bf16"), ("f32", "f32"), ("f32", "bf16"))        # (A, out); W is bf16


def _lin_cases():
    """the M x N grid thinned to 56 shapes; K, the linear_tiles knob (0: 128 x 128 also for M > 64, 2: 64 x 128 also for
    M <= 64) and the options cycle / are drawn from a seeded generator.  a2 (A + A2 on load) applies to fp32 A only."""
    rnd = random.Random(5)
    out = []
    for i, M in enumerate(LIN_M):
        for j, N in enumerate(LIN_N):
            if (i + 2 * j) % 9 == 4:
                continue
            k = len(out)
            out.append(dict(M=M, N=N, K=LIN_K[(i + j) % 4], tiles=(1, 0, 2)[k % 3], relu=rnd.random() < 0.5, mask=rnd.random() < 0.5,
                            bias=rnd.random() < 0.7, strided=rnd.random() < 0.4, a2=rnd.random() < 0.4))
            # The straddler share is about 2 d / step averaged over the results, and d grows like sqrt(K + 1): at K = 1024 a sum of
            # random signs has 2.2 - 2.8 % straddlers (the results near zero carry them), above the 2 % cap.  Behind a ReLU half of
            # them are exact zeros, so the K = 1024 shapes all run with ReLU (the k loop does not know about the epilogue).
            if out[-1]["K"] == 1024:
                out[-1]["relu"] = True
    return out


LIN_CASES = _lin_cases()


def lin_id(c):
    return "M%d_N%d_K%d_t%d" % (c["M"], c["N"], c["K"], c["tiles"]) + "".join("_" + o for o in LIN_OPTIONS if c[o])


def lin_inputs(c, seed=0):
    """dict(a, a2 fp32 (M, K), w bf16 (N, K), b fp32 (N) | None, mask uint8 (M) | None): randn rows times a per-row log-normal
    scale, weights randn / sqrt(K), a bias of both signs, about 30 % masked rows."""
    M, N, K = c["M"], c["N"], c["K"]
    gen = _gen(seed + 31 * M + 7 * N + K)
    scale = torch.exp(torch.randn(M, 1, generator=gen))
    a = torch.randn(M, K, generator=gen) * scale
    a2 = torch.randn(M, K, generator=gen) * scale
    w = (torch.randn(N, K, generator=gen) / K ** 0.5).to(BF)
    b = torch.randn(N, generator=gen)
    mask = (torch.rand(M, generator=gen) > 0.3).to(torch.uint8)
    mask[0] = 1                                          # (M = 1: the one row is kept)
    return dict(a=a, a2=a2 if c["a2"] else None, w=w, b=b if c["bias"] else None, mask=mask if c["mask"] else None)


def lin_operand(inp, a_dtype):
    """the bf16 operand of the case: bf16 A is bf16(a) handed over as it is (no A2); fp32 A is rounded on load after + A2."""
    return B.operand(inp["a"]) if a_dtype == "bf16" else B.operand(inp["a"], inp["a2"])


# ------------------------------------------------------------------------------------------- CPU emulation and the eight defects
ELEMENT_DEFECTS = ("truncate", "bias_after_round", "bias_group_shift", "relu_before_bias", "mask_before_bias")
ROW_DEFECTS = ("heads_swapped", "ragged_shift", "stale_tile")


def _truncate(v):
    return (v.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF)


def shift_bias_groups(b):
    """every 32-column block's eight 4-column groups moved on by one (columns past the end count as zeros)."""
    n = b.numel()
    p = torch.zeros((n + 31) // 32 * 32, dtype=b.dtype)
    p[:n] = b
    return p.view(-1, 8, 4).roll(1, dims=1).reshape(-1)[:n].clone()


def emulate(x, W, b=None, out_bf16=True, relu=False, mask=None, defect=None):
    """the kernels' arithmetic in torch: fp32 accumulation of the exact bf16 products, then the epilogue
    x = acc + bias; relu; keep ? x : 0; round to bf16 (nearest even) -- or one of ELEMENT_DEFECTS:
      truncate           the bf16 result cut off instead of rounded
      bias_after_round   bf(bf(acc) + bias)
      bias_group_shift   shift_bias_groups(bias)
      relu_before_bias   relu(acc) + bias
      mask_before_bias   the mask applied to the accumulator, in front of bias and ReLU: a masked row comes out as act(bias).  (The
                         mask directly in front of the ReLU, behind the bias, is no defect: relu(0) = 0.  With ReLU and an
                         all-negative bias this one hides too -- relu(bias) = 0 -- so the cases carry biases of both signs, and
                         the check runs it with a negative bias without ReLU as well.)"""
    acc = x.float() @ W.float().t()
    bias = torch.zeros(W.shape[0]) if b is None else b.float()
    keep = None if mask is None else (mask.view(-1, 1) != 0)
    zero = torch.zeros(())
    if defect == "bias_group_shift":
        bias = shift_bias_groups(bias)
    if defect == "mask_before_bias" and keep is not None:
        acc = torch.where(keep, acc, zero)
    if defect == "bias_after_round":
        v = acc.to(BF).float() + bias
    elif defect == "relu_before_bias" and relu:
        v = torch.relu(acc) + bias
    else:
        v = acc + bias
    if relu and defect != "relu_before_bias":
        v = torch.relu(v)
    if keep is not None and defect != "mask_before_bias":
        v = torch.where(keep, v, zero)
    if not out_bf16:
        return v
    return _truncate(v) if defect == "truncate" else v.to(BF)


def defect_rows(out, kind, n_img, S):
    """a clean (M, 256 | 192) result with one of ROW_DEFECTS, or None where the shape has no room for it:
      heads_swapped  the planes of heads 2 and 5 exchanged (value product)
      ragged_shift   the rows of the last, ragged tile moved down by one (each takes the row in front of it)
      stale_tile     the rows of one 32-row tile taken from the tile in front of it (a ring slot that was not refilled)"""
    M = out.shape[0]
    ntiles = (M + B.RM - 1) // B.RM
    out = out.clone()
    if kind == "heads_swapped":
        vh = B.to_planes(out, n_img, S)
        vh[:, [2, 5]] = vh[:, [5, 2]]
        return B.from_planes(vh)
    if kind == "ragged_shift":
        r0 = (ntiles - 1) * B.RM
        if M % B.RM == 0 or M < 2:
            return None
        lo = max(r0, 1)
        out[lo:M] = out[lo - 1:M - 1].clone()
        return out
    if kind == "stale_tile":
        if ntiles < 2:
            return None
        t = max(ntiles // 2, 1)
        n = min(B.RM, M - t * B.RM)
        out[t * B.RM:t * B.RM + n] = out[(t - 1) * B.RM:(t - 1) * B.RM + n].clone()
        return out
    raise KeyError(kind)
