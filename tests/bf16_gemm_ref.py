"""fp64 statement and bound of the two bf16 GEMMs: mvg_pyramid_group_ws (csrc/wreg_gemm.hip: value head planes and G) and the
bf16 paths of mvg_linear / mvg_linear_sum (csrc/gemm.hip).  Not a test module: tests/test_bf16_gemm_ref_cpu.py checks it against
a CPU emulation of the kernels and of eight defects, tests/test_bf16_gemm_fp64.py holds the kernels to it.

The operands are exactly bf16, so the truth is y = lin(x, W, b) in fp64 ON the bf16 values, and the kernel's unrounded fp32 value
(fp32 accumulation of exact products over K + 1 terms) lies within d = LAMBDA lin_err(x, None, W, b) of it (tests/chain_ref.py).
  fp32 output   |got - y| <= d.
  bf16 output   the expected value is bf(y), the allowed deviation round_err(y, d, rms=False): ZERO -- bit-equal to bf(y) --
                except where [y - d, y + d] straddles a bf16 rounding boundary ("straddlers", a share of about 2 d / step); there
                one bf16 step.
Epilogue of csrc/gemm.hip, applied to y before the rounding:  x = acc + bias; relu; keep ? x : 0; round.  ReLU does not enlarge an
error, and an element whose whole interval is <= 0 is exactly 0 behind it; a masked row is exactly 0 with bound 0.
fp32 A converted on load: x = bf(a); A + A2: x = bf(a + a2), the sum in fp32 (operand() below)."""
import torch

from tests.chain_ref import LAMBDA, bf, lin, lin_err, round_err

RM = 32                                    # rows per tile of the pyramid products


def operand(a, a2=None):
    """the bf16 operand the kernel forms from A (bf16: as it is; fp32: rounded on load, after the fp32 sum with A2)."""
    if a2 is not None:
        a = a.float() + a2.float()
    return a.to(torch.bfloat16)


def expected(x, W, b=None, out_bf16=True, relu=False, mask=None):
    """(expected value, allowed deviation) of act(x W^T + b) (* mask) per element, fp64.  x, W: bf16 values (any dtype that holds
    them exactly); b fp32 or None; mask: (M) uint8 / bool or None."""
    y = lin(x, W, b)
    d = LAMBDA * lin_err(x, None, W, b)
    zero = torch.zeros((), dtype=torch.float64, device=y.device)
    if relu:
        d = torch.where(y + d <= 0, zero, d)         # the kernel's value is <= 0 as well: exactly 0 behind the ReLU
        y = torch.relu(y)
    if mask is not None:
        keep = mask.view(-1, 1) != 0
        y, d = torch.where(keep, y, zero), torch.where(keep, d, zero)
    if out_bf16:
        return bf(y), round_err(y, d, rms=False)
    return y, d


def to_planes(y, n_img, S):
    """rows (n_img * S, 256) -> the head-plane layout vh[img][head 8][s][32] of the value product."""
    return y.view(n_img, S, 8, 32).permute(0, 2, 1, 3).contiguous()


def from_planes(vh):
    n_img, _, S, _ = vh.shape
    return vh.permute(0, 2, 1, 3).reshape(n_img * S, 256)


def group_split(M, njobs, slots=0, wreg_grid=512):
    """(ntiles, slots per XCD of every job), None for a launch the entry refuses.  Restates mvg_pyramid_group_ws in
    csrc/wreg_gemm.hip (every job's weight is 1):
        const int ntiles = (gp.M + RM - 1) / RM;
        int budget = slots_per_xcd > 0 ? slots_per_xcd : g_wreg_grid / 8;
        if (budget > WREG_MAX_SLOTS) budget = WREG_MAX_SLOTS;
        if (budget > (ntiles + 7) / 8 * njobs) budget = (ntiles + 7) / 8 * njobs;
        if (budget < njobs) budget = njobs;
        ... int c = budget * weight[j] / total;  if (c < 1) c = 1;  gp.job_slots[j] = c;  n_slots += c;
        if (n_slots > WREG_MAX_SLOTS) return MVG_E_BADARG;"""
    ntiles = (M + RM - 1) // RM
    budget = slots if slots > 0 else wreg_grid // 8
    budget = min(budget, 64)
    budget = min(budget, (ntiles + 7) // 8 * njobs)
    budget = max(budget, njobs)
    job_slots = [max(budget * 1 // njobs, 1) for _ in range(njobs)]
    if sum(job_slots) > 64:
        return None
    return ntiles, job_slots


def group_tile_counts(M, njobs, slots=0, wreg_grid=512):
    """per job, the set of tile counts of its workgroups.  Restates wreg2_group_kernel / wreg2_body:
        const int first = gp.slot_idx[slot] * 8 + xcd, stride = gp.job_slots[j] * 8;
        int tile = first_tile;  if (tile < ntiles) {...; tile += G;}  for (; tile < ntiles; tile += G) ..."""
    ntiles, job_slots = group_split(M, njobs, slots, wreg_grid)
    out = []
    for js in job_slots:
        counts = set()
        for slot_idx in range(js):
            for xcd in range(8):
                first, stride = slot_idx * 8 + xcd, js * 8
                counts.add(0 if first >= ntiles else -(-(ntiles - first) // stride))
        out.append(counts)
    return out


def linear_tile(M, N, linear_tiles=1):
    """(BM, BN) of a launch.  Restates launch_linear in csrc/gemm.hip:
        if (g_linear_tiles) {
          if (N % 192 == 0 && N % 128 != 0) return launch_linear_tile<..., 128, 192>(...);
          const long tiles128 = (long)((N + 127) / 128) * ((M + 127) / 128);
          if ((tiles128 < 384 && M > 64) || g_linear_tiles == 2) return launch_linear_tile<..., 64, 128>(...);
        }
        return launch_linear_tile<..., 128, 128>(...);"""
    if linear_tiles:
        if N % 192 == 0 and N % 128 != 0:
            return 128, 192
        tiles128 = ((N + 127) // 128) * ((M + 127) // 128)
        if (tiles128 < 384 and M > 64) or linear_tiles == 2:
            return 64, 128
    return 128, 128
