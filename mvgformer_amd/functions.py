"""autograd wrapper of the sampling op -- mirror of
lib/models/ops/functions/deform_func.py:34-65 (DeformFunction)."""
import os

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import deformable as DF
from . import ops


class DeformFunction(Function):
    @staticmethod
    def forward(ctx, value, value_spatial_shapes, value_level_start_index, sampling_locations, attention_weights,
                im2col_step):
        ctx.im2col_step = im2col_step
        output = DF.deform_forward(value, value_spatial_shapes, value_level_start_index, sampling_locations,
                                   attention_weights, ctx.im2col_step)
        ctx.save_for_backward(value, value_spatial_shapes, value_level_start_index, sampling_locations,
                              attention_weights)
        # host copies of the level tables for the deterministic backward (its binning workspace is sized on the host): looked
        # up here, where the tensors are the caller's own objects and usually carry the copy already -- not a sync per
        # backward.  Only when a gradient will be asked for: under no_grad (and inside a HIP-graph capture, where the D2H
        # copy of a first look-up is illegal) the forward touches nothing on the host.
        needs = value.is_cuda and any(ctx.needs_input_grad)
        ctx.host_levels = ops.host_levels(value_spatial_shapes, value_level_start_index) if needs else None
        return output

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        value, shapes, starts, loc, attn = ctx.saved_tensors
        DF._check_step(value, ctx.im2col_step)
        if value.dtype == torch.bfloat16:
            # bf16 training: the op's output is bf16 (so is the gradient autograd hands back); the backward takes fp32 and
            # returns an fp32 grad_value (autograd rounds it to the bf16 value's dtype)
            grad_output = grad_output.float()
        with DF._device_of(value):
            gv, gl, ga = ops.msda_backward(value, shapes, starts, loc, attn, grad_output.contiguous(), host=ctx.host_levels)
        return gv, None, None, gl, ga, None


# training-path GEMMs: "f32s" = this repo's mvg_linear (fp32 storage, fp32-accurate products on the bf16 matrix pipe from 3-way split
# operands -- csrc/gemm.hip) for forward, dgrad and wgrad; "torch" = nn.functional.linear (rocBLAS fp32: the f32-input MFMA runs at
# 1/16 of the bf16 rate and was 40 % of a training step's kernel time, profiles/r02_train_step.txt)
TRAIN_GEMM = os.environ.get("MVG_TRAIN_GEMM", "f32s")


class LinearF32S(Function):
    """y = act(x W^T + b) with all three GEMMs of its autograd on mvg_linear's split form:
         forward  y  = x W^T              (rows, K) x (N, K)^T, bias + ReLU in the epilogue
         dgrad    dx = dy W               = mvg_linear(dy, W^T as an (K, N) "weight")
         wgrad    dW = dy^T x, db = sum dy = mvg_linear_wgrad_bias_f32 (the reduction runs over the rows: split into slices, the
                                            slices' partials and the bias gradient summed inside the same launch)
       (the Linear + ReLU + Linear chains of lib/models/dq_decoder.py:659-717,763-778, mvp_decoder.py:94-98 and
       lib/models/ops/modules/projattn.py:169,180-181,203 under torch autograd).  Output widths that are not a multiple of 32 (the
       2- and 3-output heads) run with zero rows up to 32 outputs; the padding stays inside this Function."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu):
        x2 = x.reshape(-1, x.shape[-1])
        if x2.stride(1) != 1:
            x2 = x2.contiguous()
        N, K = weight.shape
        Np = (N + 31) // 32 * 32
        if Np != N:
            wp = weight.new_zeros((Np, K))
            wp[:N] = weight
            bp = None
            if bias is not None:
                bp = bias.new_zeros((Np,))
                bp[:N] = bias
        else:
            wp, bp = weight.contiguous(), bias
        y = ops.linear(x2, wp, bp, out_dtype=torch.float32, relu=bool(relu))
        if Np != N:
            y = y[:, :N].contiguous()
        ctx.relu = bool(relu)
        ctx.x_shape = x.shape
        ctx.save_for_backward(x2, wp, y if relu else None)
        ctx.has_bias = bias is not None
        ctx.n_out = N
        return y.view(*x.shape[:-1], N)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        x2, wp, y = ctx.saved_tensors
        Np, K = wp.shape
        N = ctx.n_out
        dy = grad_y.reshape(-1, N)
        if ctx.relu:
            dy = torch.ops.aten.threshold_backward(dy, y, 0.0)               # dy where y > 0, one launch
        if Np != N:
            dyp = dy.new_zeros((dy.shape[0], Np))
            dyp[:, :N] = dy
            dy = dyp
        elif not dy.is_contiguous():
            dy = dy.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = ops.linear(dy, wp.t().contiguous(), None, out_dtype=torch.float32).view(ctx.x_shape)
        want_b = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1]:
            dw, db = ops.linear_wgrad_bias(dy, x2, want_bias=want_b)     # no dy^T / x^T copies: transposed on the way into LDS
            if Np != N:
                dw = dw[:N]
                db = None if db is None else db[:N]
        elif want_b:
            db = dy.sum(0)[:N]
        return dx, dw, db, None


class LinearBF16(Function):
    """bf16 mixed-precision sibling of LinearF32S: y = act(x W^T + b) with bf16 operands, fp32 accumulation and fp32 master weights.
         forward  y  = mvg_linear(x, W16): an fp32 x is rounded to bf16 as it is loaded, bias + ReLU in the fp32 epilogue, y fp32 (or
                       bf16 when out_bf16: the value projection, whose consumer -- the sampling op -- reads bf16)
         dgrad    dx = mvg_linear(bf16(dy), W16^T)                            fp32 dx
         wgrad    dW, db = mvg_linear_wgrad_bias_bf16(bf16(dy), bf16(x))      fp32, slice-ordered (deterministic)
       w16 / w16t: the bf16 weight and its transpose, cast once per optimizer step by the caller (bf16_weights); the gradient goes to
       the fp32 `weight`.  Saves bf16(x) and, for the ReLU mask, the output.  Needs N % 64 == 0 (dgrad's K) and K % 64 == 0: the
       2- and 3-output heads stay on LinearF32S."""

    @staticmethod
    def forward(ctx, x, weight, bias, w16, w16t, relu, out_bf16):
        x2 = x.reshape(-1, x.shape[-1])
        if x2.stride(1) != 1 or x2.stride(0) != x2.shape[1]:
            x2 = x2.contiguous()
        N = w16.shape[0]
        y = ops.linear(x2, w16, bias, out_dtype=torch.bfloat16 if out_bf16 else torch.float32, relu=bool(relu))
        x16 = x2 if x2.dtype == torch.bfloat16 else x2.to(torch.bfloat16)
        ctx.relu = bool(relu)
        ctx.x_shape = x.shape
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x16, w16t, y if relu else None)
        return y.view(*x.shape[:-1], N)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        x16, w16t, y = ctx.saved_tensors
        N = w16t.shape[1]
        dy = grad_y.reshape(-1, N)
        if ctx.relu:
            dy = torch.ops.aten.threshold_backward(dy, y.to(dy.dtype) if y.dtype != dy.dtype else y, 0.0)
        dy16 = dy.to(torch.bfloat16).contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = ops.linear(dy16, w16t, None, out_dtype=torch.float32).view(ctx.x_shape)
        want_b = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1]:
            dw, db = ops.linear_wgrad_bias(dy16, x16, want_bias=want_b)
        elif want_b:
            db = dy16.float().sum(0)
        return dx, dw, db, None, None, None, None


def bf16_weights(cache, key, params, build=None):
    """(W16, W16^T) of a Linear weight for LinearBF16, cast once per optimizer step: cached on the source parameters' versions in
    `cache` (a projattn.WeightCache).  build(*params) forms the fp32 weight when it is not params[0] (ProjAttn's concatenated
    [sampling_offsets; attention_weights])."""
    w16 = cache.get(key, params, torch.bfloat16, build, sync=False)
    w16t = cache.get(key + "^T", params, torch.bfloat16, lambda *p: (build(*p) if build else p[0]).t(), sync=False)
    return w16, w16t


def linear_bf16(x, weight, bias, cache, key, params=None, build=None, relu=False, out_bf16=False):
    """the bf16 training path's Linear: LinearBF16 where its shape rules hold (both widths multiples of 64), LinearF32S otherwise
    (the 2- and 3-output heads: fp32 operands).  `weight` is the differentiable fp32 weight; its bf16 copies come from `cache`
    under `key`, stamped with `params` (default: (weight,))."""
    N, K = weight.shape
    if x.is_cuda and N % 64 == 0 and K % 64 == 0 and x.numel() > 0:
        w16, w16t = bf16_weights(cache, key, params or (weight,), build)
        return LinearBF16.apply(x, weight, bias, w16, w16t, relu, out_bf16)
    y = linear(x.float(), weight, bias, relu)
    return y.to(torch.bfloat16) if out_bf16 else y


def linear(x, weight, bias=None, relu=False):
    """nn.functional.linear (+ ReLU) for the training path: LinearF32S where mvg_linear's shape rules hold (fp32 on the GPU,
    in_features % 32 == 0 -- every Linear of the decoder), torch elsewhere."""
    N, K = weight.shape
    if TRAIN_GEMM == "f32s" and x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and K % 32 == 0 and x.numel() > 0:
        return LinearF32S.apply(x, weight, bias, relu)
    y = torch.nn.functional.linear(x, weight, bias)
    return torch.relu(y) if relu else y


class SelfAttentionFunction(Function):
    """softmax(q k^T / sqrt(32)) v per (batch element, head) with both directions on csrc/mha.hip: mvg_self_attention_train keeps
    the row statistic lse, mvg_self_attention_backward recomputes P from it (no Lq x Lq tensor is saved) and writes dq, dk, dv
    deterministically, in the inputs' dtype.  p_drop > 0: attention dropout inside the kernels from `seed` (1-element int64
    device tensor, saved for the backward: both directions see one mask)."""

    @staticmethod
    def forward(ctx, q, k, v, p_drop, seed):
        out, lse = ops.self_attention_train(q, k, v, p_drop, seed)
        ctx.p_drop = p_drop
        ctx.save_for_backward(q, k, v, out, lse, seed if p_drop > 0 else None)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        q, k, v, out, lse, seed = ctx.saved_tensors
        dq, dk, dv = ops.self_attention_backward(q, k, v, out, grad_out.contiguous(), lse, ctx.p_drop, seed)
        return dq, dk, dv, None, None


def attention_seed(device):
    """a fresh dropout seed for self_attention: 1-element int64 tensor drawn on the device by torch's generator on the current
    stream -- torch.manual_seed repeats it, a captured graph draws a new one per replay, and the host never reads it"""
    return torch.empty((1,), dtype=torch.int64, device=device).random_()


def self_attention(q, k, v, dropout_p=0.0, training=False, seed=None):
    """differentiable ops.self_attention (SelfAttentionFunction): q, k, v (B, Lq, 256) float32 or bfloat16, column blocks of wider
    tensors allowed.  Attention dropout with dropout_p while `training`, as nn.MultiheadAttention applies it; seed: the tensor to
    take the mask from (default: attention_seed, a fresh one per call)."""
    p = float(dropout_p) if training else 0.0
    if p > 0.0 and seed is None:
        seed = attention_seed(q.device)
    return SelfAttentionFunction.apply(q, k, v, p, seed)


class RefGatherAdd(Function):
    """xin[n, q, l] = bilinear(feat[n], level l, reference point (n, q, l)) + query[n, q]  (projattn.py:134-141,180: grid_sample at the
    clamped reference points, zeros padding, align_corners=False) through mvg_gather_ref; differentiable in `query` only."""

    @staticmethod
    def forward(ctx, query, feat, ref_lvl, levels):
        n, Lq, C = query.shape
        ain = ops.gather_ref(feat, ref_lvl, query.detach(), levels, 1, n)
        ctx.shape = (n, Lq, levels.L, C)
        return ain.view(n, Lq, levels.L, C)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return g.reshape(ctx.shape).sum(2), None, None, None


class CriterionFunction(Function):
    """(L, 8) loss table of ops.criterion (columns ops.CRITERION_COLUMNS) for all decoder layers of one step.  The kernels
    produce the gradients of loss_ce, loss_pose_perjoint and loss_pose_perprojection_2d in the forward pass; backward scales them
    per layer by the table's grad_output (the 2D term also by keep_2d: a guarded layer gives a zero gradient).  The metric columns
    carry no gradient.  joint_map (not differentiable): ops.criterion's; the pose gradients keep the predictions' joint count."""

    @staticmethod
    def forward(ctx, logits, poses, poses_2d, pair_query, pair_gt, pair_count, joints_3d, joints_3d_vis, joints_vis, num_person,
                cams, space_size, space_center, pred_conf_threshold, num_samples, focal_alpha, focal_gamma, joint_map=None):
        table, gl, gp, gp2 = ops.criterion(logits, poses, poses_2d, pair_query, pair_gt, pair_count, joints_3d, joints_3d_vis,
                                           joints_vis, num_person, cams, space_size, space_center, pred_conf_threshold,
                                           num_samples, focal_alpha, focal_gamma, joint_map=joint_map)
        ctx.save_for_backward(gl, gp, gp2, table)
        return table

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_table):
        gl, gp, gp2, table = ctx.saved_tensors
        g = grad_table.to(torch.float32)
        keep = table[:, 7] > 0
        zero = torch.zeros_like(gp2)
        g_logits = gl * g[:, 0].view(-1, 1, 1, 1)
        g_poses = gp * g[:, 5].view(-1, 1, 1, 1)
        g_2d = torch.where(keep.view(-1, 1, 1, 1, 1), gp2 * g[:, 6].view(-1, 1, 1, 1, 1), zero)
        return (g_logits, g_poses, g_2d) + (None,) * 15
