"""Stage-level wrappers over the C ABI: torch tensors in, torch tensors out.

Each function validates what the C side cannot (device, dtype, contiguity), allocates the
output with torch and enqueues the HIP kernel on torch's current stream.  No host sync.
"""
from __future__ import annotations

import ctypes as C

import math

import numpy as np
import torch

from . import _lib as L

_D = L.DEFINES      # the numeric #defines of include/mvg_decoder.h: every limit and code below takes its value from there

# backward of the sampling op: "det" = deterministic tile-binned form where the shape allows (D = 32), "atomic" = always the
# fp32-atomics form of round 1 (the reference's own scheme), "balanced" = the deterministic form with its reduce step launched over
# (bin, chunk) work items (mvg_msda_backward_bal_*: det's bits, a time that does not depend on where the samples fall)
BACKWARD_MODE = __import__("os").environ.get("MVG_BACKWARD", "det")
# entries per work item of the balanced mode: None = the library default, otherwise a positive multiple of 256.  Read at every
# call and passed as an argument: a captured graph keeps the value it was captured with.
BACKWARD_CHUNK = None


def _det_entry(lib, bf16, dims, shapes_c):
    """(symbol, workspace bytes, trailing arguments) of the deterministic backward that BACKWARD_MODE selects; workspace bytes 0:
    the shape is not supported, the caller falls back to the atomic kernel."""
    kind = "bf16" if bf16 else "f32"
    if BACKWARD_MODE == "balanced":
        chunk = 0 if BACKWARD_CHUNK is None else int(BACKWARD_CHUNK)
        if chunk < 0 or chunk % 256:
            raise L.MvgError("BACKWARD_CHUNK must be None, 0 or a positive multiple of 256 (got %r)" % (BACKWARD_CHUNK,))
        # the chunk follows the stream in this prototype, so the stream is passed here
        return ("mvg_msda_backward_bal_" + kind, int(lib.mvg_msda_backward_bal_workspace(*dims, shapes_c, chunk)),
                (L.stream_ptr(), chunk))
    return "mvg_msda_backward_det_" + kind, int(lib.mvg_msda_backward_det_workspace(*dims, shapes_c)), ()


# ---- optional per-launch timing with HIP events on the launch stream (bench.py roofline) -----
PROFILE = None   # None (off) or dict name -> list[(start_event, end_event)]


class _timed:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        if PROFILE is not None:
            self.s = torch.cuda.Event(enable_timing=True)
            self.e = torch.cuda.Event(enable_timing=True)
            self.s.record()      # recorded on torch's current stream == the stream the kernel is launched on

    def __exit__(self, *a):
        if PROFILE is not None:
            self.e.record()
            PROFILE.setdefault(self.name, []).append((self.s, self.e))
        return False


def _launch(symbol, *args, label=None):
    """The one way this module enqueues an entry point of the library: tensors (and None) are passed as they are (L.TensorPtr),
    the current stream is appended where the prototype ends in it, the launch is timed under ``label`` (the key of bench.py's
    per-kernel records; None: not timed) and a non-zero return code raises."""
    fn = getattr(L.load(), symbol)
    if symbol in L.STREAM_LAST:
        args += (L.stream_ptr(),)
    if label is None:
        rc = fn(*args)
    else:
        with _timed(label):
            rc = fn(*args)
    L.check(rc, symbol)


def profile_summary():
    """name -> (launches, mean ms) after a torch.cuda.synchronize()."""
    out = {}
    for k, evs in (PROFILE or {}).items():
        ms = [a.elapsed_time(b) for a, b in evs]
        out[k] = (len(ms), sum(ms) / max(len(ms), 1))
    return out


def _i64_host(t):
    """small int64 table (shapes / starts) as a host ctypes array (no device sync if it is
    already a CPU tensor / list)."""
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().tolist()
    flat = np.asarray(t, dtype=np.int64).reshape(-1)
    return (C.c_int64 * len(flat))(*flat.tolist()), flat


def host_levels(spatial_shapes, level_start_index):
    """(shapes_c, starts_c) host ctypes copies of the two level tables.  A device tensor costs one D2H sync the first time it is
    seen; the copy is then kept ON THE TENSOR OBJECT (valid while its version counter is unchanged), so a training loop that
    reuses its level tensors -- and the backward of a forward that already looked them up -- never syncs again."""
    out = []
    for t in (spatial_shapes, level_start_index):
        cached = getattr(t, "_mvg_host", None) if isinstance(t, torch.Tensor) else None
        # keyed on (storage address, version): in-place writes bump the version, .data / set_() re-pointing changes the address
        if cached is not None and cached[0] == (t.data_ptr(), t._version):
            out.append(cached[1])
            continue
        arr, _ = _i64_host(t)
        if isinstance(t, torch.Tensor):
            try:
                t._mvg_host = ((t.data_ptr(), t._version), arr)
            except Exception:      # pragma: no cover - tensor subclasses without a __dict__
                pass
        out.append(arr)
    return tuple(out)


class Levels:
    """Host copy of (spatial_shapes, level_start_index): avoids a D2H sync per call."""

    def __init__(self, spatial_shapes, level_start_index):
        self.shapes_c, shapes = _i64_host(spatial_shapes)
        self.starts_c, starts = _i64_host(level_start_index)
        self.shapes = shapes.reshape(-1, 2)
        self.starts = starts
        self.L = len(starts)
        self.S = int((self.shapes[:, 0] * self.shapes[:, 1]).sum())


# --------------------------------------------------------------------------- Deformable op
def msda_forward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight):
    """Deformable.deform_forward (lib/models/ops/src/deform.h:32-50)."""
    L.require_cuda(value, spatial_shapes, level_start_index, sampling_loc, attn_weight)
    for name, t in (("value", value), ("spatial_shapes", spatial_shapes), ("level_start_index", level_start_index),
                    ("sampling_loc", sampling_loc), ("attn_weight", attn_weight)):
        if not t.is_contiguous():
            raise RuntimeError("%s tensor has to be contiguous" % name)      # deform_cuda.cu:39-43
    if spatial_shapes.dtype != torch.int64 or level_start_index.dtype != torch.int64:
        raise RuntimeError("spatial_shapes / level_start_index must be int64")
    N, S, M, D = value.shape
    _, Lq, _, nl, P, _ = sampling_loc.shape
    L.load()
    out = torch.empty((N, Lq, M * D), dtype=value.dtype, device=value.device)
    if Lq == 0:
        return out
    if value.dtype == torch.float32:
        if sampling_loc.dtype != torch.float32 or attn_weight.dtype != torch.float32:
            raise RuntimeError("sampling_loc / attn_weight must be float32")
        symbol = "mvg_msda_forward_f32"
    elif value.dtype == torch.float64:      # AT_DISPATCH_FLOATING_TYPES' double case (deform_cuda.cu:75)
        if sampling_loc.dtype != torch.float64 or attn_weight.dtype != torch.float64:
            raise RuntimeError("sampling_loc / attn_weight must be float64")
        symbol = "mvg_msda_forward_f64"
    elif value.dtype == torch.bfloat16:
        sampling_loc, attn_weight = sampling_loc.float().contiguous(), attn_weight.float().contiguous()
        symbol = "mvg_msda_forward_bf16"
    else:
        raise RuntimeError("deform_forward: float32 / float64 / bfloat16 only (got %s)" % value.dtype)
    _launch(symbol, value, spatial_shapes, level_start_index, sampling_loc, attn_weight, out, N, S, M, D, nl, Lq, P)
    return out


def msda_backward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output, host=None):
    """Deformable.deform_backward (lib/models/ops/src/deform.h:53-72).  host: host_levels(...) of the two tables when the
    caller already has them (DeformFunction keeps the forward's).

    float32 with D = 32 runs the deterministic form (MVG_BACKWARD=atomic selects the reference's fp32-atomic scheme,
    MVG_BACKWARD=balanced the same deterministic chain with large bins cut into chunks of BACKWARD_CHUNK entries: det's bits): grad_value is
    summed in 64-bit fixed point with one scale PER IMAGE, 2^30 / (max |grad_output[n]| * max |attn_weight[n]|) over the finite
    entries -- any weight magnitude and any gradient magnitude down to 2^-96 are exact int32 contributions; what is smaller than
    2^-31 of its image's largest possible contribution rounds to zero.  Non-finite grad_output entries do not enter grad_value."""
    L.require_cuda(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output)
    if value.dtype == torch.bfloat16:
        return _msda_backward_bf16(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output, host)
    if value.dtype not in (torch.float32, torch.float64):
        raise RuntimeError("deform_backward: float32 / float64 only")        # AT_DISPATCH_FLOATING_TYPES, deform_cuda.cu:145
    for t in (sampling_loc, attn_weight, grad_output):
        if t.dtype != value.dtype:
            raise RuntimeError("deform_backward: all floating tensors must have value's dtype (%s)" % value.dtype)
    grad_output = grad_output.contiguous()
    N, S, M, D = value.shape
    _, Lq, _, nl, P, _ = sampling_loc.shape
    if value.dtype == torch.float32 and BACKWARD_MODE != "atomic":
        # deterministic form (csrc/msda_bwd.hip): binned by destination tile, fixed-point accumulation in LDS
        lib = L.load()
        shapes_c, starts_c = host if host is not None else host_levels(spatial_shapes, level_start_index)
        symbol, ws_bytes, tail = _det_entry(lib, False, (N, S, M, D, nl, Lq, P), shapes_c)
        if ws_bytes:
            ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=value.device)
            gv, gl, ga = torch.empty_like(value), torch.empty_like(sampling_loc), torch.empty_like(attn_weight)
            _launch(symbol, value, shapes_c, starts_c, sampling_loc, attn_weight, grad_output, gv, gl, ga, N, S, M, D, nl, Lq, P,
                    ws, ws_bytes, *tail, label="msda_backward_det")
            return gv, gl, ga
    gv = torch.zeros_like(value)                                             # deform_cuda.cu:132-134
    gl = torch.empty_like(sampling_loc)
    ga = torch.empty_like(attn_weight)
    _launch("mvg_msda_backward_f32" if value.dtype == torch.float32 else "mvg_msda_backward_f64", value, spatial_shapes,
            level_start_index, sampling_loc, attn_weight, grad_output, gv, gl, ga, N, S, M, D, nl, Lq, P)
    return gv, gl, ga


def _msda_backward_bf16(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output, host):
    """bf16 value (mixed-precision training), fp32 sampling_loc / attn_weight / grad_output -> three fp32 gradients.  The
    deterministic form reads the bf16 patch and widens it exactly (mvg_msda_backward_det_bf16): bit-identical to the fp32 call on
    value.float().  Where that form does not take the shape (workspace 0) or MVG_BACKWARD=atomic, the fp32 atomic kernel runs on
    value.float()."""
    for name, t in (("sampling_loc", sampling_loc), ("attn_weight", attn_weight), ("grad_output", grad_output)):
        if t.dtype != torch.float32:
            raise RuntimeError("deform_backward: with a bfloat16 value, %s must be float32 (got %s)" % (name, t.dtype))
    if not value.is_contiguous():
        raise RuntimeError("value tensor has to be contiguous")
    grad_output = grad_output.contiguous()
    N, S, M, D = value.shape
    _, Lq, _, nl, P, _ = sampling_loc.shape
    lib = L.load()
    if BACKWARD_MODE != "atomic":
        shapes_c, starts_c = host if host is not None else host_levels(spatial_shapes, level_start_index)
        symbol, ws_bytes, tail = _det_entry(lib, True, (N, S, M, D, nl, Lq, P), shapes_c)
        if ws_bytes:
            ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=value.device)
            gv = torch.empty(value.shape, dtype=torch.float32, device=value.device)
            gl, ga = torch.empty_like(sampling_loc), torch.empty_like(attn_weight)
            _launch(symbol, value, shapes_c, starts_c, sampling_loc, attn_weight, grad_output, gv, gl, ga, N, S, M, D, nl, Lq, P,
                    ws, ws_bytes, *tail, label="msda_backward_det_bf16")
            return gv, gl, ga
    v32 = value.float()
    gv = torch.zeros_like(v32)
    gl = torch.empty_like(sampling_loc)
    ga = torch.empty_like(attn_weight)
    _launch("mvg_msda_backward_f32", v32, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output, gv, gl, ga,
            N, S, M, D, nl, Lq, P)
    return gv, gl, ga


# ----------------------------------------------------------------------------- stage ops
def pyramid_level_views(feat, levels):
    """The L levels of a packed pyramid (n_img, S, C) as (n_img, C, H_l, W_l) tensors in channels-last strides --
    what a producer (the backbone's last deconvolutions run in torch.channels_last) writes into so that
    pack_pyramid has nothing left to do."""
    n_img, _, Cc = feat.shape
    views = []
    for l in range(levels.L):
        H, W = int(levels.shapes[l, 0]), int(levels.shapes[l, 1])
        st = int(levels.starts[l])
        views.append(feat[:, st:st + H * W, :].view(n_img, H, W, Cc).permute(0, 3, 1, 2))
    return views


def pack_pyramid(src_views, levels, dtype, out=None):
    """list of L (N_img,C,H,W) maps -> channels-last pyramid (N_img,S,C) in `dtype`.

    Per level, by layout of the producer's tensor:
      * it IS the level view of `out` (pyramid_level_views) in `dtype`: produced in place, nothing to do;
      * torch.channels_last memory format (fp32 / bf16 / fp16): one cast+copy, no transposition;
      * NCHW (what the reference's backbone emits, pose_resnet.py:198-216): LDS-tiled transpose kernel."""
    L.load()
    n_img, Cc = src_views[0].shape[:2]
    feat = out if out is not None else torch.empty((n_img, levels.S, Cc), dtype=dtype, device=src_views[0].device)
    if tuple(feat.shape) != (n_img, levels.S, Cc) or feat.dtype != dtype or not feat.is_contiguous():
        raise RuntimeError("pack_pyramid: out must be a contiguous (%d,%d,%d) %s tensor" % (n_img, levels.S, Cc, dtype))
    dst_views = pyramid_level_views(feat, levels)
    if len(src_views) != levels.L:
        raise RuntimeError("pack_pyramid: %d feature maps for %d levels" % (len(src_views), levels.L))
    if (all(s.dtype == torch.float32 and s.is_contiguous() and s.is_cuda and tuple(s.shape) ==
                                (n_img, Cc, int(levels.shapes[l, 0]), int(levels.shapes[l, 1])) and s.data_ptr() != dst_views[l].data_ptr()
                                for l, s in enumerate(src_views))):
        # the reference's hand-over format on every level: one launch for the whole pyramid
        ptrs = (C.c_void_p * levels.L)(*[s.data_ptr() for s in src_views])
        _launch("mvg_pack_pyramid", ptrs, feat, L.dtype_code(dtype), n_img, Cc, levels.shapes_c, levels.starts_c, levels.L,
                levels.S, label="pack_level")
        return feat
    for l, src in enumerate(src_views):
        L.require_cuda(src)
        H, W = int(levels.shapes[l, 0]), int(levels.shapes[l, 1])
        if tuple(src.shape) != (n_img, Cc, H, W):
            raise RuntimeError("src_views[%d] has shape %s, expected %s" % (l, tuple(src.shape), (n_img, Cc, H, W)))
        dst = dst_views[l]
        if src.data_ptr() == dst.data_ptr() and src.stride() == dst.stride() and src.dtype == dtype:
            continue
        if src.is_contiguous(memory_format=torch.channels_last) and not src.is_contiguous():
            with _timed("pack_level_nhwc"):
                dst.copy_(src)
            continue
        s = src.float().contiguous()
        one = (C.c_void_p * 1)(s.data_ptr())
        _launch("mvg_pack_pyramid", one, feat, L.dtype_code(dtype), n_img, Cc, (C.c_int64 * 2)(H, W),       # the same kernel on
                (C.c_int64 * 1)(int(levels.starts[l])), 1, levels.S, label="pack_level")                    # this level alone
    return feat


def _live_table(who, live, V, B, device):
    """live = (view_idx (B, V) i32, n_live (B) i32) on `device` (DecoderContext.set_live_views builds them) -> the pair, checked"""
    view_idx, n_live = live
    for t, shp in ((view_idx, (B, V)), (n_live, (B,))):
        if (not torch.is_tensor(t) or t.dtype != torch.int32 or tuple(t.shape) != shp or not t.is_contiguous()
                or t.device != torch.device(device)):
            raise RuntimeError("%s: live = (view_idx (%d, %d), n_live (%d,)) contiguous int32 on %s expected" % (who, B, V, B, device))
    return view_idx, n_live


def project(X, cams, levels, V, B, live=None):
    """live: the live-view table (_live_table); pairs of a dead view get inside = 0, r = ref_lvl = 0"""
    Lq = X.shape[1]
    r = torch.empty((V * B, Lq, 2), dtype=torch.float32, device=X.device)
    ref_lvl = torch.empty((V * B, Lq, levels.L, 2), dtype=torch.float32, device=X.device)
    inside = torch.empty((V * B, Lq), dtype=torch.uint8, device=X.device)
    if live is not None:
        _launch("mvg_project_live", X, cams, levels.shapes_c, levels.L, r, ref_lvl, inside, V, B, Lq,
                *_live_table("mvg_project_live", live, V, B, X.device))
    else:
        _launch("mvg_project", X, cams, levels.shapes_c, levels.L, r, ref_lvl, inside, V, B, Lq)
    return r, ref_lvl, inside


def gather_ref(feat, r, x, levels, V, B):
    """r: per-level reference points (n_img, Lq, L, 2)."""
    n_img, S, Cc = feat.shape
    Lq = r.shape[1]
    ain = torch.empty((n_img * Lq * levels.L, Cc), dtype=feat.dtype, device=feat.device)
    _launch("mvg_gather_ref", feat, L.dtype_code(feat.dtype), r, x, levels.shapes_c, levels.starts_c, ain, V, B, Lq, levels.L, S, Cc,
            label="gather_ref")
    return ain


def linear(a, w, bias, out_dtype=None, relu=False, rowmask=None, out=None, add=None):
    """out = act((a [+ add]) @ w.T + bias) (* rowmask).  a (M,K) f32|bf16; w (N,K) f32|bf16 (compute type); add: optional fp32
    tensor of a's shape and strides, summed with a on load (mvg_linear_sum)."""
    M, K = a.shape
    N = w.shape[0]
    out_dtype = out_dtype or (torch.float32 if w.dtype == torch.float32 else torch.bfloat16)
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype, device=a.device)
    if a.stride(1) != 1 or not w.is_contiguous() or out.stride(1) != 1:
        raise RuntimeError("mvg_linear: K-contiguous operands required")
    if add is not None and (add.dtype != torch.float32 or a.dtype != torch.float32 or add.shape != a.shape
                            or add.stride() != a.stride()):
        raise RuntimeError("mvg_linear_sum: the addend must be an fp32 tensor with a's shape and strides")
    _launch("mvg_linear_sum", a, add, L.dtype_code(a.dtype), a.stride(0), w, L.dtype_code(w.dtype), bias, out,
            L.dtype_code(out.dtype), out.stride(0), rowmask, 1 if relu else 0, M, N, K, label="linear_%dx%dx%d" % (M, N, K))
    return out


def linear_wgrad(dy, x, splits=None):
    """dW (N, K) = dy^T x for dy (rows, N), x (rows, K) fp32 row-major: linear_wgrad_bias without the bias gradient"""
    return linear_wgrad_bias(dy, x, want_bias=False, splits=splits)[0]


def linear_wgrad_bias(dy, x, want_bias=True, splits=None):
    """(dW (N, K), db (N) | None) = (dy^T x, column sums of dy) (mvg_linear_wgrad_bias_f32): the weight-gradient launch also leaves the
    bias gradient's per-slice partials, a second small launch adds both in slice order.  bf16 dy and x (both) run
    mvg_linear_wgrad_bias_bf16: one bf16 MFMA per 16 k, fp32 accumulation, fp32 dW / db, the same slices and order."""
    rows, N = dy.shape
    K = x.shape[1]
    if dy.dtype == torch.bfloat16 and x.dtype == torch.bfloat16:
        return _linear_wgrad_bias_bf16(dy, x, want_bias, splits)
    if (dy.dtype != torch.float32 or x.dtype != torch.float32 or dy.stride(1) != 1 or x.stride(1) != 1 or x.shape[0] != rows
            or N % 4 or K % 4):
        raise RuntimeError("mvg_linear_wgrad_bias: fp32 row-major (rows, N) / (rows, K) operands with N, K multiples of 4 required")
    if splits is None:
        splits = _wgrad_splits(rows, N, K)
    partial = torch.empty((splits, N, K), dtype=torch.float32, device=dy.device)
    dw = torch.empty((N, K), dtype=torch.float32, device=dy.device)
    pdb = torch.empty((splits, N), dtype=torch.float32, device=dy.device) if want_bias else None
    db = torch.empty((N,), dtype=torch.float32, device=dy.device) if want_bias else None
    _launch("mvg_linear_wgrad_bias_f32", dy, dy.stride(0), x, x.stride(0), partial, pdb, dw, db, rows, N, K, splits,
            label="linear_wgrad_bias_%dx%dx%d" % (N, K, rows))
    return dw, db


def _wgrad_splits(rows, N, K):
    tiles = ((N + 127) // 128) * ((K + 127) // 128)
    # ~512 workgroups (two per CU), at most 128 slices, at least 256 rows per slice (tools/bench_wgrad.py)
    return max(1, min((rows + 255) // 256, 128, (512 + tiles - 1) // tiles))


def _linear_wgrad_bias_bf16(dy, x, want_bias, splits):
    rows, N = dy.shape
    K = x.shape[1]
    if (dy.stride(1) != 1 or x.stride(1) != 1 or x.shape[0] != rows or N % 4 or K % 4 or dy.stride(0) % 4 or x.stride(0) % 4
            or dy.data_ptr() % 8 or x.data_ptr() % 8):
        raise RuntimeError("mvg_linear_wgrad_bias: bf16 row-major (rows, N) / (rows, K) operands with N, K and the row strides "
                           "multiples of 4 required")
    if rows == 0:
        return (torch.zeros((N, K), dtype=torch.float32, device=dy.device),
                torch.zeros((N,), dtype=torch.float32, device=dy.device) if want_bias else None)
    if splits is None:
        splits = _wgrad_splits(rows, N, K)
    partial = torch.empty((splits, N, K), dtype=torch.float32, device=dy.device)
    dw = torch.empty((N, K), dtype=torch.float32, device=dy.device)
    pdb = torch.empty((splits, N), dtype=torch.float32, device=dy.device) if want_bias else None
    db = torch.empty((N,), dtype=torch.float32, device=dy.device) if want_bias else None
    _launch("mvg_linear_wgrad_bias_bf16", dy, dy.stride(0), x, x.stride(0), partial, pdb, dw, db, rows, N, K, splits,
            label="linear_wgrad_bias_bf16_%dx%dx%d" % (N, K, rows))
    return dw, db


def linear_ordered(a, w, bias, order, inside, masked_row, relu=False, rowmask=None, out=None):
    """fp32 ``linear`` over the rows in processing order ``order`` (mvg_linear_ordered): tiles without a row of ``inside`` write
    ``masked_row`` (N,) to all their rows instead of computing them.  Rows keep their places in a / out."""
    M, K = a.shape
    N = w.shape[0]
    if a.dtype != torch.float32 or w.dtype != torch.float32 or a.stride(1) != 1 or not w.is_contiguous():
        raise RuntimeError("mvg_linear_ordered: fp32 K-contiguous operands required")
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    # the kernel indexes a / out through `order` and reads `inside` / `masked_row` unchecked: a stale order (another query count)
    # would read and write out of bounds
    if out.dtype != torch.float32 or tuple(out.shape) != (M, N) or out.stride(1) != 1:
        raise RuntimeError("mvg_linear_ordered: out must be an fp32 (%d, %d) tensor with contiguous rows" % (M, N))
    if order.dtype != torch.int32 or order.numel() != M or not order.is_contiguous():
        raise RuntimeError("mvg_linear_ordered: order must be a contiguous int32 tensor with one entry per row (%d)" % M)
    if inside.dtype != torch.uint8 or inside.numel() != M or not inside.is_contiguous():
        raise RuntimeError("mvg_linear_ordered: inside must be a contiguous uint8 tensor with one entry per row (%d)" % M)
    if masked_row.dtype != torch.float32 or masked_row.numel() != N or not masked_row.is_contiguous():
        raise RuntimeError("mvg_linear_ordered: masked_row must be a contiguous fp32 tensor with %d entries" % N)
    if rowmask is not None and (rowmask.dtype != torch.uint8 or rowmask.numel() != M or not rowmask.is_contiguous()):
        raise RuntimeError("mvg_linear_ordered: rowmask must be a contiguous uint8 tensor with one entry per row (%d)" % M)
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != N):
        raise RuntimeError("mvg_linear_ordered: bias must be fp32 with %d entries" % N)
    _launch("mvg_linear_ordered", a, a.stride(0), w, bias, out, out.stride(0), rowmask, 1 if relu else 0, M, N, K, order, inside,
            masked_row, label="linear_ordered_%dx%dx%d" % (M, N, K))
    return out


def msda_fused(value, oa, r, levels):
    """r: per-level reference points (n_img, Lq, L, 2)."""
    n_img, S, Cc = value.shape
    Lq = r.shape[1]
    samp = torch.empty((n_img * Lq, Cc), dtype=value.dtype, device=value.device)
    _launch("mvg_msda_fused", value, L.dtype_code(value.dtype), oa, r, levels.shapes_c, levels.starts_c, samp, n_img, Lq, levels.L, S,
            label="msda_fused")
    return samp


def msda_gfused_f32(value, G, xw, r, levels, B, pair_mask=None, order=None):
    """fp32 G-sampling (include/mvg_decoder.h: mvg_msda_gfused_f32): value (n_img,S,256) f32, G (n_img*S,192) f32 and
    xw (B*Lq,192) f32 in gsamp_column_order, r (n_img,Lq,L,2) -> samp (n_img*Lq,256) f32."""
    n_img, S, Cc = value.shape
    Lq = r.shape[1]
    assert value.dtype == torch.float32 and G.dtype == torch.float32 and xw.dtype == torch.float32 and Cc == 256
    assert G.is_contiguous() and tuple(G.shape) == (n_img * S, 192) and xw.is_contiguous() and xw.shape[1] == 192
    samp = torch.empty((n_img * Lq, 256), dtype=torch.float32, device=value.device)
    if pair_mask is not None:
        assert pair_mask.dtype == torch.uint8 and pair_mask.numel() == n_img * Lq and pair_mask.is_contiguous()
    if order is not None:
        assert order.dtype == torch.int32 and order.numel() == n_img * Lq and order.is_contiguous()
    _launch("mvg_msda_gfused_f32", value, G, xw, r, levels.shapes_c, levels.starts_c, samp, pair_mask, order, n_img, Lq, levels.L, S,
            B, label="msda_gfused_f32")
    return samp


def value_proj_planes_ws(feat, w_frag, bias, vp):
    """weight-stationary value projection (bf16 feat, swizzled weight) into head planes vh[img][head][s][32]: a one-product launch
    of mvg_pyramid_group_ws."""
    pyramid_group_ws(feat, [(w_frag, bias, vp, True)], label="value_proj_ws")
    return vp


def feat_linear_ws(feat, w_frag, N=192, out=None):
    """G = feat @ W^T, row-major bf16 (n_img*S, 192) (weight-stationary kernel, no bias): a one-product launch of
    mvg_pyramid_group_ws."""
    n_img, S, _ = feat.shape
    if N != 192:
        raise RuntimeError("feat_linear_ws: 192 columns (the [offsets | logits] Linear of the G-sampling form)")
    G = out if out is not None else torch.empty((n_img * S, N), dtype=torch.bfloat16, device=feat.device)
    pyramid_group_ws(feat, [(w_frag, None, G, False)], label="feat_linear_ws")
    return G


def pyramid_group_ws(feat, jobs, slots=0, label=None):
    """Several weight-stationary products of the same packed bf16 pyramid in one launch (mvg_pyramid_group_ws): jobs = list of
    (w_frag, bias or None, out, planes) -- planes: value projection into head planes (out = vh (n_img, 8, S, 32)), else
    G = feat @ W^T row-major (out (n_img*S, 192)).  Outputs bit-identical to value_proj_planes_ws / feat_linear_ws.
    slots: workgroups per XCD (0 = the library default, all 64 resident ones; fewer leave room for kernels running next to it)."""
    n_img, S, K = feat.shape
    n = len(jobs)
    assert 1 <= n <= 8 and K == 256 and feat.dtype == torch.bfloat16 and feat.is_contiguous()
    for w, b, out, planes in jobs:
        assert out.dtype == torch.bfloat16 and out.is_contiguous() and out.numel() == n_img * S * (256 if planes else 192)
        assert w.dtype == torch.bfloat16 and w.numel() == 256 * 256 and (b is not None or not planes)
    vpp = C.c_void_p * n
    Wf = vpp(*[w.data_ptr() for w, _, _, _ in jobs])
    bias = vpp(*[(b.data_ptr() if b is not None else None) for _, b, _, _ in jobs])
    outs = vpp(*[o.data_ptr() for _, _, o, _ in jobs])
    Ns = (C.c_int * n)(*[256 if p else 192 for _, _, _, p in jobs])
    planes = (C.c_int * n)(*[1 if p else 0 for _, _, _, p in jobs])
    _launch("mvg_pyramid_group_ws", feat, n_img, S, n, Wf, bias, outs, Ns, planes, int(slots),
            label=label or "pyramid_group_ws_%d" % n)


def gsamp_column_order(device=None):
    """Row permutation of [sampling_offsets.weight (128); attention_weights.weight (64)] that msda_gsamp expects
    for G and xw: 8 groups of (16 offset rows | 8 logit rows).  With the reference's memory reinterpretation
    (projattn.py:180-184) head m of a level row uses whole groups, so its 72 values are contiguous in a G row."""
    j = torch.arange(192, dtype=torch.long, device=device)       # built on the device: legal during graph capture
    g, w = j // 24, j % 24
    return torch.where(w < 16, 16 * g + w, 128 + 8 * g + (w - 16))


def msda_gsamp(vp, G, xw, r, levels, B, pair_mask=None, order=None, out=None):
    """fused sampling with in-kernel gather of the offsets/logits from G (see include/mvg_decoder.h); the 192
    columns of G and xw are in gsamp_column_order().
    pair_mask (n_img*Lq) u8: rows with 0 are zero-filled, not sampled; order (n_img*Lq) i32 from bin_pairs."""
    n_img = vp.shape[0]
    Lq = r.shape[1]
    samp = out if out is not None else torch.empty((n_img * Lq, 256), dtype=torch.bfloat16, device=vp.device)
    assert samp.dtype == torch.bfloat16 and tuple(samp.shape) == (n_img * Lq, 256) and samp.is_contiguous()
    if pair_mask is not None:
        assert pair_mask.dtype == torch.uint8 and pair_mask.numel() == n_img * Lq and pair_mask.is_contiguous()
    if order is not None:
        assert order.dtype == torch.int32 and order.numel() == n_img * Lq and order.is_contiguous()
    _launch("mvg_msda_gsamp", vp, G, xw, r, levels.shapes_c, levels.starts_c, samp, pair_mask, order, n_img, Lq, levels.L, levels.S,
            B, label="msda_gsamp")
    return samp


def bin_pairs(r, inside, levels, out=None):
    """processing order of the (image, query) pairs for msda_gsamp: Morton-sorted by level-0 cell block, pairs with
    inside == 0 last.  r (n_img, Lq, L, 2) per-level reference points; inside (n_img, Lq) u8 or None."""
    n_img, Lq = r.shape[0], r.shape[1]
    if Lq > 65536:          # the binning kernel keeps a thread's keys in registers (<= 64 per thread)
        return None
    if out is None:
        out = torch.empty((n_img * Lq,), dtype=torch.int32, device=r.device)
    order = out
    lib = L.load()
    ws_bytes = int(lib.mvg_bin_pairs_workspace(n_img, Lq))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=r.device) if ws_bytes else None     # multi-workgroup variant
    _launch("mvg_bin_pairs", r, inside, levels.shapes_c, levels.L, order, n_img, Lq, ws, ws_bytes, label="bin_pairs")
    return order


_SIDE_STREAMS = {}


def side_stream(device):
    """one auxiliary HIP stream per device for small kernels that overlap with the main stream (fork/join with
    wait_stream: legal inside HIP-graph capture)."""
    idx = torch.device(device).index
    if idx is None:
        idx = torch.cuda.current_device()
    if idx not in _SIDE_STREAMS:
        _SIDE_STREAMS[idx] = torch.cuda.Stream(device=idx)
    return _SIDE_STREAMS[idx]


def swizzle_weight(w):
    """nn.Linear weight (N, K) bf16 with N % 256 == 0 -> MFMA-fragment order of csrc/chain.hip:
    Wf[nb N/256][wn 4][ks K/16][j 2][lane 64][8], lane = h*32 + rl holds
    W[nb*256 + wn*64 + j*32 + rl][ks*16 + h*8 : +8]."""
    N, K = w.shape
    assert N % 256 == 0 and K % 16 == 0, (N, K)
    t = w.reshape(N // 256, 4, 2, 32, K // 16, 2, 8)          # nb, wn, j, rl, ks, h, e
    return t.permute(0, 1, 4, 2, 5, 3, 6).contiguous().reshape(-1)


def split_swizzle_weight_h2(w, pad_rows_to=256):
    """fp32 nn.Linear weight (N, K) -> the operand of the two-part fp16 kernels (csrc/f32s.hip, "f32h"): (planes, s) with
    w 2^s = h + l, h = fp16(w 2^s), l = fp16(w 2^s - h), s chosen so that max |w| 2^s lies in [2^13, 2^14); each plane in swizzle_weight
    order, concatenated (N zero-padded to a multiple of 256).  One host sync (the tensor's maximum) when the operand cache is built."""
    w = w.detach().float()
    N, K = w.shape
    Np = (N + pad_rows_to - 1) // pad_rows_to * pad_rows_to
    if Np != N:
        w = torch.cat([w, w.new_zeros(Np - N, K)], 0)
    mx = float(w.abs().max())
    s = 0 if not (mx > 0 and math.isfinite(mx)) else max(-100, min(100, 13 - math.frexp(mx)[1] + 1))
    ws = torch.ldexp(w, torch.tensor(s, device=w.device))
    h = ws.to(torch.float16)
    l = (ws - h.float()).to(torch.float16)
    return torch.cat([swizzle_weight(p) for p in (h, l)]), s


def pyramid_f32h(feat, Wv_planes, wv_scale, bv, Wg_planes, wg_scale, n_g, value=None, G=None):
    """value = feat Wv^T + bv (n_img, S, 256) and G = feat Wg^T (n_img*S, n_g), fp32, in one pass over the channels-last fp32
    pyramid feat (n_img, S, 256) on two-part fp16 operands (include/mvg_decoder.h: mvg_pyramid_f32h); weights from
    split_swizzle_weight_h2."""
    n_img, S, Cc = feat.shape
    if feat.dtype != torch.float32 or Cc != 256 or not feat.is_contiguous():
        raise RuntimeError("mvg_pyramid_f32h: contiguous fp32 (n_img, S, 256) pyramid required")
    rows = n_img * S
    for t in (Wv_planes, Wg_planes):
        if t.dtype != torch.float16 or t.numel() != 2 * 256 * 256 or not t.is_contiguous():
            raise RuntimeError("mvg_pyramid_f32h: weight planes from split_swizzle_weight_h2 required")
    if value is None:
        value = torch.empty((n_img, S, 256), dtype=torch.float32, device=feat.device)
    if G is None:
        G = torch.empty((rows, n_g), dtype=torch.float32, device=feat.device)
    assert value.dtype == torch.float32 and value.numel() == rows * 256 and value.is_contiguous()
    assert G.dtype == torch.float32 and tuple(G.shape) == (rows, n_g) and G.is_contiguous()
    _launch("mvg_pyramid_f32h", feat, Wv_planes, int(wv_scale), bv, Wg_planes, int(wg_scale), value, G, rows, n_g,
            label="pyramid_f32h")
    return value, G


def chain_attn_pose_f32h(samp, inside, Wp, swp, bp, W0, sw0, b0, W1, sw1, b1, W2, b2, order=None, o_masked=None):
    """fp32 chain A on two-part fp16 operands (include/mvg_decoder.h: mvg_chain_attn_pose_f32h): samp (rows, 256) f32 -> (attn f32
    (rows, 256), o f32 (rows, 3)); (Wp, swp) / (W0, sw0) / (W1, sw1) from split_swizzle_weight_h2."""
    rows = samp.shape[0]
    if samp.dtype != torch.float32 or samp.shape[1] != 256 or not samp.is_contiguous():
        raise RuntimeError("mvg_chain_attn_pose_f32h: contiguous fp32 (rows, 256) samples required")
    for t in (Wp, W0, W1):
        if t.dtype != torch.float16 or t.numel() != 2 * 256 * 256 or not t.is_contiguous():
            raise RuntimeError("mvg_chain_attn_pose_f32h: weight planes from split_swizzle_weight_h2 required")
    if inside.dtype != torch.uint8 or inside.numel() != rows or not inside.is_contiguous():
        raise RuntimeError("mvg_chain_attn_pose_f32h: inside must be a contiguous uint8 tensor with one entry per row")
    if W2.dtype != torch.float32 or tuple(W2.shape) != (3, 256) or not W2.is_contiguous():
        raise RuntimeError("mvg_chain_attn_pose_f32h: the last pose layer's (3, 256) fp32 weight required")
    if order is not None:
        assert order.dtype == torch.int32 and order.numel() == rows and order.is_contiguous()
    attn = torch.empty((rows, 256), dtype=torch.float32, device=samp.device)
    o = torch.empty((rows, 3), dtype=torch.float32, device=samp.device)
    _launch("mvg_chain_attn_pose_f32h", samp, inside, Wp, int(swp), bp, W0, int(sw0), b0, W1, int(sw1), b1, W2, b2, attn, o, order,
            o_masked, rows, label="chain_attn_pose_f32h")
    return attn, o


def chain_masked_row_output_f32h(Wp, swp, bp, W0, sw0, b0, W1, sw1, b1, W2, b2):
    """o (3,) f32 of a row with inside == 0 as the two-part fp16 chain A computes it (the chain run on one masked row)."""
    dev = Wp.device
    samp = torch.zeros((1, 256), dtype=torch.float32, device=dev)
    inside = torch.zeros((1,), dtype=torch.uint8, device=dev)
    global PROFILE
    saved, PROFILE = PROFILE, None
    try:
        _, o = chain_attn_pose_f32h(samp, inside, Wp, swp, bp, W0, sw0, b0, W1, sw1, b1, W2, b2)
    finally:
        PROFILE = saved
    return o.reshape(3)


def chain_update_ffn_class_f32h(attn, V, tgt, Wu, su, bu, g2, be2, W1, s1, b1, W2, s2, b2, g3, be3, Wc, bc, threshold, B, NQ, J,
                                forced_valid=None, has_ffn=True, tgt_out=None, any_valid=None, next_query_proj=None, live=None):
    """fp32 chain B on two-part fp16 operands (include/mvg_decoder.h: mvg_chain_update_ffn_class_f32h); arguments and results as
    chain_update_ffn_class, attn (V * rows, 256) f32, weights (planes, scale) from split_swizzle_weight_h2, next_query_proj = (qpos, Wn, sn, bn, n_next)."""
    dev = attn.device
    rows = B * NQ * J
    if attn.dtype != torch.float32 or attn.numel() != V * rows * 256 or not attn.is_contiguous():
        raise RuntimeError("mvg_chain_update_ffn_class_f32h: contiguous fp32 (V * rows, 256) attn required")
    assert tgt.dtype == torch.float32 and tgt.numel() == rows * 256 and tgt.is_contiguous()
    assert Wu.dtype == torch.float16 and Wu.numel() == 2 * 256 * 256
    if has_ffn:
        assert W1.dtype == torch.float16 and W1.numel() == 2 * 1024 * 256 and W2.dtype == torch.float16 and W2.numel() == 2 * 256 * 1024
    if tgt_out is None:
        tgt_out = torch.empty((rows, 256), dtype=torch.float32, device=dev)
    else:
        assert tgt_out.dtype == torch.float32 and tgt_out.numel() == rows * 256 and tgt_out.is_contiguous()
        tgt_out = tgt_out.view(rows, 256)
    prob = torch.empty((B, NQ, 2), dtype=torch.float32, device=dev)
    valid = torch.empty((B, NQ), dtype=torch.uint8, device=dev)
    qpos = Wn = bn = xw_next = None
    n_next = sn = 0
    if next_query_proj is not None:
        qpos, Wn, sn, bn, n_next = next_query_proj
        assert Wn.dtype == torch.float16 and Wn.numel() == 2 * 256 * 256 and bn.numel() == 256 and bn.dtype == torch.float32
        if qpos is not None:
            assert qpos.dtype == torch.float32 and qpos.numel() == rows * 256 and qpos.is_contiguous()
        xw_next = torch.empty((rows, n_next), dtype=torch.float32, device=dev)
    if any_valid is None:
        any_valid = torch.zeros((1,), dtype=torch.int32, device=dev)
    sym = "mvg_chain_update_ffn_class_f32h" if live is None else "mvg_chain_update_ffn_class_f32h_live"
    _launch(sym, attn, V, tgt, Wu, int(su), bu, g2, be2, W1, int(s1 or 0), b1, W2, int(s2 or 0), b2, g3,
            be3, Wc, bc, float(threshold), forced_valid, tgt_out, prob, valid, any_valid, qpos, Wn, int(sn), bn, xw_next, n_next,
            B, NQ, J, 1 if has_ffn else 0, *(() if live is None else _live_table(sym, live, V, B, dev)),
            label="chain_update_ffn_class_f32h")
    if next_query_proj is not None:
        return tgt_out, prob, valid, any_valid, xw_next
    return tgt_out, prob, valid, any_valid


def chain_attn_pose(samp, inside, Wp, bp, W0, b0, W1, b1, W2, b2, order=None, o_masked=None):
    """fused output_proj (* in-image mask) + 3-layer pose MLP; Wp/W0/W1 in swizzle_weight order.
    order (rows) i32: row processing order (bin_pairs: masked rows last); o_masked (3) f32 from
    chain_masked_row_output: lets all-masked 64-row tiles skip the chain.
    Returns (attn bf16 (rows,256), o f32 (rows,3))."""
    rows = samp.shape[0]
    attn = torch.empty((rows, 256), dtype=torch.bfloat16, device=samp.device)
    o = torch.empty((rows, 3), dtype=torch.float32, device=samp.device)
    if order is not None:
        assert order.dtype == torch.int32 and order.numel() == rows and order.is_contiguous()
    _launch("mvg_chain_attn_pose", samp, inside, Wp, bp, W0, b0, W1, b1, W2, b2, attn, o, order, o_masked, rows,
            label="chain_attn_pose")
    return attn, o


def chain_masked_row_output(Wp, bp, W0, b0, W1, b1, W2, b2):
    """o (3,) f32 of a row with inside == 0: the chain run on one masked row (weights only -> cacheable)."""
    dev = Wp.device
    samp = torch.zeros((1, 256), dtype=torch.bfloat16, device=dev)
    inside = torch.zeros((1,), dtype=torch.uint8, device=dev)
    global PROFILE
    saved, PROFILE = PROFILE, None
    try:
        _, o = chain_attn_pose(samp, inside, Wp, bp, W0, b0, W1, b1, W2, b2)
    finally:
        PROFILE = saved
    return o.reshape(3)


def chain_update_ffn_class(attn, V, tgt, Wu, bu, g2, be2, W1, b1, W2, b2, g3, be3, Wc, bc, threshold, B, NQ, J,
                           forced_valid=None, has_ffn=True, tgt_out=None, any_valid=None, next_query_proj=None, attn_inside=None,
                           live=None):
    """fused view-mean + update MLP + LN2 + FFN + LN3 + class head (weights in swizzle_weight order).
    attn_inside (V * rows) u8: chain A's in-image flags -- attn rows with flag 0 are zero and are not read.
    live: the live-view table (_live_table) -- the mean is the one over the live views of the row's stream.
    Returns (tgt_update f32 (B*NQ*J,256), prob (B,NQ,2), valid (B,NQ) u8, any_valid int32[1])."""
    dev = attn.device
    rows = B * NQ * J
    if tgt_out is None:
        tgt_out = torch.empty((rows, 256), dtype=torch.float32, device=dev)
    else:       # caller-owned destination (e.g. a slice of the stacked per-layer output)
        assert tgt_out.dtype == torch.float32 and tgt_out.numel() == rows * 256 and tgt_out.is_contiguous()
        tgt_out = tgt_out.view(rows, 256)
    prob = torch.empty((B, NQ, 2), dtype=torch.float32, device=dev)
    valid = torch.empty((B, NQ), dtype=torch.uint8, device=dev)
    # next_query_proj = (query_pos (rows,256) f32 | None, W_next fragments (256,256) bf16, b_next (256,) f32, n_next):
    # also emit xw_next = (tgt' + query_pos) @ W_next^T + b_next for the next layer's sampler
    qpos = Wn = bn = xw_next = None
    n_next = 0
    if next_query_proj is not None:
        qpos, Wn, bn, n_next = next_query_proj
        assert Wn.dtype == torch.bfloat16 and Wn.numel() == 256 * 256 and bn.numel() == 256 and bn.dtype == torch.float32
        if qpos is not None:
            assert qpos.dtype == torch.float32 and qpos.numel() == rows * 256 and qpos.is_contiguous()
        xw_next = torch.empty((rows, n_next), dtype=torch.float32, device=dev)
    if any_valid is None:       # else: a caller-owned int32[1] that is already zero
        any_valid = torch.zeros((1,), dtype=torch.int32, device=dev)
    if attn_inside is not None:
        assert attn_inside.dtype == torch.uint8 and attn_inside.numel() == V * rows and attn_inside.is_contiguous()
    sym = "mvg_chain_update_ffn_class" if live is None else "mvg_chain_update_ffn_class_live"
    _launch(sym, attn, V, tgt, Wu, bu, g2, be2, W1, b1, W2, b2, g3, be3, Wc, bc, float(threshold),
            forced_valid, tgt_out, prob, valid, any_valid, qpos, Wn, bn, xw_next, n_next, B, NQ, J, 1 if has_ffn else 0, attn_inside,
            *(() if live is None else _live_table(sym, live, V, B, dev)), label="chain_update_ffn_class")
    if next_query_proj is not None:
        return tgt_out, prob, valid, any_valid, xw_next
    return tgt_out, prob, valid, any_valid


def mean_views(attn, V, live=None):
    """live: the live-view table (_live_table; its B streams split the rows evenly) -- the mean over the live views of the row's stream"""
    rows = attn.shape[0] // V
    out = torch.empty((rows, attn.shape[1]), dtype=attn.dtype, device=attn.device)
    if live is not None:
        B = live[1].shape[0]
        if rows % B:
            raise RuntimeError("mvg_mean_views_live: %d rows do not split into %d streams" % (rows, B))
        _launch("mvg_mean_views_live", attn, L.dtype_code(attn.dtype), out, V, B, rows, attn.shape[1],
                *_live_table("mvg_mean_views_live", live, V, B, attn.device))
    else:
        _launch("mvg_mean_views", attn, L.dtype_code(attn.dtype), out, V, rows, attn.shape[1])
    return out


def add_layernorm(res, h, gamma, beta):
    rows, Cc = res.shape
    y = torch.empty((rows, Cc), dtype=torch.float32, device=res.device)
    _launch("mvg_add_layernorm", res, h, L.dtype_code(h.dtype), gamma, beta, y, rows, Cc)
    return y


def self_attention(q, k, v):
    """softmax(q k^T / sqrt(32)) v per (batch element, head) on the fused kernel (csrc/mha.hip): q, k, v (B, Lq, 256) float32 or
    bfloat16 (all the same), 8 heads in columns 32 h .. 32 h + 31 -- what nn.MultiheadAttention computes between its in- and
    out-projection.  Each may be a column block of a wider (B, Lq, n) tensor (last stride 1, batch stride Lq * row stride): the
    in-projection's output is attended where it lies.  Returns (B, Lq, 256) in the inputs' dtype.  Finite inputs only."""
    B, Lq, Cc = _attention_operands("self_attention", q=q, k=k, v=v)
    out = torch.empty((B, Lq, Cc), dtype=q.dtype, device=q.device)
    _launch("mvg_self_attention", q, k, v, out, q.stride(1), k.stride(1), v.stride(1), B, Lq, Cc, 8, L.dtype_code(q.dtype),
            label="self_attention")
    return out


def _attention_operands(fn, **tensors):
    """the checks the attention kernels' (B, Lq, 256) operands share; the first one sets shape, dtype and device.  -> (B, Lq, C)"""
    L.require_cuda(*tensors.values())
    names, ts = ", ".join(tensors), list(tensors.values())
    q = ts[0]
    if q.dim() != 3 or any(t.shape != q.shape for t in ts):
        raise RuntimeError("%s: %s of one shape (B, Lq, C) expected, got %s" % (fn, names, " ".join(str(tuple(t.shape)) for t in ts)))
    B, Lq, Cc = q.shape
    if Cc != 256 or Lq < 1 or B < 1:
        raise RuntimeError("%s: built for d_model 256 (8 heads of 32), B >= 1, Lq >= 1; got %s" % (fn, tuple(q.shape)))
    if q.dtype not in (torch.float32, torch.bfloat16) or any(t.dtype != q.dtype for t in ts):
        raise RuntimeError("%s: %s all float32 or all bfloat16, got %s" % (fn, names, " ".join(str(t.dtype) for t in ts)))
    if any(t.device != q.device for t in ts):
        raise RuntimeError("%s: %s on one device expected" % (fn, names))
    vec = 16 // q.element_size()
    for name, t in tensors.items():
        if t.stride(2) != 1 or (B > 1 and t.stride(0) != Lq * t.stride(1)) or t.stride(1) < Cc or t.stride(1) % vec \
                or t.data_ptr() % 16:
            raise RuntimeError("%s: %s must be row-major (a column block of a row-major tensor at most), 16-byte "
                               "aligned rows; strides %s" % (fn, name, t.stride()))
    return B, Lq, Cc


def _attention_seed(fn, p_drop, seed, device):
    """p_drop in [0, 1); with p_drop > 0 the seed is a 1-element int64 tensor on the device (the kernels read it there)"""
    p_drop = float(p_drop)
    if not 0.0 <= p_drop < 1.0:
        raise RuntimeError("%s: p_drop in [0, 1) expected, got %r" % (fn, p_drop))
    if p_drop > 0.0 and (seed is None or seed.dtype != torch.int64 or seed.numel() != 1 or seed.device != device):
        raise RuntimeError("%s: dropout needs seed, a 1-element int64 tensor on %s" % (fn, device))
    return p_drop, (seed if p_drop > 0.0 else None)


def dropout_p_quantised(p_drop):
    """the probability the attention kernels drop with: p_drop rounded to 8 bits (at most 255 / 256)"""
    return min(255, int(float(p_drop) * 256.0 + 0.5)) / 256.0


def self_attention_train(q, k, v, p_drop=0.0, seed=None):
    """self_attention for training (mvg_self_attention_train): -> (out, lse).  out as self_attention gives it (the same bits with
    p_drop == 0), lse (B, 8, Lq) float32 = ln sum_j exp(q_i . k_j / sqrt(32)) for self_attention_backward.  p_drop > 0: attention
    dropout inside the kernel, out = (keep o P / (1 - p_q)) v with p_q = dropout_p_quantised(p_drop) and keep a function of
    (seed, b, head, query, key) alone (self_attention_dropout_mask); seed: 1-element int64 device tensor, read by the kernel."""
    B, Lq, Cc = _attention_operands("self_attention_train", q=q, k=k, v=v)
    p_drop, seed = _attention_seed("self_attention_train", p_drop, seed, q.device)
    out = torch.empty((B, Lq, Cc), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, 8, Lq), dtype=torch.float32, device=q.device)
    _launch("mvg_self_attention_train", q, k, v, out, lse, q.stride(1), k.stride(1), v.stride(1), B, Lq, Cc, 8,
            L.dtype_code(q.dtype), p_drop, seed, label="self_attention_train")
    return out, lse


def self_attention_backward(q, k, v, out, dout, lse, p_drop=0.0, seed=None):
    """(dq, dk, dv) of self_attention_train's out (mvg_self_attention_backward: deterministic, no atomics), in the inputs' dtype,
    contiguous.  q, k, v, lse, p_drop, seed as the forward had them; out as it returned it; dout (B, Lq, 256) contiguous."""
    B, Lq, Cc = _attention_operands("self_attention_backward", q=q, k=k, v=v, out=out, dout=dout)
    p_drop, seed = _attention_seed("self_attention_backward", p_drop, seed, q.device)
    if not out.is_contiguous() or not dout.is_contiguous():
        raise RuntimeError("self_attention_backward: out, dout must be row-major and contiguous; strides %s %s" % (out.stride(), dout.stride()))
    if lse.shape != (B, 8, Lq) or lse.dtype != torch.float32 or not lse.is_contiguous() or lse.device != q.device:
        raise RuntimeError("self_attention_backward: lse (B, 8, Lq) float32 contiguous expected, got %s %s" % (tuple(lse.shape), lse.dtype))
    dq, dk, dv = (torch.empty((B, Lq, Cc), dtype=q.dtype, device=q.device) for _ in range(3))
    nbytes = int(L.load().mvg_self_attention_backward_workspace(B, Lq))
    ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=q.device)
    _launch("mvg_self_attention_backward", q, k, v, out, dout, lse, dq, dk, dv, q.stride(1), k.stride(1), v.stride(1), Cc, Cc, Cc,
            B, Lq, Cc, 8, L.dtype_code(q.dtype), p_drop, seed, ws, nbytes, label="self_attention_backward")
    return dq, dk, dv


def self_attention_dropout_mask(B, Lq, p_drop, seed):
    """(B, 8, Lq, Lq) uint8 keep mask of the attention dropout for `seed` (1 = kept), from the device function the training
    kernels call (mvg_self_attention_dropout_mask): a test and debugging aid, Lq <= 1024."""
    L.require_cuda(seed)
    p_drop, seed = _attention_seed("self_attention_dropout_mask", p_drop, seed, None if seed is None else seed.device)
    if B < 1 or not 1 <= Lq <= 1024:
        raise RuntimeError("self_attention_dropout_mask: B >= 1, 1 <= Lq <= 1024 expected, got B %d Lq %d" % (B, Lq))
    mask = torch.empty((B, 8, Lq, Lq), dtype=torch.uint8, device="cuda" if seed is None else seed.device)
    _launch("mvg_self_attention_dropout_mask", mask, B, Lq, p_drop, seed)
    return mask


def class_head(tgt, Wc, bc, threshold, B, NQ, J, forced_valid=None):
    Cc = tgt.shape[-1]
    prob = torch.empty((B, NQ, 2), dtype=torch.float32, device=tgt.device)
    valid = torch.empty((B, NQ), dtype=torch.uint8, device=tgt.device)
    any_valid = torch.zeros((1,), dtype=torch.int32, device=tgt.device)
    _launch("mvg_class_head", tgt, Wc, bc, float(threshold), forced_valid, prob, valid, any_valid, B, NQ, J, Cc)
    return prob, valid, any_valid


def rowdot3(h, W3, b3):
    rows, Cc = h.shape
    o = torch.empty((rows, 3), dtype=torch.float32, device=h.device)
    _launch("mvg_rowdot3", h, L.dtype_code(h.dtype), W3, b3, o, rows, Cc)
    return o


def triangulate(r, o, cams, valid, any_valid, V, B, NQ, J, out=None, next_levels=None, live=None):
    """live: the live-view table (_live_table) -- the problem of a token is the one of its stream's live views; 2D outputs and next
    projections of dead views are zeros.
    out: optional caller-owned (new_ref (B,Lq,3), ref2d (B,V,Lq,2), proj2d (B,V,Lq,2)) contiguous f32 destinations
    (e.g. slices of the stacked per-layer outputs).  next_levels (a Levels): also project the new points for the next
    layer in the same launch -> returns (new_ref, ref2d, proj2d, (r_next, ref_lvl_next, inside_next))."""
    Lq = NQ * J
    dev = r.device
    if out is not None:
        new_ref, ref2d, proj2d = out
        for t, shp in ((new_ref, (B, Lq, 3)), (ref2d, (B, V, Lq, 2)), (proj2d, (B, V, Lq, 2))):
            assert tuple(t.shape) == shp and t.dtype == torch.float32 and t.is_contiguous()
    else:
        new_ref = torch.empty((B, Lq, 3), dtype=torch.float32, device=dev)
        ref2d = torch.empty((B, V, Lq, 2), dtype=torch.float32, device=dev)
        proj2d = torch.empty((B, V, Lq, 2), dtype=torch.float32, device=dev)
    sfx, tab = ("", ()) if live is None else ("_live", _live_table("mvg_triangulate_live", live, V, B, dev))
    if next_levels is not None:
        lv = next_levels
        r_n = torch.empty((V * B, Lq, 2), dtype=torch.float32, device=dev)
        ref_n = torch.empty((V * B, Lq, lv.L, 2), dtype=torch.float32, device=dev)
        in_n = torch.empty((V * B, Lq), dtype=torch.uint8, device=dev)
        _launch("mvg_triangulate_project" + sfx, r, o, cams, valid, any_valid, new_ref, ref2d, proj2d, V, B, NQ, J, lv.shapes_c, lv.L,
                r_n, ref_n, in_n, *tab, label="triangulate_project")
        return new_ref, ref2d, proj2d, (r_n, ref_n, in_n)
    _launch("mvg_triangulate" + sfx, r, o, cams, valid, any_valid, new_ref, ref2d, proj2d, V, B, NQ, J, *tab, label="triangulate")
    return new_ref, ref2d, proj2d


# ------------------------------------------------------------------------- camera packing
def pack_cameras(meta, img_size, device):
    """meta (list[V] of per-view dicts, JointsDataset.py:197-220) -> (V*B, CAM_STRIDE) fp32
    device tensor, image index n = v*B + b.  The crop affine is the closed form of
    get_affine_transform(center, scale, 0, img_size) (lib/utils/transforms.py:72-112) that the
    reference evaluates with numpy/cv2 per view per layer (dq_decoder.py:361-372); here it is
    computed once per forward."""
    V = len(meta)
    B = meta[0]["center"].shape[0]
    rec = np.zeros((V, B, L.CAM_STRIDE), dtype=np.float32)
    wh_all = []
    for v, m in enumerate(meta):
        cam = {k: t.detach().float().cpu().numpy() for k, t in m["camera"].items()
               if k in ("R", "T", "fx", "fy", "cx", "cy", "k", "p")}
        center = m["center"].detach().cpu().numpy().astype(np.float64)            # (B,2)
        scale = m["scale"].detach().cpu().numpy().astype(np.float32)
        inv = m["inv_affine_trans"].detach().cpu().numpy().astype(np.float64)[:, :2, :]
        rec[v, :, 0:9] = cam["R"].reshape(B, 9)
        rec[v, :, 9:12] = cam["T"].reshape(B, 3)
        rec[v, :, 12], rec[v, :, 13] = cam["fx"].reshape(B), cam["fy"].reshape(B)
        rec[v, :, 14], rec[v, :, 15] = cam["cx"].reshape(B), cam["cy"].reshape(B)
        rec[v, :, 16:19] = cam["k"].reshape(B, 3)
        rec[v, :, 19:21] = cam["p"].reshape(B, 2)
        c32 = center.astype(np.float32).astype(np.float64)
        st = (scale * np.float32(200.0)).astype(np.float64)
        dw, dh = float(img_size[0]), float(img_size[1])
        s = np.where(st[:, 0] >= st[:, 1], dw / st[:, 0], dh / st[:, 1])
        rec[v, :, 21], rec[v, :, 25] = s, s
        rec[v, :, 23] = dw * 0.5 - s * c32[:, 0]
        rec[v, :, 26] = dh * 0.5 - s * c32[:, 1]
        rec[v, :, 27:33] = inv.reshape(B, 6)
        wh = center * 2.0
        rec[v, :, 33:35] = wh
        rec[v, :, 35] = wh.max()                                                   # dq_decoder.py:383 (whole-batch max)
        rec[v, :, 36], rec[v, :, 37] = dw, dh
        wh_all.append(wh)
    return torch.from_numpy(rec.reshape(V * B, L.CAM_STRIDE)).to(device)


def uncrop_undistort_jac(ref2d, cams, V, B):
    """ref2d (B, V, Lq, 2) f32 -> (ud (B, V, Lq, 2), jac (B, V, Lq, 2, 2) = d ud / d ref2d) (mvg_uncrop_undistort_jac)."""
    if ref2d.dtype != torch.float32 or tuple(ref2d.shape[:2]) != (B, V) or ref2d.shape[-1] != 2:
        raise RuntimeError("mvg_uncrop_undistort_jac: (B, V, Lq, 2) float32 expected")
    ref2d = ref2d.contiguous()
    Lq = ref2d.shape[2]
    ud = torch.empty_like(ref2d)
    jac = torch.empty((B, V, Lq, 2, 2), dtype=torch.float32, device=ref2d.device)
    _launch("mvg_uncrop_undistort_jac", ref2d, cams, ud, jac, V, B, Lq)
    return ud, jac


def _dlt_args(ud, conf, Pm, valid, J):
    B, V, Lq = conf.shape
    if (ud.dtype != torch.float32 or conf.dtype != torch.float32 or Pm.dtype != torch.float32 or valid.dtype != torch.uint8
            or tuple(ud.shape) != (B, V, Lq, 2) or tuple(Pm.shape) != (B, V, 3, 4) or Lq % J or valid.numel() != B * (Lq // J)):
        raise RuntimeError("mvg_dlt: ud (B,V,Lq,2) / conf (B,V,Lq) / Pm (B,V,3,4) float32 and valid (B,NQ) uint8 expected")
    return B, V, Lq


def dlt_forward(ud, conf, Pm, valid, J):
    """X (B, Lq, 3) of the dense differentiable triangulation (mvg_dlt_forward); zeros for the tokens of queries with valid == 0."""
    B, V, Lq = _dlt_args(ud, conf, Pm, valid, J)
    ud, conf, Pm, valid = ud.contiguous(), conf.contiguous(), Pm.contiguous(), valid.contiguous()
    X = torch.empty((B, Lq, 3), dtype=torch.float32, device=ud.device)
    _launch("mvg_dlt_forward", ud, conf, Pm, valid, X, V, B, Lq // J, J)
    return X


def dlt_backward(ud, conf, Pm, valid, J, gX):
    """(g_ud, g_conf) of dlt_forward for gX (B, Lq, 3) (mvg_dlt_backward)."""
    B, V, Lq = _dlt_args(ud, conf, Pm, valid, J)
    if gX.dtype != torch.float32 or tuple(gX.shape) != (B, Lq, 3):
        raise RuntimeError("mvg_dlt_backward: gX (B, Lq, 3) float32 expected")
    ud, conf, Pm, valid, gX = ud.contiguous(), conf.contiguous(), Pm.contiguous(), valid.contiguous(), gX.contiguous()
    g_ud = torch.empty_like(ud)
    g_conf = torch.empty_like(conf)
    _launch("mvg_dlt_backward", ud, conf, Pm, valid, gX, g_ud, g_conf, V, B, Lq // J, J)
    return g_ud, g_conf


def sym4_eigh(G):
    """eigen-decomposition of symmetric 4x4 matrices G (..., 4, 4) fp64 on the GPU: (evals (..., 4), evecs (..., 4, 4),
    eigenvectors as columns, no particular order)."""
    if G.dtype != torch.float64 or G.shape[-2:] != (4, 4):
        raise RuntimeError("mvg_sym4_eigh: (..., 4, 4) float64 expected")
    Gc = G.contiguous()
    n = Gc.numel() // 16
    w = torch.empty(Gc.shape[:-1], dtype=torch.float64, device=G.device)
    V = torch.empty_like(Gc)
    _launch("mvg_sym4_eigh", Gc, w, V, n)
    return w, V


# ---- training criterion (csrc/criterion.hip) ---------------------------------------------------------------------------------
MATCH_METHODS = {"KNN": _D["MVG_MATCH_KNN"], "multiple": _D["MVG_MATCH_MULTIPLE"]}
CRITERION_COLUMNS = ("loss_ce", "class_error", "class_recall", "class_precision", "cardinality_error", "loss_pose_perjoint",
                     "loss_pose_perprojection_2d", "keep_2d")


def _host3(x):
    return (C.c_float * 3)(*(float(v) for v in x))


def _count_tensor(num_person, B):
    if num_person.dtype not in (torch.int32, torch.int64) or num_person.numel() != B:
        raise RuntimeError("num_person: (B,) int32 / int64 tensor expected")
    return num_person.contiguous(), int(num_person.dtype == torch.int64)


def _joint_map_arg(joint_map, Jp, joints_3d, what):
    """joint_map (Jc distinct ints inside [0, Jp): converted joint j is prediction joint joint_map[j]) -> the host int array the
    *_jm entry points take, checked against the joint counts before the library sees it; None stays None (the identity)"""
    if joint_map is None:
        return None
    jm = [int(v) for v in joint_map]
    if Jp is None or Jp < 1 or Jp > 64:
        raise ValueError("%s: joint_map needs the joints per query of the predictions (1..64), got %r" % (what, Jp))
    if not jm or len(jm) > 64:
        raise ValueError("%s: joint_map must hold 1..64 entries, got %d" % (what, len(jm)))
    if len(set(jm)) != len(jm):
        raise ValueError("%s: joint_map repeats an entry: %r" % (what, jm))
    if min(jm) < 0 or max(jm) >= Jp:
        raise ValueError("%s: joint_map entries must lie in [0, %d): %r" % (what, Jp, jm))
    if joints_3d.dim() != 4 or joints_3d.shape[2] != len(jm):
        raise RuntimeError("%s: joints_3d %s does not have the %d joints of joint_map" % (what, tuple(joints_3d.shape), len(jm)))
    return (C.c_int * len(jm))(*jm)


def knn_match(poses, joints_3d, num_person, space_size, space_center, method="KNN", value=5, joint_map=None, num_joints=None):
    """poses (B, NQ*J, 3) abs mm, joints_3d (B, Gmax, J, 3) abs mm, num_person (B,) -> pair_query, pair_gt (B, Pmax) int32 (-1 in
    unused slots), pair_count (B,) int32, matched (B, NQ) uint8 (mvg_knn_match: one launch, nothing read back).  method 'KNN'
    (value = K, Pmax = Gmax*K) or 'multiple' (value = cost threshold, Pmax = NQ).
    joint_map (Shelf / Campus joint format, mvg_knn_match_jm): Jc distinct ints, converted joint j is prediction joint
    joint_map[j]; poses then are (B, NQ*Jp, 3) with Jp = num_joints (poses alone do not tell NQ from Jp) and joints_3d
    (B, Gmax, Jc, 3).  Still one launch; the map is a launch argument."""
    if method in ("hungarian", "hungarian-dis"):
        raise NotImplementedError("match method %r: knn_match does not solve the Hungarian assignment (ops.hungarian_match "
                                  "does)" % method)
    if method not in MATCH_METHODS:
        raise ValueError("unknown match method %r" % (method,))
    jm = _joint_map_arg(joint_map, num_joints, joints_3d, "mvg_knn_match_jm")
    L.require_cuda(poses, joints_3d, num_person)
    if poses.dtype != torch.float32 or joints_3d.dtype != torch.float32 or joints_3d.dim() != 4 or joints_3d.shape[-1] != 3 \
            or poses.dim() != 3 or poses.shape[-1] != 3 or poses.shape[0] != joints_3d.shape[0]:
        raise RuntimeError("mvg_knn_match: poses (B, NQ*J, 3) / joints_3d (B, Gmax, J, 3) float32 expected")
    B, Gmax, J = joints_3d.shape[:3]
    Jp = J if jm is None else int(num_joints)
    if poses.shape[1] % Jp:
        raise RuntimeError("mvg_knn_match: poses rows (%d) are not a multiple of J = %d" % (poses.shape[1], Jp))
    NQ = poses.shape[1] // Jp
    num_person, is64 = _count_tensor(num_person, B)
    poses, joints_3d = poses.detach().contiguous(), joints_3d.contiguous()
    knn = method == "KNN"
    K = int(value) if knn else 0
    Pmax = Gmax * max(K, 1) if knn else NQ
    lib = L.load()
    dev = poses.device
    pq = torch.empty((B, Pmax), dtype=torch.int32, device=dev)
    pg = torch.empty((B, Pmax), dtype=torch.int32, device=dev)
    pc = torch.empty((B,), dtype=torch.int32, device=dev)
    matched = torch.empty((B, NQ), dtype=torch.uint8, device=dev)
    nbytes = lib.mvg_knn_match_workspace(B, NQ, Gmax)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev) if nbytes else None
    head = (poses, joints_3d, num_person, is64, _host3(space_size), _host3(space_center), MATCH_METHODS[method], K, float(value))
    tail = (Pmax, ws, nbytes, pq, pg, pc, matched)
    if jm is None:
        _launch("mvg_knn_match", *head, B, NQ, Gmax, J, *tail, label="knn_match")
    else:
        _launch("mvg_knn_match_jm", *head, B, NQ, Gmax, Jp, J, jm, *tail, label="knn_match")
    return pq, pg, pc, matched


HUNGARIAN_METHODS = {"hungarian": _D["MVG_MATCH_HUNGARIAN"], "hungarian-dis": _D["MVG_MATCH_HUNGARIAN_DIS"]}
HUNGARIAN_MAX_G, HUNGARIAN_MAX_NQ = _D["MVG_HUNGARIAN_MAX_G"], _D["MVG_HUNGARIAN_MAX_NQ"]


def hungarian_match(poses, joints_3d, num_person, space_size, space_center, logits=None, method="hungarian", cost_class=1.0,
                    cost_pose=1.0, joint_map=None, num_joints=None, duals=False):
    """The reference's one-to-one matcher (methods 'hungarian' / 'hungarian-dis') on the device: mvg_hungarian_match, ONE launch
    for all problems, nothing read back, no scipy.  poses (B, NQ*J, 3) or (Lm, B, NQ*J, 3) abs mm -- Lm sets of predictions (the
    decoder layers) matched against the same ground truth in the same launch --, logits (B, NQ, 2) / (Lm, B, NQ, 2) or None
    (= logit 1 everywhere), joints_3d (B, Gmax, J, 3), num_person (B,).  C = cost_pose * pose + cost_class * class for
    'hungarian', C = pose for 'hungarian-dis' (logits ignored).
    -> pair_query, pair_gt (B, Gmax) int32: the num_person pairs in ascending query order, -1 behind them; pair_count (B,) int32;
    matched (B, NQ) uint8; with duals=True also the solver's potentials u (B, Gmax), v (B, NQ) fp64.  A leading Lm is kept.
    joint_map / num_joints as for knn_match.  The methods 'KNN' and 'multiple' are ops.knn_match; ops.knn_match keeps refusing
    the Hungarian names."""
    if method not in HUNGARIAN_METHODS:
        raise ValueError("unknown Hungarian match method %r (hungarian | hungarian-dis)" % (method,))
    jm = _joint_map_arg(joint_map, num_joints, joints_3d, "mvg_hungarian_match")
    L.require_cuda(poses, joints_3d, num_person, logits)
    lead = poses.dim() == 4
    if poses.dtype != torch.float32 or joints_3d.dtype != torch.float32 or joints_3d.dim() != 4 or joints_3d.shape[-1] != 3 \
            or poses.dim() not in (3, 4) or poses.shape[-1] != 3 or poses.shape[-3] != joints_3d.shape[0]:
        raise RuntimeError("mvg_hungarian_match: poses ([Lm,] B, NQ*J, 3) / joints_3d (B, Gmax, J, 3) float32 expected")
    B, Gmax, J = joints_3d.shape[:3]
    Lm = poses.shape[0] if lead else 1
    Jp = J if jm is None else int(num_joints)
    if poses.shape[-2] % Jp:
        raise RuntimeError("mvg_hungarian_match: poses rows (%d) are not a multiple of J = %d" % (poses.shape[-2], Jp))
    NQ = poses.shape[-2] // Jp
    if logits is not None and (logits.dtype != torch.float32 or tuple(logits.shape) != tuple(poses.shape[:-2]) + (NQ, 2)):
        raise RuntimeError("mvg_hungarian_match: logits %s float32 expected" % (tuple(poses.shape[:-2]) + (NQ, 2),))
    if Gmax > HUNGARIAN_MAX_G or NQ > HUNGARIAN_MAX_NQ or NQ < Gmax:
        raise RuntimeError("mvg_hungarian_match: Gmax <= %d, Gmax <= NQ <= %d expected, got Gmax = %d, NQ = %d"
                           % (HUNGARIAN_MAX_G, HUNGARIAN_MAX_NQ, Gmax, NQ))
    num_person, is64 = _count_tensor(num_person, B)
    poses, joints_3d = poses.detach().contiguous(), joints_3d.contiguous()
    logits = None if logits is None else logits.detach().contiguous()
    P = Lm * B
    lib = L.load()
    dev = poses.device
    head = (Lm, B) if lead else (B,)
    pq = torch.empty(head + (Gmax,), dtype=torch.int32, device=dev)
    pg = torch.empty(head + (Gmax,), dtype=torch.int32, device=dev)
    pc = torch.empty(head, dtype=torch.int32, device=dev)
    matched = torch.empty(head + (NQ,), dtype=torch.uint8, device=dev)
    uv = torch.empty(head + (Gmax + NQ,), dtype=torch.float64, device=dev) if duals else None
    nbytes = lib.mvg_hungarian_match_workspace(P, NQ, Gmax)
    ws = torch.empty(((nbytes + 3) // 4,), dtype=torch.float32, device=dev) if nbytes else None
    _launch("mvg_hungarian_match", logits, poses, joints_3d, num_person, is64, _host3(space_size), _host3(space_center),
            HUNGARIAN_METHODS[method], float(cost_class), float(cost_pose), P, B, NQ, Gmax, Jp, J, jm, ws, nbytes, pq, pg, pc, matched,
            uv, label="hungarian_match")
    if duals:
        return pq, pg, pc, matched, uv[..., :Gmax], uv[..., Gmax:]
    return pq, pg, pc, matched


def criterion(logits, poses, poses_2d, pair_query, pair_gt, pair_count, joints_3d, joints_3d_vis, joints_vis, num_person, cams,
              space_size, space_center, pred_conf_threshold, num_samples=None, focal_alpha=0.25, focal_gamma=2.0, joint_map=None):
    """All layers' losses, metrics and gradients in three launches (mvg_criterion).  logits (L,B,NQ,2), poses (L,B,NQ*J,3),
    poses_2d (L,B,V,NQ*J,2) fp32; the pair list of knn_match; joints_3d / joints_3d_vis (B,Gmax,J,3), joints_vis (V,B,Gmax,J,2)
    fp32; cams = pack_cameras(...).  -> table (L, 8) fp32 in the order of CRITERION_COLUMNS, grad_logits, grad_poses,
    grad_poses_2d (shaped like the inputs; the 2D gradient is the unguarded one, to be multiplied by keep_2d).
    joint_map (Shelf / Campus joint format, mvg_criterion_jm): Jc distinct ints, converted joint j is prediction joint
    joint_map[j]; poses / poses_2d keep their Jp joints per query, the ground truth has Jc.  The losses are those of the
    gathered predictions, the gradients come back in the Jp shape (zeros at joints the map does not name).  Still three launches."""
    Jp = None
    if joint_map is not None and logits.dim() == 4 and poses.dim() == 4 and logits.shape[2] and poses.shape[2] % logits.shape[2] == 0:
        Jp = poses.shape[2] // logits.shape[2]
    jm = _joint_map_arg(joint_map, Jp, joints_3d, "mvg_criterion_jm")
    tensors = (logits, poses, poses_2d, pair_query, pair_gt, pair_count, joints_3d, joints_3d_vis, joints_vis, num_person, cams)
    L.require_cuda(*tensors, num_samples)
    if any(t.dtype != torch.float32 for t in (logits, poses, poses_2d, joints_3d, joints_3d_vis, joints_vis, cams)):
        raise RuntimeError("mvg_criterion: float32 tensors expected")
    if any(t.dtype != torch.int32 for t in (pair_query, pair_gt, pair_count)):
        raise RuntimeError("mvg_criterion: int32 pair list expected")
    if logits.dim() != 4 or logits.shape[-1] != 2 or poses.dim() != 4 or poses_2d.dim() != 5 or joints_3d.dim() != 4:
        raise RuntimeError("mvg_criterion: logits (L,B,NQ,2) / poses (L,B,NQ*J,3) / poses_2d (L,B,V,NQ*J,2) expected")
    Ln, B, NQ = logits.shape[:3]
    Gmax, J = joints_3d.shape[1:3]
    V = poses_2d.shape[2]
    Pmax = pair_query.shape[-1]
    Jp = J if jm is None else Jp
    if (tuple(poses.shape) != (Ln, B, NQ * Jp, 3) or tuple(poses_2d.shape) != (Ln, B, V, NQ * Jp, 2)
            or tuple(joints_3d.shape) != (B, Gmax, J, 3) or tuple(joints_3d_vis.shape) != (B, Gmax, J, 3)
            or tuple(joints_vis.shape) != (V, B, Gmax, J, 2) or tuple(pair_query.shape) != (B, Pmax)
            or tuple(pair_gt.shape) != (B, Pmax) or pair_count.numel() != B or tuple(cams.shape) != (V * B, L.CAM_STRIDE)):
        raise RuntimeError("mvg_criterion: inconsistent shapes")
    if num_samples is not None and (num_samples.dtype != torch.float32 or num_samples.numel() != 1):
        raise RuntimeError("mvg_criterion: num_samples must be a float32 device scalar")
    num_person, is64 = _count_tensor(num_person, B)
    logits, poses, poses_2d = logits.detach().contiguous(), poses.detach().contiguous(), poses_2d.detach().contiguous()
    pair_query, pair_gt, pair_count = pair_query.contiguous(), pair_gt.contiguous(), pair_count.contiguous()
    joints_3d, joints_3d_vis, joints_vis, cams = (t.contiguous() for t in (joints_3d, joints_3d_vis, joints_vis, cams))
    lib = L.load()
    dev = logits.device
    nbytes = lib.mvg_criterion_workspace(Ln, B, Gmax, V, J)
    ws = torch.empty(((nbytes + 7) // 8,), dtype=torch.float64, device=dev)
    table = torch.empty((Ln, len(CRITERION_COLUMNS)), dtype=torch.float32, device=dev)
    gl, gp, gp2 = torch.empty_like(logits), torch.empty_like(poses), torch.empty_like(poses_2d)
    head = (logits, poses, poses_2d, pair_query, pair_gt, pair_count, joints_3d, joints_3d_vis, joints_vis, num_person, is64,
            num_samples, cams, _host3(space_size), _host3(space_center), float(pred_conf_threshold), float(focal_alpha),
            float(focal_gamma))
    tail = (V, Gmax, Pmax, ws, nbytes, table, gl, gp, gp2)
    if jm is None:
        _launch("mvg_criterion", *head, Ln, B, NQ, J, *tail, label="criterion")
    else:
        _launch("mvg_criterion_jm", *head, Ln, B, NQ, Jp, J, jm, *tail, label="criterion")
    return table, gl, gp, gp2


# ---- optimizer step (csrc/optim.hip) -----------------------------------------------------------------------------------------
OPTIM_CHUNK = _D["MVG_OPTIM_CHUNK"]
OPTIM_TENSOR_WORDS, OPTIM_GROUP_WORDS = _D["MVG_OPTIM_TENSOR_WORDS"], _D["MVG_OPTIM_GROUP_WORDS"]
OPTIM_STATE_HEADER, OPTIM_STATE_PER_GROUP = _D["MVG_OPTIM_STATE_HEADER"], _D["MVG_OPTIM_STATE_PER_GROUP"]


def optim_state_words(n_groups):
    """int64 words of the state block of optim_step for n_groups hyper-parameter groups"""
    return (OPTIM_STATE_HEADER + n_groups * OPTIM_STATE_PER_GROUP) // 8


def optim_step(tensor_table, chunk_table, group_table, state, workspace, loss=None, max_norm=0.0, zero_grad=False, norm_out=None):
    """clip_grad_norm_ + Adam / AdamW over every tensor of the tables in at most three launches (mvg_optim_step; the table layouts
    are in include/mvg_decoder.h).  tensor_table (n_tensors, 6) int64, chunk_table (n_chunks, 2) int32, group_table (n_groups, 6)
    float64, state (>= optim_state_words(n_groups),) int64, workspace (>= max(n_chunks, 1),) float64; loss / norm_out: float32
    device scalars or None.  Updates the tensors the tables point to in place; nothing is read back."""
    L.require_cuda(tensor_table, chunk_table, group_table, state, workspace, loss, norm_out)
    if (tensor_table.dtype != torch.int64 or tensor_table.dim() != 2 or tensor_table.shape[1] != OPTIM_TENSOR_WORDS
            or chunk_table.dtype != torch.int32 or chunk_table.dim() != 2 or chunk_table.shape[1] != 2
            or group_table.dtype != torch.float64 or group_table.dim() != 2 or group_table.shape[1] != OPTIM_GROUP_WORDS
            or state.dtype != torch.int64 or workspace.dtype != torch.float64
            or not all(t.is_contiguous() for t in (tensor_table, chunk_table, group_table, state, workspace))):
        raise RuntimeError("mvg_optim_step: tables (n, 6) int64 / (n, 2) int32 / (n, 6) float64, state int64, workspace float64, "
                           "all contiguous, expected")
    for s in (loss, norm_out):
        if s is not None and (s.dtype != torch.float32 or s.numel() != 1):
            raise RuntimeError("mvg_optim_step: loss / norm_out must be float32 device scalars")
    _launch("mvg_optim_step", tensor_table, tensor_table.shape[0], chunk_table, chunk_table.shape[0], group_table,
            group_table.shape[0], state, state.numel() * 8, workspace, workspace.numel() * 8, loss, float(max_norm),
            int(bool(zero_grad)), norm_out, label="optim_step")


# ---- derived bf16 operands of the bf16 training path (csrc/operands.hip) ---------------------------------------------------------
OPERANDS_TILE, OPERANDS_RECORD_WORDS = _D["MVG_OPERANDS_TILE"], _D["MVG_OPERANDS_RECORD_WORDS"]


def refresh_operands(record_table, tile_table):
    """bf16 copy and / or transposed bf16 copy of every fp32 matrix of the tables in one launch on the current stream
    (mvg_refresh_operands; the table layouts are in include/mvg_decoder.h): record_table (n_records, 8) int64, tile_table
    (n_tiles, 2) int32, both on the device.  Writes the destinations the records point to; nothing is read back."""
    L.require_cuda(record_table, tile_table)
    if (record_table.dtype != torch.int64 or record_table.dim() != 2 or record_table.shape[1] != OPERANDS_RECORD_WORDS
            or tile_table.dtype != torch.int32 or tile_table.dim() != 2 or tile_table.shape[1] != 2
            or not record_table.is_contiguous() or not tile_table.is_contiguous()):
        raise RuntimeError("mvg_refresh_operands: tables (n, 8) int64 / (n, 2) int32, contiguous, expected")
    _launch("mvg_refresh_operands", record_table, record_table.shape[0], tile_table, tile_table.shape[0], label="refresh_operands")


# ---- serving: caller-owned static buffers and the checks their wrappers share ---------------------------------------------------
class _Layout:
    """One family of caller-owned static buffers, written once: entries (key, dtype, shape, fill), the shape in named dimensions
    and plain ints (("B", "T", "J", 3)), fill None for memory that is left uninitialised.  ``maker`` is the *_buffers function
    that messages point to."""

    def __init__(self, maker, *entries):
        self.maker, self.entries, self.keys = maker, entries, tuple(e[0] for e in entries)

    def alloc(self, dims, device):
        out = {}
        for key, dtype, shape, fill in self.entries:
            shape = tuple(dims[d] if isinstance(d, str) else d for d in shape)
            out[key] = (torch.empty(shape, dtype=dtype, device=device) if fill is None
                        else torch.full(shape, fill, dtype=dtype, device=device))
        return out

    def check(self, buffers, dims, keys=None, who=None):
        """raises unless the tensors ``keys`` (default: all) of ``buffers`` have the family's dtype, its shape for ``dims`` and are
        contiguous"""
        for key, dtype, shape, _ in self.entries:
            if keys is not None and key not in keys:
                continue
            shape = tuple(dims[d] if isinstance(d, str) else d for d in shape)
            t = buffers[key]
            if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
                raise RuntimeError("%s: buffer %r must be a contiguous %s tensor of shape %s, got %s %s with strides %s (see %s)"
                                   % (who or self.maker, key, dtype, shape, t.dtype, tuple(t.shape), t.stride(), self.maker))


def _check_limits(who, *terms):
    """terms (name, value, largest value): raises unless 1 <= value <= largest for each"""
    if not all(1 <= v <= hi for _, v, hi in terms):
        raise L.MvgError("%s: unsupported shape %s" % (who, ", ".join("%s = %d (<= %d)" % t for t in terms)))


def _check_dets(who, dets, count):
    """dets (B, R, J, 5) fp32 and count (B, 2) int32 or None, as pose_nms leaves them -> (B, R, J)"""
    if dets.dim() != 4 or dets.shape[-1] != 5 or dets.dtype != torch.float32:
        raise RuntimeError("%s: dets (B, R, J, 5) float32 expected" % who)
    B, R, J = dets.shape[:3]
    if count is not None and (count.dtype != torch.int32 or tuple(count.shape) != (B, 2)):
        raise RuntimeError("%s: count (B, 2) int32 or None expected" % who)
    return B, R, J


def _check_ground_truth(who, joints_3d, joints_3d_vis, num_person, B, J):
    """joints_3d (B, G, J, 3) fp32, joints_3d_vis (B, G, J) fp32 and num_person (B) int32, as the evaluators take them -> G"""
    if joints_3d.dim() != 4 or joints_3d.dtype != torch.float32 or joints_3d.shape[0] != B or tuple(joints_3d.shape[2:]) != (J, 3):
        raise RuntimeError("%s: joints_3d (B, G, J, 3) float32 expected" % who)
    G = joints_3d.shape[1]
    if joints_3d_vis.dtype != torch.float32 or tuple(joints_3d_vis.shape) != (B, G, J):
        raise RuntimeError("%s: joints_3d_vis (B, G, J) float32 expected" % who)
    if num_person.dtype != torch.int32 or tuple(num_person.shape) != (B,):
        raise RuntimeError("%s: num_person (B) int32 expected" % who)
    return G


NMS_MAX_N, NMS_MAX_J = _D["MVG_NMS_MAX_N"], _D["MVG_NMS_MAX_J"]
_NMS = _Layout("pose_nms_buffers", ("keep", torch.int32, ("B", "N"), None), ("count", torch.int32, ("B", 2), None),
               ("dets", torch.float32, ("B", "rows", "J", 5), None), ("workspace", torch.uint8, ("nbytes",), None))


def pose_nms_buffers(B, N, J, dets_rows=None, device="cuda"):
    """the static buffers of pose_nms(out=...): keep (B, N) int32, count (B, 2) int32, dets (B, dets_rows, J, 5) fp32 and the
    workspace.  A caller that captures pose_nms in a HIP graph allocates them once and keeps them alive with the graph."""
    rows = N if dets_rows is None else int(dets_rows)
    nbytes = L.load().mvg_pose_nms_workspace(B, N, J)
    if nbytes == 0 or rows < 1:
        raise L.MvgError("mvg_pose_nms: unsupported shape B = %d, N = %d (<= %d), J = %d (<= %d), dets_rows = %d"
                         % (B, N, NMS_MAX_N, J, NMS_MAX_J, rows))
    return _NMS.alloc(dict(B=B, N=N, J=J, rows=rows, nbytes=nbytes), device)


def pose_nms(pred, dist_thr=0.3, num_nearby_joints_thr=7, max_dets=-1, dets_rows=None, out=None):
    """Classification filter + nearby-joints NMS on the device (mvg_pose_nms: three launches, nothing read back, no
    synchronisation; validate_3d.py:228-234, lib/core/nms.py:210-283).  pred (B, N, J, 5) fp32 contiguous, rows
    [x, y, z, flag, score] as written by caller.pack_predictions; row n is a candidate iff pred[b, n, 0, 3] >= 0.
    -> keep (B, N) int32: kept row indices in keep order, -1 behind the count; count (B, 2) int32: [kept, candidates skipped for an
    empty neighbourhood]; dets (B, dets_rows, J, 5): the kept rows in keep order, rows behind the count are 0 with flag -1.
    The arithmetic is numpy's fp64 (the closeness matrix is the reference's bit for bit).  Candidates are visited in descending
    score and, among equal scores, the higher row first (np.argsort(scores, kind="stable")[::-1]); the reference's unstable
    default argsort leaves the order among tied scores unspecified and coincides with this rule for N <= 16.  A candidate whose
    own neighbourhood is empty (zero extent, NaN coordinate) is counted in count[:, 1] and otherwise ignored, where the reference
    raises.  num_nearby_joints_thr None = J // 2.  out: the dict of pose_nms_buffers (static buffers for graph capture); None
    allocates per call."""
    if not dist_thr > 0:
        raise AssertionError("`dist_thr` must be greater than 0.")                   # nms.py:233
    if pred.dim() != 4 or pred.shape[-1] != 5 or pred.dtype != torch.float32:
        raise RuntimeError("mvg_pose_nms: pred (B, N, J, 5) float32 expected")
    B, N, J = pred.shape[:3]
    if num_nearby_joints_thr is None:
        num_nearby_joints_thr = J // 2
    if not num_nearby_joints_thr < J:
        raise AssertionError("`num_nearby_joints_thr` must be less than the number of joints.")
    L.require_cuda(pred)
    if not pred.is_contiguous():
        raise RuntimeError("mvg_pose_nms: pred must be contiguous")
    if out is None:
        out = pose_nms_buffers(B, N, J, dets_rows, pred.device)
    keep, count, dets, ws = out["keep"], out["count"], out["dets"], out["workspace"]
    L.require_cuda(keep, count, dets, ws)
    rows = dets_rows if dets_rows is not None else dets.shape[1] if dets.dim() == 4 else 0      # any number of rows, or dets_rows
    _NMS.check(out, dict(B=B, N=N, J=J, rows=rows, nbytes=ws.numel()), who="mvg_pose_nms")
    _launch("mvg_pose_nms", pred, B, N, J, float(dist_thr), int(num_nearby_joints_thr), int(max_dets), ws, ws.numel(), keep, count,
            dets, dets.shape[1], label="pose_nms")
    return keep, count, dets


EVAL_MAX_R, EVAL_MAX_J, EVAL_MAX_G, EVAL_MAX_B = (_D["MVG_EVAL_MAX_" + k] for k in "RJGB")
EVAL_STATE = ("n_entries", "total_gt", "frames", "overflow", "kept_rows", "match_gt", "empty_frame", "reserved")
_EVAL = _Layout("eval_buffers", ("mpjpe", torch.float64, ("capacity",), 0), ("score", torch.float64, ("capacity",), 0),
                ("gt_id", torch.int64, ("capacity",), 0), ("correct", torch.int64, ("actors",), 0),
                ("total", torch.int64, ("actors",), 0), ("bone_correct", torch.int64, ("actors", 10), 0),
                ("state", torch.int64, (len(EVAL_STATE),), 0))


def eval_buffers(capacity, actors=4, device="cuda"):
    """the zeroed accumulators of eval_match / eval_pcp: the entry list mpjpe / score (capacity) fp64 and gt_id (capacity) int64,
    the PCP counters correct / total (actors) and bone_correct (actors, 10) int64, and the int64 state block (EVAL_STATE).
    Allocated once and kept alive by the caller: a captured HIP graph addresses them by pointer, like pose_nms_buffers."""
    capacity, actors = int(capacity), int(actors)
    if capacity < 1 or not 1 <= actors <= EVAL_MAX_G:
        raise L.MvgError("eval_buffers: capacity >= 1 and 1 <= actors <= %d expected (got %d, %d)" % (EVAL_MAX_G, capacity, actors))
    return _EVAL.alloc(dict(capacity=capacity, actors=actors), device)


def _eval_inputs(name, dets, count, joints_3d, joints_3d_vis, num_person, buffers, keys, dims):
    """the checks eval_match and eval_pcp share -> (B, R, J, G)"""
    L.require_cuda(dets, count, joints_3d, joints_3d_vis, num_person, *(buffers[k] for k in keys))
    B, R, J = _check_dets(name, dets, count)
    G = _check_ground_truth(name, joints_3d, joints_3d_vis, num_person, B, J)
    if not all(t is None or t.is_contiguous() for t in (dets, count, joints_3d, joints_3d_vis, num_person)):
        raise RuntimeError("%s: every tensor must be contiguous" % name)
    _EVAL.check(buffers, dims, keys, who=name)
    return B, R, J, G


def eval_match(dets, count, joints_3d, joints_3d_vis, num_person, buffers):
    """Panoptic ground-truth matching on the device (mvg_eval_match: two launches, nothing read back, no synchronisation;
    panoptic.py:497-556 as evaluate.match_predictions restates it for score_sort).  dets (B, R, J, 5) fp32 and count (B, 2) int32
    or None as pose_nms leaves them; joints_3d (B, Gmax, J, 3) fp32, joints_3d_vis (B, Gmax, J) fp32 (visible when > 0),
    num_person (B) int32.  Appends (mpjpe, score, gt_id) of every participating row to ``buffers`` (eval_buffers) in the
    reference's order and advances the state block; entries past the capacity are counted, not written."""
    keys = ("mpjpe", "score", "gt_id", "state")
    capacity = buffers["mpjpe"].numel()      # the entry list is as long as the caller made it
    B, R, J, G = _eval_inputs("mvg_eval_match", dets, count, joints_3d, joints_3d_vis, num_person, buffers, keys,
                              dict(capacity=capacity))
    mp, sc, gid, state = (buffers[k] for k in keys)
    _launch("mvg_eval_match", dets, count, joints_3d, joints_3d_vis, num_person, B, R, J, G, mp, sc, gid, capacity, state,
            label="eval_match")


def eval_pcp(dets, count, joints_3d, joints_3d_vis, num_person, buffers, recall_threshold=500.0, alpha=0.5):
    """PCP counters of Shelf.evaluate / Campus.evaluate on the device (mvg_eval_pcp: one launch, nothing read back; shelf.py:255-330
    as evaluate.evaluate_pcp restates it).  Inputs as eval_match, in the 14-joint format; actor slot a of element b is annotated
    when some joints_3d_vis[b, a] != 0.  Adds to correct / total / bone_correct and the state block of ``buffers``."""
    keys = ("correct", "total", "bone_correct", "state")
    A = buffers["correct"].numel()           # as many actors as the caller's counters have
    B, R, J, G = _eval_inputs("mvg_eval_pcp", dets, count, joints_3d, joints_3d_vis, num_person, buffers, keys, dict(actors=A))
    correct, total, bones, state = (buffers[k] for k in keys)
    _launch("mvg_eval_pcp", dets, count, joints_3d, joints_3d_vis, num_person, B, R, J, G, A, float(recall_threshold), float(alpha),
            correct, total, bones, state, label="eval_pcp")


LAP_MAX_N, LAP_BIG = _D["MVG_LAP_MAX_N"], _D["MVG_LAP_BIG"]
TRACK_MAX_D, TRACK_MAX_T, TRACK_MAX_J, TRACK_MAX_R, TRACK_MAX_B = (_D["MVG_TRACK_MAX_" + k] for k in "DTJRB")
TRACK_STATE = ("frames", "matches", "births", "deaths", "overflow", "dropped", "active", "reserved")
_TRACK = _Layout("track_buffers", ("id", torch.int32, ("B", "T"), -1), ("hits", torch.int32, ("B", "T"), 0),
                 ("misses", torch.int32, ("B", "T"), 0), ("born", torch.int64, ("B", "T"), 0), ("score", torch.float32, ("B", "T"), 0),
                 ("pose", torch.float32, ("B", "T", "J", 3), 0), ("next_id", torch.int32, ("B",), 0),
                 ("state", torch.int64, (len(TRACK_STATE),), 0), ("ids", torch.int32, ("B", "R"), -1),
                 ("slots", torch.int32, ("B", "R"), -1))
_TRACK_MOTION = _Layout("track_motion_buffers", ("mean", torch.float64, ("B", "T", "J", 2, 3), 0),
                        ("var", torch.float64, ("B", "T", 3), 0), ("row_pose", torch.float32, ("B", "R", "J", 3), 0))


def _check_track_limits(who, B, T, J, R):
    _check_limits(who, ("B", B, TRACK_MAX_B), ("T", T, TRACK_MAX_T), ("J", J, TRACK_MAX_J), ("R", R, TRACK_MAX_R))


def linear_assignment(cost, n=None, m=None):
    """Minimum-cost assignment on the device (mvg_linear_assignment: one launch, one wavefront per problem, nothing read back).
    cost (B, N, M) fp64 contiguous with N, M <= LAP_MAX_N; n, m (B) int32 live sizes or None (= N, M): the problem of element b is
    cost[b, :n[b], :m[b]], padded with zeros to a square.  An entry that is NaN or above LAP_BIG counts as LAP_BIG.
    -> col_of_row (B, N) int32 (-1: dead row, or a row left unassigned because n > m) and total (B) fp64, the assigned entries of
    the input added in row order.  Shortest augmenting paths with potentials, rows in order, lowest column among equal minima:
    the rule of include/mvg_decoder.h, which a host restatement reproduces bit for bit."""
    L.require_cuda(cost, n, m)
    if cost.dim() != 3 or cost.dtype != torch.float64:
        raise RuntimeError("mvg_linear_assignment: cost (B, N, M) float64 expected")
    B, N, M = cost.shape
    for name, t in (("n", n), ("m", m)):
        if t is not None and (t.dtype != torch.int32 or tuple(t.shape) != (B,)):
            raise RuntimeError("mvg_linear_assignment: %s (B) int32 or None expected" % name)
    if not all(t is None or t.is_contiguous() for t in (cost, n, m)):
        raise RuntimeError("mvg_linear_assignment: every tensor must be contiguous")
    if not (1 <= B <= TRACK_MAX_B and 1 <= N <= LAP_MAX_N and 1 <= M <= LAP_MAX_N):
        raise L.MvgError("mvg_linear_assignment: unsupported shape B = %d (<= %d), N = %d, M = %d (<= %d)"
                         % (B, TRACK_MAX_B, N, M, LAP_MAX_N))
    col = torch.empty((B, N), dtype=torch.int32, device=cost.device)
    total = torch.empty((B,), dtype=torch.float64, device=cost.device)
    _launch("mvg_linear_assignment", cost, n, m, B, N, M, col, total, label="linear_assignment")
    return col, total


def track_buffers(B, T, J, R, device="cuda"):
    """the state of track_update for B streams of T slots and J joints -- id (B, T) int32 filled with -1 (free), hits, misses
    (B, T) int32, born (B, T) int64, score (B, T) fp32, pose (B, T, J, 3) fp32, next_id (B) int32 and the int64 state block
    (TRACK_STATE) -- plus the static outputs ids, slots (B, R) int32 (-1).  Allocated once and kept alive by the caller: a captured
    HIP graph addresses them by pointer, like pose_nms_buffers."""
    B, T, J, R = int(B), int(T), int(J), int(R)
    _check_track_limits("track_buffers", B, T, J, R)
    return _TRACK.alloc(dict(B=B, T=T, J=J, R=R), device)


def track_update(dets, count, buffers, max_dist=500.0, max_misses=10, min_hits=1):
    """One frame of the pose tracker on the device (mvg_track_update: one launch, nothing read back, no synchronisation).  dets
    (B, R, J, 5) fp32 and count (B, 2) int32 or None as pose_nms leaves them; ``buffers`` from track_buffers.  The detections (row
    order, the first TRACK_MAX_D) are assigned to the live tracks at the minimum total mean joint distance, a pair further apart
    than max_dist (the unit of the poses) costing max_dist like a non-match; matched tracks take the detection, the others age and
    are freed after more than max_misses misses, unmatched detections open tracks in the lowest free slots.  -> (ids, slots), the
    (B, R) int32 tensors of ``buffers``: per row the track's id (once it has min_hits hits) and slot, else -1."""
    tensors = [buffers[k] for k in _TRACK.keys]
    L.require_cuda(dets, count, *tensors)
    B, R, J = _check_dets("mvg_track_update", dets, count)
    if not all(t is None or t.is_contiguous() for t in (dets, count)):
        raise RuntimeError("mvg_track_update: every tensor must be contiguous")
    ident = buffers["id"]
    T = ident.shape[1] if ident.dim() == 2 else 0         # as many slots as the caller's state has
    _TRACK.check(buffers, dict(B=B, T=T, J=J, R=R), who="mvg_track_update")
    _check_track_limits("mvg_track_update", B, T, J, R)
    if not (0.0 <= float(max_dist) <= LAP_BIG) or int(max_misses) < 0 or int(min_hits) < 0:
        raise L.MvgError("mvg_track_update: 0 <= max_dist <= %g, max_misses >= 0 and min_hits >= 0 expected (got %r, %r, %r)"
                         % (LAP_BIG, max_dist, max_misses, min_hits))
    state = (buffers[k] for k in ("id", "hits", "misses", "born", "score", "pose", "next_id", "state"))
    _launch("mvg_track_update", dets, count, B, R, J, T, *state, float(max_dist), int(max_misses), int(min_hits), buffers["ids"],
            buffers["slots"], label="track_update")
    return buffers["ids"], buffers["slots"]


def track_motion_buffers(B, T, J, R, device="cuda"):
    """the state of the tracker's motion model next to track_buffers(B, T, J, R) -- mean (B, T, J, 2, 3) fp64 (position and velocity
    xyz per joint), var (B, T, 3) fp64 (pxx, pxv, pvv: one covariance per track) -- plus the static output row_pose (B, R, J, 3)
    fp32, the filtered pose of every row.  All zeros; allocated once and kept alive by the caller like track_buffers."""
    B, T, J, R = int(B), int(T), int(J), int(R)
    _check_track_limits("track_motion_buffers", B, T, J, R)
    return _TRACK_MOTION.alloc(dict(B=B, T=T, J=J, R=R), device)


def _track_motion_inputs(name, buffers, motion, keys):
    """the checks track_predict and track_correct share -> (B, T, J, R)"""
    L.require_cuda(*(buffers[k] for k in keys), *(motion[k] for k in _TRACK_MOTION.keys))
    pose = buffers["pose"]
    if pose.dim() != 4 or pose.shape[-1] != 3:
        raise RuntimeError("%s: buffers are not those of track_buffers" % name)
    B, T, J = pose.shape[:3]
    R = buffers["slots"].shape[1] if buffers["slots"].dim() == 2 else 0
    dims = dict(B=B, T=T, J=J, R=R)
    _TRACK.check(buffers, dims, keys, who=name)
    _TRACK_MOTION.check(motion, dims, who=name)
    _check_track_limits(name, B, T, J, R)
    return B, T, J, R


def track_predict(buffers, motion, dt=1.0, q=25.0):
    """The motion model's step BEFORE track_update (mvg_track_predict: one launch, nothing read back): every live slot of
    ``buffers`` (track_buffers) moves one step of dt ahead at its velocity in ``motion`` (track_motion_buffers), its covariance
    grows by the process noise q (the variance of a random acceleration), and ``buffers["pose"]`` becomes the predicted pose the
    update associates against.  Free slots are not touched."""
    B, T, J, _ = _track_motion_inputs("mvg_track_predict", buffers, motion, ("id", "pose"))
    dt, q = float(dt), float(q)
    if not (0.0 < dt < float("inf")) or not (0.0 <= q <= LAP_BIG):
        raise L.MvgError("mvg_track_predict: finite dt > 0 and 0 <= q <= %g expected (got %r, %r)" % (LAP_BIG, dt, q))
    _launch("mvg_track_predict", B, T, J, buffers["id"], buffers["pose"], motion["mean"], motion["var"], dt, q, label="track_predict")


def track_correct(buffers, motion, r=400.0, v0=2500.0):
    """The motion model's step AFTER track_update (mvg_track_correct: one launch, nothing read back), every slot by the state the
    update left: a matched track's mean moves towards the detection by the Kalman gain of its covariance and measurement noise r
    and ``buffers["pose"]`` becomes the filtered pose; a track born in this update starts at the detection with zero velocity and
    the covariance (r, 0, v0); a missed track keeps its prediction; a free slot's motion state is zeroed.  Then
    ``motion["row_pose"]`` (B, R, J, 3) gets the pose of every row's slot (``buffers["slots"]``), zeros for rows without one."""
    B, T, J, R = _track_motion_inputs("mvg_track_correct", buffers, motion, ("id", "hits", "misses", "slots", "pose"))
    r, v0 = float(r), float(v0)
    if not (0.0 < r <= LAP_BIG) or not (0.0 <= v0 <= LAP_BIG):
        raise L.MvgError("mvg_track_correct: 0 < r <= %g and 0 <= v0 <= %g expected (got %r, %r)" % (LAP_BIG, LAP_BIG, r, v0))
    _launch("mvg_track_correct", B, R, T, J, *(buffers[k] for k in ("id", "hits", "misses", "slots", "pose")), motion["mean"],
            motion["var"], r, v0, motion["row_pose"], label="track_correct")
    return motion["row_pose"]


TRACK_EVAL_MAX_P, TRACK_EVAL_MAX_K = _D["MVG_TRACK_EVAL_MAX_P"], _D["MVG_TRACK_EVAL_MAX_K"]
TRACK_EVAL_STATE = ("frames", "gt", "hyp", "matches", "misses", "false_pos", "switches", "kept", "dropped", "unreported", "bad_id",
                    "id_overflow", "reserved")      # MVG_TRACK_EVAL_WORDS
_TRACK_EVAL = _Layout("track_eval_buffers", ("last_track", torch.int32, ("B", "P"), -1),
                      ("counters", torch.int64, ("B", len(TRACK_EVAL_STATE)), 0), ("dist_sum", torch.float64, ("B",), 0),
                      ("seen", torch.int64, ("B", "P"), 0), ("covered", torch.int64, ("B", "P"), 0),
                      ("overlap", torch.int32, ("B", "P", "K"), 0))


def track_eval_buffers(B, P, K, device="cuda"):
    """the state of track_eval for B streams of P identities and K track ids -- last_track (B, P) int32 filled with -1, counters
    (B, len(TRACK_EVAL_STATE)) int64, dist_sum (B) fp64, seen, covered (B, P) int64, overlap (B, P, K) int32, zeros.  Allocated
    once and kept alive by the caller, like track_buffers."""
    B, P, K = int(B), int(P), int(K)
    _check_limits("track_eval_buffers", ("B", B, TRACK_MAX_B), ("P", P, TRACK_EVAL_MAX_P), ("K", K, TRACK_EVAL_MAX_K))
    return _TRACK_EVAL.alloc(dict(B=B, P=P, K=K), device)


def track_eval(dets, count, ids, joints_3d, joints_3d_vis, num_person, buffers, dist_thr=500.0, row_pose=None, person_id=None):
    """One frame of CLEAR-MOT / identity scoring on the device (mvg_track_eval: one launch behind track_update, nothing read back,
    no atomics).  dets (B, R, J, 5) fp32, count (B, 2) int32 or None and ids (B, R) int32 as pose_nms and track_update leave them;
    row_pose (B, R, J, 3) fp32 or None: the motion model's filtered poses, scored instead of dets; joints_3d (B, G, J, 3),
    joints_3d_vis (B, G, J) fp32, num_person (B) int32 as the evaluator takes them (num_person < 0: the frame has no annotation
    and is skipped); person_id (B, G) int32 or None (person slot g is identity g); ``buffers`` from track_eval_buffers.  The rows
    with an id are matched to the persons by the CLEAR-MOT rules of include/mvg_decoder.h (last frame's pairs first while within
    dist_thr, the rest by minimum-cost assignment) and misses, false positives, identity switches, the matched distance and the
    person x track id overlap table are accumulated.  -> buffers."""
    name = "mvg_track_eval"
    keys = ("last_track", "counters", "dist_sum", "seen", "covered", "overlap")
    tensors = [buffers[k] for k in keys]
    L.require_cuda(dets, count, ids, row_pose, joints_3d, joints_3d_vis, num_person, person_id, *tensors)
    B, R, J = _check_dets(name, dets, count)
    if ids.dtype != torch.int32 or tuple(ids.shape) != (B, R):
        raise RuntimeError("mvg_track_eval: ids (B, R) int32 expected")
    if row_pose is not None and (row_pose.dtype != torch.float32 or tuple(row_pose.shape) != (B, R, J, 3)):
        raise RuntimeError("mvg_track_eval: row_pose (B, R, J, 3) float32 or None expected")
    G = _check_ground_truth(name, joints_3d, joints_3d_vis, num_person, B, J)
    if person_id is not None and (person_id.dtype != torch.int32 or tuple(person_id.shape) != (B, G)):
        raise RuntimeError("mvg_track_eval: person_id (B, G) int32 or None expected")
    if not all(t is None or t.is_contiguous() for t in (dets, count, ids, row_pose, joints_3d, joints_3d_vis, num_person, person_id)):
        raise RuntimeError("mvg_track_eval: every tensor must be contiguous")
    overlap = buffers["overlap"]
    P, K = (overlap.shape[1], overlap.shape[2]) if overlap.dim() == 3 else (0, 0)      # as the caller's tables have them
    _TRACK_EVAL.check(buffers, dict(B=B, P=P, K=K), who=name)
    if not (1 <= B <= TRACK_MAX_B and 1 <= R <= TRACK_MAX_R and 1 <= J <= TRACK_MAX_J and 1 <= G <= P <= TRACK_EVAL_MAX_P
            and 1 <= K <= TRACK_EVAL_MAX_K):
        raise L.MvgError("mvg_track_eval: unsupported shape B = %d (<= %d), R = %d (<= %d), J = %d (<= %d), G = %d <= P = %d (<= %d), "
                         "K = %d (<= %d)" % (B, TRACK_MAX_B, R, TRACK_MAX_R, J, TRACK_MAX_J, G, P, TRACK_EVAL_MAX_P, K,
                                             TRACK_EVAL_MAX_K))
    if not (0.0 <= float(dist_thr) <= LAP_BIG):
        raise L.MvgError("mvg_track_eval: 0 <= dist_thr <= %g expected (got %r)" % (LAP_BIG, dist_thr))
    _launch(name, dets, count, ids, row_pose, joints_3d, joints_3d_vis, num_person, person_id, B, R, J, G, P, K, float(dist_thr),
            *tensors, label="track_eval")
    return buffers


ST_MAX_J, ST_MAX_V, ST_MAX_STEPS = _D["MVG_ST_MAX_J"], _D["MVG_ST_MAX_V"], _D["MVG_ST_MAX_STEPS"]
ST_METHODS = {"LS": _D["MVG_ST_LS"], "ST": _D["MVG_ST_ST"]}
_STRUCTURAL = _Layout("structural_buffers", ("poses", torch.float32, ("B", "P", "J", 3), 0), ("status", torch.int32, ("B", "P"), -1))


def structural_check(parent, n_steps=1, method="ST"):
    """the host-side argument checks of structural_triangulate: parent a tree rooted at joint 0 with 2 .. ST_MAX_J joints, n_steps
    in 1 .. ST_MAX_STEPS, method "ST" or "LS" -> (parent as a ctypes int array, the method's code)"""
    if torch.is_tensor(parent):
        if parent.is_cuda:
            raise RuntimeError("mvg_structural_triangulate: parent travels by value with the launch: host ints expected, not a device "
                               "tensor")
        parent = parent.tolist()
    parent = [int(p) for p in parent]
    J = len(parent)
    if not 2 <= J <= ST_MAX_J:
        raise L.MvgError("mvg_structural_triangulate: unsupported tree of %d joints (2 .. %d)" % (J, ST_MAX_J))
    ok = parent[0] == -1 and all(0 <= p < J for p in parent[1:])
    for i in range(1, J):
        j = i
        for _ in range(J):
            if not ok or j == 0:
                break
            j = parent[j]
        ok = ok and j == 0
    if not ok:
        raise L.MvgError("mvg_structural_triangulate: parent %s is not a tree rooted at joint 0 (parent[0] = -1)" % (parent,))
    if method not in ST_METHODS:
        raise L.MvgError("mvg_structural_triangulate: unknown method %r (one of %s)" % (method, sorted(ST_METHODS)))
    if not 1 <= int(n_steps) <= ST_MAX_STEPS:
        raise L.MvgError("mvg_structural_triangulate: n_steps = %r outside 1 .. %d" % (n_steps, ST_MAX_STEPS))
    return (C.c_int * J)(*parent), ST_METHODS[method]


def structural_buffers(B, P, J, device="cuda"):
    """the static outputs of structural_triangulate(out=...): poses (B, P, J, 3) fp32 zeros and status (B, P) int32 filled with -1
    (not computed).  A caller that captures the launch in a HIP graph allocates them once and keeps them alive with the graph."""
    B, P, J = int(B), int(P), int(J)
    if not (B >= 1 and P >= 1 and 2 <= J <= ST_MAX_J):
        raise L.MvgError("structural_buffers: unsupported shape B = %d, P = %d, J = %d (2 .. %d)" % (B, P, J, ST_MAX_J))
    return _STRUCTURAL.alloc(dict(B=B, P=P, J=J), device)


def structural_triangulate(ud, conf, Pm, parent, bone_lengths, valid=None, rows=None, count=None, n_steps=1, method="ST", out=None):
    """Structural triangulation on the device (mvg_structural_triangulate: one launch, one wavefront per person, fp64, nothing read
    back): every person's J joints from their observations ud (B, V, NQ*J, 2) fp32 (undistorted original-image px) in the views
    Pm (B, V, 3, 4) fp32 with weights conf (B, V, NQ*J) fp32 or None (= 1 / V), under the bone lengths bone_lengths, fp32 (J-1)
    shared or (B, P, J-1) per person (entry k-1: the bone that ends at joint k; None is allowed for method "LS").  parent: the
    tree as J host ints (a sequence or a CPU tensor), parent[0] = -1.
    Persons: dense (rows None): every query, P = NQ, where valid (B, NQ) uint8 is None or non-zero.  Rows: rows (B, P) int32 query
    indices (unit stride in a row; a column slice of a wider tensor is fine) and count (B, 2) int32 or None as pose_nms writes
    keep and count: person (b, p) is query rows[b, p] for p < count[b, 0].
    method "ST": n_steps (1 .. 8) constrained steps; "LS": the unconstrained solution in the same coordinates.
    -> (X (B, P, J, 3) fp32, status (B, P) int32): 0 solved, 1 degenerate or non-finite input (X = 0), 2 a step's multiplier system
    was not positive definite (X from the last completed step), -1 not computed (X = 0).  out: the dict of structural_buffers."""
    L.require_cuda(ud, conf, Pm, bone_lengths, valid, rows, count)
    name = "mvg_structural_triangulate"
    parent_c, method_c = structural_check(parent, n_steps, method)
    J = len(parent_c)
    if ud.dim() != 4 or ud.shape[-1] != 2 or ud.dtype != torch.float32 or ud.shape[2] % J:
        raise RuntimeError("%s: ud (B, V, NQ * %d, 2) float32 expected" % (name, J))
    B, V, Lq = ud.shape[:3]
    NQ = Lq // J
    if Pm.dtype != torch.float32 or tuple(Pm.shape) != (B, V, 3, 4):
        raise RuntimeError("%s: Pm (B, V, 3, 4) float32 expected" % name)
    if conf is not None and (conf.dtype != torch.float32 or tuple(conf.shape) != (B, V, Lq)):
        raise RuntimeError("%s: conf (B, V, NQ * J) float32 or None expected" % name)
    if rows is not None:
        if valid is not None:
            raise RuntimeError("%s: valid selects the persons of the dense mode; it cannot be given with rows" % name)
        if rows.dtype != torch.int32 or rows.dim() != 2 or rows.shape[0] != B or rows.shape[1] < 1:
            raise RuntimeError("%s: rows (B, P) int32 expected" % name)
        if rows.stride(1) != 1 or (B > 1 and rows.stride(0) < rows.shape[1]):
            raise RuntimeError("%s: rows must have unit stride along a row" % name)
        if count is not None and (count.dtype != torch.int32 or tuple(count.shape) != (B, 2)):
            raise RuntimeError("%s: count (B, 2) int32 or None expected" % name)
        P, rows_ld = rows.shape[1], (rows.stride(0) if B > 1 else rows.shape[1])
    else:
        if count is not None:
            raise RuntimeError("%s: count belongs to the rows mode; it cannot be given without rows" % name)
        if valid is not None and (valid.dtype != torch.uint8 or tuple(valid.shape) != (B, NQ)):
            raise RuntimeError("%s: valid (B, NQ) uint8 or None expected" % name)
        P, rows_ld = NQ, 0
    per_person = 0
    if bone_lengths is None:
        if method != "LS":
            raise RuntimeError("%s: method %r needs bone_lengths" % (name, method))
    else:
        if bone_lengths.dtype != torch.float32 or tuple(bone_lengths.shape) not in ((J - 1,), (B, P, J - 1)):
            raise RuntimeError("%s: bone_lengths (J-1) or (B, P, J-1) float32 expected" % name)
        per_person = int(bone_lengths.dim() == 3)
    if not all(t is None or t.is_contiguous() for t in (ud, conf, Pm, bone_lengths, valid, count)):
        raise RuntimeError("%s: every tensor must be contiguous" % name)
    if not 1 <= V <= ST_MAX_V:
        raise L.MvgError("%s: unsupported number of views %d (1 .. %d)" % (name, V, ST_MAX_V))
    if out is None:
        out = structural_buffers(B, P, J, ud.device)
    X, status = out["poses"], out["status"]
    L.require_cuda(X, status)
    _STRUCTURAL.check(out, dict(B=B, P=P, J=J), who=name)
    _launch(name, ud, conf, Pm, valid, rows, rows_ld, count, parent_c, bone_lengths, per_person, method_c, int(n_steps), X, status,
            V, B, NQ, P, J, label="structural_triangulate")
    return X, status


BONES_MAX_W = _D["MVG_BONES_MAX_W"]
_TRACK_BONES = _Layout("track_bones_buffers", ("owner", torch.int32, ("B", "T"), -1), ("seen", torch.int32, ("B", "T"), 0),
                       ("hist", torch.float32, ("B", "T", "W", "K"), 0), ("length", torch.float32, ("B", "T", "K"), 0),
                       ("row_length", torch.float32, ("B", "R", "K"), 0), ("row_source", torch.int32, ("B", "R"), -1))


def _check_bones_limits(who, B, T, J, R, W):
    _check_limits(who, ("B", B, TRACK_MAX_B), ("T", T, TRACK_MAX_T), ("J - 1", J - 1, ST_MAX_J - 1), ("R", R, TRACK_MAX_R),
                  ("W", W, BONES_MAX_W))


def track_bones_buffers(B, T, J, R, W, device="cuda"):
    """the state of track_bones for B streams of T slots, J joints and a window of W frames -- owner (B, T) int32 filled with -1,
    seen (B, T) int32, hist (B, T, W, J-1) fp32, length (B, T, J-1) fp32 -- plus the static outputs row_length (B, R, J-1) fp32 and
    row_source (B, R) int32 (-1).  Allocated once and kept alive by the caller, like track_buffers."""
    B, T, J, R, W = int(B), int(T), int(J), int(R), int(W)
    _check_bones_limits("track_bones_buffers", B, T, J, R, W)
    return _TRACK_BONES.alloc(dict(B=B, T=T, K=J - 1, R=R, W=W), device)


def track_bones(dets, count, track_buffers, parent, bones_buffers, min_frames=4, fallback=None):
    """One frame of the per-track bone-length estimate on the device (mvg_track_bones: one launch behind track_update /
    track_correct, nothing read back, no atomics).  dets (B, R, J, 5) fp32 and count (B, 2) int32 or None as pose_nms leaves them;
    ``track_buffers`` as track_update left them (its slots and id are read, nothing of it is written); parent: the tree as J host
    ints (structural_check); ``bones_buffers`` from track_bones_buffers.  Every slot keeps the bone lengths of its track's last W
    detections (W as the buffers have it) and their median; a slot that changed hands starts over.  -> (row_length (B, R, J-1)
    fp32, row_source (B, R) int32), static tensors of ``bones_buffers``, per row of dets: the slot's median once the slot has
    min_frames samples (source 0), else ``fallback`` (J-1 fp32; source 1) or, without one, the row's own lengths (source 2);
    zeros and -1 for a row that is no detection.  row_length is the per-person bone_lengths of structural_triangulate."""
    name = "mvg_track_bones"
    slots, ident = track_buffers["slots"], track_buffers["id"]
    tensors = [bones_buffers[k] for k in _TRACK_BONES.keys]
    parent_c, _ = structural_check(parent)
    B, R, J = _check_dets(name, dets, count)
    if len(parent_c) != J:
        raise RuntimeError("%s: a tree of %d joints for dets of %d joints" % (name, len(parent_c), J))
    T = ident.shape[1] if ident.dim() == 2 else 0           # as many slots as the tracker's state has
    hist = bones_buffers["hist"]
    W = hist.shape[2] if hist.dim() == 4 else 0             # the window the caller's ring has
    _TRACK.check(track_buffers, dict(B=B, T=T, J=J, R=R), ("slots", "id"), who=name)
    _TRACK_BONES.check(bones_buffers, dict(B=B, T=T, K=J - 1, R=R, W=W), who=name)
    if fallback is not None and (fallback.dtype != torch.float32 or tuple(fallback.shape) != (J - 1,)):
        raise RuntimeError("%s: fallback (J-1) float32 or None expected" % name)
    if not all(t is None or t.is_contiguous() for t in (dets, count, fallback)):
        raise RuntimeError("%s: every tensor must be contiguous" % name)
    L.require_cuda(dets, count, slots, ident, fallback, *tensors)        # behind the shape checks: those hold for any device
    _check_bones_limits(name, B, T, J, R, W)
    if int(min_frames) < 1:
        raise L.MvgError("%s: min_frames >= 1 expected (got %r)" % (name, min_frames))
    _launch(name, dets, count, slots, ident, parent_c, B, R, J, T, W, int(min_frames), fallback, *tensors, label="track_bones")
    return bones_buffers["row_length"], bones_buffers["row_source"]
