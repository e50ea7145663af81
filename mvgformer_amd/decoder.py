"""DQDecoderLayer / DQDecoder -- the MVGFormer decoder with the reference's class surface
(lib/models/dq_decoder.py:248-328,850-1045,1101-1172; base classes lib/models/mvp_decoder.py:49-98,
267-282; MLP lib/models/multi_view_pose_transformer.py:81-102), running on libmvgformer_hip.so.

What differs from the reference by design (MI355X-first, results identical):
  * the V per-view ProjAttn calls of generate_features (dq_decoder.py:553-591) are ONE batched
    launch sequence over all (view, batch) images;
  * camera constants and the crop affine are packed once per forward instead of going through
    numpy/cv2 per view per layer (dq_decoder.py:361-372: a host sync each time);
  * no torch.where / bincount / sort / Python loops (dq_decoder.py:596-656,929-967): every
    query is processed and the validity mask is applied in the final scatter kernel -- every step
    is per-query, so the outputs are the same and the layer never synchronises with the host;
  * the per-valid-query Python loop of 15-matrix SVD launches (multiview.py:262-266) is one
    kernel (thread per joint) that solves the 4x4 normal equations of the DLT rows in fp64.
"""
from __future__ import annotations

import collections
import copy
import os

import torch
import torch.nn.functional as F
from torch import nn

from . import ops
from .projattn import ProjAttn, PyramidProducts, WeightCache, f32_split_on

# backend of the init_self_attention block under autograd, read once: "torch" | "native" (DQDecoderLayer.set_self_attention_training)
SELF_ATTN_TRAIN = os.environ.get("MVG_SELF_ATTN_TRAIN", "torch")
if SELF_ATTN_TRAIN not in ("torch", "native"):
    raise ValueError("MVG_SELF_ATTN_TRAIN must be 'torch' or 'native', got %r" % SELF_ATTN_TRAIN)


class MLP(nn.Module):
    """multi_view_pose_transformer.py:81-102"""

    def __init__(self, input_dim, hidden_dim, output_dim, num_layers):
        super().__init__()
        self.num_layers = num_layers
        h = [hidden_dim] * (num_layers - 1)
        self.layers = nn.ModuleList(nn.Linear(n, k) for n, k in zip([input_dim] + h, h + [output_dim]))

    def forward(self, x):
        for i, layer in enumerate(self.layers):
            x = F.relu(layer(x)) if i < self.num_layers - 1 else layer(x)
        return x


class offset_net(nn.Module):
    """dq_decoder.py:97-111: (dx, dy) pixel offsets + a view-confidence logit."""

    def __init__(self, in_dim, hid_dim, layer_num):
        super().__init__()
        self.MLP = MLP(in_dim, hid_dim, 3, layer_num)

    def forward(self, feature):
        out = self.MLP(feature)
        return out[..., :2], out[..., -1]


def _get_clones(module, N):
    return nn.ModuleList([copy.deepcopy(module) for _ in range(N)])


def _get_activation_fn(activation):
    if activation == "relu":
        return F.relu
    if activation == "gelu":
        return F.gelu
    if activation == "glu":
        return F.glu
    raise RuntimeError(F"activation should be relu/gelu, not {activation}.")


def _mask_indices(indices, B, NQ, device):
    """`indices` given as the matched-query mask (B, NQ) uint8 / bool on the device -> a fresh uint8 mask (the layer may force query
    (0, 0) into it); a list of per-element index tensors stays the other accepted form."""
    if indices.dtype not in (torch.uint8, torch.bool) or tuple(indices.shape) != (B, NQ) or indices.device != torch.device(device):
        raise RuntimeError("indices as a tensor: (B, NQ) = (%d, %d) uint8 / bool mask on %s expected, got %s %s on %s"
                           % (B, NQ, device, tuple(indices.shape), indices.dtype, indices.device))
    return indices.to(torch.uint8).clone()


LayerPlan = collections.namedtuple("LayerPlan", "dt sampler chain_a chain_b binning skip_masked query_term products_ahead grouped")
LayerPlan.__doc__ = """What one DQDecoderLayer.forward_features call runs (DQDecoderLayer.plan decides, everybody else reads):
  dt              compute dtype
  sampler         ProjAttn.sampler_form: "gsamp" | "gfused_f32h" | "gfused_f32" | "gather"
  chain_a / _b    "bf16" (fused LDS-resident chains, csrc/chain.hip), "f32h" (fp32 on pre-split two-part fp16 operands, csrc/f32s.hip)
                  or None (one launch per GEMM / row op); the two can differ
  binning         the (image, query) pairs get a processing order (mvg_bin_pairs: image-space Morton order, pairs outside their image
                  last): "layer" binned per layer, "first" once per forward from the first layer's projections, None: query order
  skip_masked     unfused fp32: output projection + pose MLP skip the tiles whose pairs are all outside their image
  query_term      the previous layer's fused chain B may compute this layer's query term when it runs as this path; None: never
  products_ahead  the pyramid products may be issued ahead of the layer on the decoder's side stream
  grouped         ... and may share a launch with other layers' (ops.pyramid_group_ws)"""
# operands of forward_features in the order the ops take them (DQDecoderLayer._operands)
LayerOperands = collections.namedtuple("LayerOperands", "sampler self_attn chain_a o_masked pose masked_rows chain_b")


def live_view_table(mask, B, V):
    """The live-view table of DecoderContext.set_live_views as host arrays: mask (B, V) or (V,) -- bool; a sequence, a numpy array or
    a CPU tensor -- -> (view_idx (B, V) int32: the live views of stream b in ascending order, padded with -1; n_live (B) int32).
    A device tensor is refused (validating it would need a read-back), and so is a stream without a live view."""
    import numpy as np
    if torch.is_tensor(mask):
        if mask.device.type != "cpu":
            raise TypeError("set_live_views: the mask is validated on the host -- a CPU tensor, numpy array or sequence, not a "
                            "tensor on %s" % (mask.device,))
        mask = mask.detach().numpy()
    m = np.asarray(mask)
    if m.dtype != np.bool_:
        if m.dtype.kind not in "iu" or ((m != 0) & (m != 1)).any():
            raise ValueError("set_live_views: a bool mask expected (got dtype %s)" % (m.dtype,))
        m = m.astype(np.bool_)
    if m.shape == (V,):
        m = np.broadcast_to(m, (B, V))
    if m.shape != (B, V):
        raise ValueError("set_live_views: mask of shape (%d, %d) or (%d,) expected, got %s" % (B, V, V, tuple(m.shape)))
    n_live = m.sum(1).astype(np.int32)
    if (n_live == 0).any():
        raise ValueError("set_live_views: stream %d has no live view" % int(np.flatnonzero(n_live == 0)[0]))
    view_idx = np.full((B, V), -1, dtype=np.int32)
    for b in range(B):
        view_idx[b, :n_live[b]] = np.flatnonzero(m[b])
    return view_idx, n_live


class DecoderContext:
    """Per-forward, layer-independent state: level table + packed cameras (host side, built from
    ``meta``) and the packed channels-last pyramid (device side, built from ``src_views``).

    ``prepare`` touches host memory (it reads the small camera tensors of ``meta``), ``pack`` only
    enqueues kernels -- so a HIP-graph capture can call ``pack`` with a prepared context."""

    # live-view table (set_live_views).  Class defaults: a context that never had a table carries no field for it.
    #   live          None (no table: the launches without one), or the static device pair (view_idx (B, V) i32, n_live (B) i32)
    #   live_buffers  that pair, from the first table on and for good: switching the table off and on again refills the SAME
    #                 tensors, so a graph captured with them keeps addressing live memory
    #   live_staging  (pinned host pair, event recorded behind their last copy) on a CUDA context
    live = live_buffers = live_staging = None

    def __init__(self, levels=None, cams=None, V=0, B=0, dtype=torch.float32):
        self.levels, self.cams, self.V, self.B, self.dtype = levels, cams, V, B, dtype
        self.feat = None
        self._buffer = None    # producer-owned packed pyramid (pyramid_buffers)
        self.packed_event = None    # recorded behind a pack on the decoder's side stream (DQDecoder.pack_pyramid), else None
        # training constants of a context that outlives its forward (training.GraphedTrainStep): the projection matrices of the camera
        # records, the (pointer, version) of the records they were built from, the head's initial reference points
        self.train_Pm = self.train_key = self.train_ref = None

    def set_live_views(self, mask):
        """Which of the V views take part, per stream: mask (B, V) or (V,) bool -- a sequence, a numpy array or a CPU tensor; None
        switches the table off (every launch is then the one without a table; the buffers stay, and ``tensors()`` keeps pinning
        them).  Fills the two static device buffers of ``live`` (live_view_table; allocated by the first call and refilled in
        place ever after: a captured graph addresses them) with one small H2D copy each on the current stream.  On a CUDA context
        the copies leave from two pinned host buffers the context keeps, so they are asynchronous; before refilling those the host
        waits for the event behind the PREVIOUS call's copies (16 + 4 V bytes per stream: long done in a frame loop) -- no device
        synchronisation, nothing waits for the forward.  The forward then gives, bit for bit, what it gives on the live views alone
        (2D outputs of dead views: zeros).  One live view means what a V = 1 run means."""
        if mask is None:
            self.live = None
            return self
        host = tuple(torch.from_numpy(t) for t in live_view_table(mask, self.B, self.V))
        cuda = self.cams.is_cuda
        if self.live_buffers is None:
            if cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("set_live_views: first call inside a HIP-graph capture; set a table before capturing")
            self.live_buffers = tuple(torch.empty(t.shape, dtype=torch.int32, device=self.cams.device) for t in host)
            if cuda:
                self.live_staging = (tuple(torch.empty(t.shape, dtype=torch.int32).pin_memory() for t in host), torch.cuda.Event())
        if cuda:
            with torch.cuda.device(self.cams.device):
                pinned, sent = self.live_staging
                sent.synchronize()          # the copies of the previous table have left the pinned buffers (no-op the first time)
                for dst, stage, src in zip(self.live_buffers, pinned, host):
                    stage.copy_(src)
                    dst.copy_(stage, non_blocking=True)
                sent.record()
        else:
            for dst, src in zip(self.live_buffers, host):
                dst.copy_(src)
        self.live = self.live_buffers
        return self

    @classmethod
    def prepare(cls, spatial_shapes, level_start_index, meta, img_size, dtype, batch_size, device):
        levels = ops.Levels(spatial_shapes, level_start_index)
        cams = ops.pack_cameras(meta, img_size, device)
        V = cams.shape[0] // batch_size
        return cls(levels, cams, V, batch_size, dtype)

    def pack(self, src_views):
        if src_views[0].shape[0] != self.V * self.B:
            raise RuntimeError("meta describes %d images, src_views hold %d" % (self.V * self.B, src_views[0].shape[0]))
        out = self._buffer if (self._buffer is not None and self._buffer.shape[0] == src_views[0].shape[0]) else None
        self.feat = ops.pack_pyramid(src_views, self.levels, self.dtype, out=out)
        return self

    def pyramid_buffers(self, channels=256, device=None):
        """Producer hand-off: allocates the packed pyramid and returns its L levels as
        (V*B, C, H_l, W_l) channels-last views in the compute dtype.  A backbone that writes its feature maps
        into these tensors (or hands them back as ``src_views``) makes ``pack`` free: no 206-MB NCHW->channels-last
        pass (projattn.py:160's cat + permute) per forward."""
        dev = device if device is not None else self.cams.device
        self._buffer = torch.empty((self.V * self.B, self.levels.S, channels), dtype=self.dtype, device=dev)
        return ops.pyramid_level_views(self._buffer, self.levels)

    def proj_matrices(self):
        """training path: the projection matrices of the camera records, rebuilt when the records were replaced or rewritten"""
        key = (self.cams.data_ptr(), self.cams._version)
        if self.train_key != key:
            from . import geometry_torch as G
            self.train_Pm, self.train_key = G.proj_matrices_from_records(self.cams, self.V, self.B), key
        return self.train_Pm

    def set_cameras(self, meta, img_size):
        """new calibration / crop for the same number of images: refills the packed camera records in place (host packing + one small
        H2D copy) and, from them, the training path's projection matrices; a captured graph reads both through the same pointers"""
        fresh = ops.pack_cameras(meta, img_size, self.cams.device)
        if fresh.shape != self.cams.shape:
            raise RuntimeError("set_cameras: %s camera records, the runner was built for %s" % (tuple(fresh.shape), tuple(self.cams.shape)))
        with torch.no_grad():
            self.cams.copy_(fresh)
            if self.train_Pm is not None:       # same tensor, new values, stamped current
                from . import geometry_torch as G
                self.train_Pm.copy_(G.proj_matrices_from_records(self.cams, self.V, self.B))
                self.train_key = (self.cams.data_ptr(), self.cams._version)
        return self

    def tensors(self):
        """the device tensors the context holds (what a captured graph addresses and does not own)"""
        return [t for t in (self.cams, self.feat, self._buffer, self.train_Pm, self.train_ref) + (self.live_buffers or ())
                if t is not None]

    @classmethod
    def build(cls, src_views, spatial_shapes, level_start_index, meta, img_size, dtype, batch_size):
        return cls.prepare(spatial_shapes, level_start_index, meta, img_size, dtype, batch_size,
                           src_views[0].device).pack(src_views)


class DecoderRun:
    """State of ONE forward over an ordered list of layers.  ``with run:`` attaches it to the layers (``_run``) and detaches it however
    the block ends: a hand-off nobody consumed or a hook that never fired goes with it.  The runner sets ``i`` to the position of
    the layer it calls next (a decoder with share_layer_weights holds ONE layer object at every position)."""

    def __init__(self, layers, ctx, chained):
        self.layers, self.ctx, self.chained, self.i = list(layers), ctx, chained, 0
        self.hs_buf = self.flags = self.geo_buf = None      # (layers,B,Lq,C) f32; (layers,) int32 zeros; the stacked 3D / 2D outputs
        # consumed once, by position: the query term (B*Lq,192) f32 from the previous layer's chain B, (new_ref, (r, ref_lvl, inside))
        # from the previous layer's triangulation launch, the callable that issues the NEXT layer's pyramid products
        self.xw_in, self.proj_in, self.after_chain_b = {}, {}, {}
        self.order = None       # "first" binning: the pairs' processing order from the first layer's projections

    def __enter__(self):
        for layer in self.layers:
            layer._run = self
        return self

    def __exit__(self, *exc):
        for layer in self.layers:
            layer._run = None

    def __deepcopy__(self, memo):
        return None         # a copy of a layer is outside every forward

    def next_layer(self):
        """the layer that consumes the current layer's output, when the layers are chained"""
        return self.layers[self.i + 1] if (self.chained and self.i + 1 < len(self.layers)) else None

    def outputs(self):
        """the current layer's slices of the stacked buffers: (hidden state, any-valid flag int32[1], (3D, 2D, projected 2D)) or None"""
        return (None if self.hs_buf is None else self.hs_buf[self.i], None if self.flags is None else self.flags[self.i:self.i + 1],
                None if self.geo_buf is None else tuple(buf[self.i] for buf in self.geo_buf))


def refuse_live_views(ctx, who):
    """the paths that are not built for a live-view table (DecoderContext.set_live_views) say so by name, before any launch"""
    if ctx is not None and getattr(ctx, "live", None) is not None:
        raise NotImplementedError("%s: not built for a live-view table (DecoderContext.set_live_views); run it on all views, or on "
                                  "a rig of the live views" % who)


_NO_RUN = DecoderRun((), None, False)       # what a layer called on its own sees: no context, no next layer, no preallocated outputs


class MvPDecoderLayer(nn.Module):
    """helpers shared with the MvP base class (mvp_decoder.py:49-105)."""

    @staticmethod
    def with_pos_embed(tensor, pos):
        return tensor if pos is None else tensor + pos

    def forward_ffn(self, tgt):
        tgt2 = self.linear2(self.dropout3(self.activation(self.linear1(tgt))))
        tgt = tgt + self.dropout4(tgt2)
        return self.norm3(tgt)

    def norm2absolute(self, norm_coords):
        device = norm_coords.device
        grid_size = self.grid_size.to(device=device)
        grid_center = self.grid_center.to(device=device)
        return norm_coords * grid_size + grid_center - grid_size / 2.0


class DQDecoderLayer(MvPDecoderLayer):
    def __init__(self, space_size, space_center, img_size, pose_embed_layer, d_model=256, d_ffn=1024,
                 dropout=0.1, activation="relu", n_levels=4, n_heads=8, n_points=4,
                 detach_refpoints_cameraprj=True, fuse_view_feats="mean", n_views=5,
                 projattn_posembed_mode="use_rayconv", feature_update_method="MLP",
                 init_self_attention=False, open_forward_ffn=False, query_filter_method="threshold",
                 visualization_jump_num=200, bayesian_update=False, triangulation_method="linalg",
                 filter_query=True, num_joints=15):
        super().__init__()
        # --- same sub-module names / shapes as the reference => same state-dict keys
        self.proj_attn = ProjAttn(d_model, n_levels, n_heads, n_points, projattn_posembed_mode)
        self.dropout1 = nn.Dropout(dropout)
        self.norm1 = nn.LayerNorm(d_model)
        self.self_attn = nn.MultiheadAttention(d_model, n_heads, dropout=dropout)
        self.feature_update_mlp = nn.Linear(d_model, d_model)
        self.dropout2 = nn.Dropout(dropout)
        self.norm2 = nn.LayerNorm(d_model)
        self.linear1 = nn.Linear(d_model, d_ffn)
        self.activation = _get_activation_fn(activation)
        self.activation_name = activation
        self.dropout3 = nn.Dropout(dropout)
        self.linear2 = nn.Linear(d_ffn, d_model)
        self.dropout4 = nn.Dropout(dropout)
        self.norm3 = nn.LayerNorm(d_model)
        self.grid_size = torch.tensor(space_size)
        self.grid_center = torch.tensor(space_center)
        self.img_size = img_size
        self.detach_refpoints_cameraprj = detach_refpoints_cameraprj
        self.fuse_view_feats = fuse_view_feats
        self.pose_embed = offset_net(d_model, d_model, pose_embed_layer)
        self.softmax_conf = nn.Softmax(dim=0)
        self.open_bayesian_update = bayesian_update
        if self.open_bayesian_update:
            self.bayesian_conf = nn.Linear(d_model, 1)
        self.use_confidences = False
        self.class_embed = nn.Linear(d_model, 2)
        self.num_joints = num_joints
        self.feature_update_method = feature_update_method
        self.init_self_attention = init_self_attention
        self.open_forward_ffn = open_forward_ffn
        self.query_filter_method = query_filter_method
        self.visualization_jump_num = visualization_jump_num
        self.triangulation_method = triangulation_method
        self.filter_query = filter_query
        self.d_model = d_model
        self.compute_dtype = torch.float32
        self.training_dtype = torch.float32     # set_training_dtype
        self.self_attention_training = SELF_ATTN_TRAIN      # set_self_attention_training
        self.use_fused_chains = True    # bf16 inference: LDS-resident Linear chains (csrc/chain.hip)
        # fp32 inference: the same two chains on pre-split operands (csrc/f32s.hip); MVG_F32_FUSED=0: one launch per GEMM / row op
        self.use_fused_chains_f32 = os.environ.get("MVG_F32_FUSED", "1") != "0"
        self.fuse_boundary = True       # the triangulation launch also projects the new points for the next layer
        # fp32 path: output projection + pose MLP skip the tiles whose pairs are all outside their image (round 3)
        self.skip_masked_f32 = True
        self._wc = WeightCache()
        self._run = None   # the DecoderRun of the forward this layer is part of; None outside one
        # query-sharded runs (mvgformer_amd.dist): callable(any_valid int32[1]) that makes the
        # "no query valid anywhere -> force query (0,0)" rule (dq_decoder.py:620-623) global
        self._any_valid_hook = None

    # ------------------------------------------------------------------------------ config
    def set_compute_dtype(self, dtype):
        """torch.float32 (reference arithmetic) or torch.bfloat16 (bf16 storage + bf16 MFMA with
        fp32 accumulation; geometry stays fp32/fp64)."""
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("compute dtype must be float32 or bfloat16")
        self.compute_dtype = dtype
        self.proj_attn.compute_dtype = dtype
        return self

    def set_training_dtype(self, dtype):
        """Precision of the autograd path (forward_autograd: grad enabled, or dropout active).  torch.float32 (default): fp32 storage,
        fp32-accurate GEMMs.  torch.bfloat16: mixed precision -- bf16 GEMM operands with fp32 accumulation, fp32 master weights and
        fp32 gradients, a bf16 value for the sampling op (rounding points: forward_autograd).  LayerNorm, softmax, dropout, sigmoid
        and all geometry stay fp32 / fp64.  The native inference path, compute_dtype, GraphedDecoder and the query-sharded
        runners do not read it.  torch.autocast is NOT consulted: this switch alone selects the bf16 path.  The self-attention block
        of init_self_attention follows it only on the native backend (set_self_attention_training("native"): bf16 q, k, v and the
        bf16 attention kernels, fp32 projections); through torch's module it stays fp32 either way."""
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("training dtype must be float32 or bfloat16")
        self.training_dtype = dtype
        self.proj_attn.training_dtype = dtype
        return self

    def set_self_attention_training(self, backend):
        """Backend of the init_self_attention block on the autograd path (_attend_queries_autograd).  "torch" (default, or the
        environment variable MVG_SELF_ATTN_TRAIN): nn.MultiheadAttention, fp32.  "native": the HIP training kernels of
        csrc/mha.hip -- forward with lse, deterministic backward, attention dropout inside the kernels -- in training_dtype
        (_attend_queries_native).  The inference path does not read it."""
        if backend not in ("torch", "native"):
            raise ValueError("self-attention training backend must be 'torch' or 'native'")
        self.self_attention_training = backend
        return self

    def _check_supported(self):
        bad = None
        if self.feature_update_method != "MLP":
            bad = "feature_update_method=%r" % self.feature_update_method
            if self.feature_update_method.startswith("attention"):
                bad += " (the attention* feature updates of dq_decoder.py:779-830 are not built)"
        elif self.init_self_attention and (self.d_model != 256 or self.self_attn.num_heads != 8):
            bad = "init_self_attention=True with d_model=%d, nhead=%d (the attention kernel is built for 256 / 8)" \
                % (self.d_model, self.self_attn.num_heads)
        elif self.open_bayesian_update:
            bad = "bayesian_update=True"
        elif self.triangulation_method not in ("linalg", "batch", "default", "cpu"):
            bad = "triangulation_method=%r" % self.triangulation_method
        elif self.filter_query and self.query_filter_method not in ("threshold", "all"):
            bad = "query_filter_method=%r" % self.query_filter_method
        elif self.activation_name != "relu":
            bad = "activation=%r" % self.activation_name
        elif len(self.pose_embed.MLP.layers) < 1 or self.pose_embed.MLP.layers[-1].out_features != 3:
            bad = "pose_embed shape"
        elif not self.proj_attn.fused_supported(3):
            bad = "ProjAttn geometry (need d_model=256, nhead=8, dec_n_points=8, num_feature_levels=1)"
        if bad:
            # of the cross-query variants only init_self_attention is built (attend_queries)
            raise NotImplementedError("DQDecoderLayer: %s is outside the built hot path (feature_update_method='MLP', "
                                      "init_self_attention=False | True, triangulation_method='linalg', "
                                      "bayesian_update=False)" % bad)

    def _w(self, key, params, dtype, build=None):
        return self._wc.get(key, params, dtype, build)

    def _mfma_operand(self, path, dt):
        """(key, weight) -> the cached operand of one MFMA weight as `path`'s kernels take it, as a tuple to splice into an argument
        list: "bf16" (fragments,); "f32h" (two fp16 planes, their power-of-two scale); None (the weight in dt,)"""
        if path == "f32h":
            return lambda key, w: self._w(key + "_f32h", (w,), torch.float16, ops.split_swizzle_weight_h2)
        if path == "bf16":
            return lambda key, w: (self._w(key + "_sw", (w,), dt, lambda t: ops.swizzle_weight(t.to(dt))),)
        return lambda key, w: (self._w(key, (w,), dt),)

    def _pose_operands(self, path, dt):
        """(W0, b0, W1, b1, ..., W_last, b_last) of the pose MLP, the hidden layers' weights as `path` takes them (_mfma_operand)"""
        f32, mm = torch.float32, self._mfma_operand(path, dt)
        layers = list(self.pose_embed.MLP.layers)       # (a slice of a ModuleList would be a new module)
        hidden = sum((mm("Wpe%d" % i, lin.weight) + (self._w("bpe%d" % i, (lin.bias,), f32),) for i, lin in enumerate(layers[:-1])), ())
        return hidden + (self._w("Wpe_last", (layers[-1].weight,), f32), self._w("bpe_last", (layers[-1].bias,), f32))

    def _chain_a_operands(self, path, dt):
        """operands of ops.chain_attn_pose ("bf16") / ops.chain_attn_pose_f32h ("f32h") and that kernel's masked-row constant"""
        out_proj = self.proj_attn.output_proj
        wts = (self._mfma_operand(path, dt)("Wp", out_proj.weight) + (self._w("bp", (out_proj.bias,), torch.float32),)
               + self._pose_operands(path, dt))
        params = tuple(p for lin in self.pose_embed.MLP.layers for p in (lin.weight, lin.bias))
        key, build = "o_masked", ops.chain_masked_row_output
        if path == "f32h":
            key, build, params = "o_masked_f32h", ops.chain_masked_row_output_f32h, params + (out_proj.bias,)
        # o of a masked row, computed by the kernel that is going to use it (the variants reduce the last pose layer in
        # different orders; a masked row inside a mixed tile and one in an all-masked tile must agree bit for bit)
        return wts, self._w(key, params, torch.float32, lambda *_: build(*wts))

    def _pose_masked_rows(self, dt):
        """what the hidden pose-MLP layers give for a pair outside its image (attn row = 0): layer i's output row, computed by the
        GEMM kernel itself on a one-row input so that rows of all-masked tiles (broadcast) and masked rows inside computed tiles
        agree bit for bit.  Cached per weight version."""
        f32 = torch.float32
        layers = self.pose_embed.MLP.layers[:-1]
        params = tuple(p for lin in layers for p in (lin.weight, lin.bias))

        def build(*_):
            rows, cur = [], torch.zeros((1, layers[0].weight.shape[1]), dtype=f32, device=layers[0].weight.device)
            for lin in layers:
                cur = ops.linear(cur, lin.weight.detach().to(f32).contiguous(), lin.bias.detach().to(f32).contiguous(), relu=True)
                rows.append(cur[0])
            return torch.stack(rows)
        # keyed on the active GEMM form as well: the rows must come from the form that computes the unmasked tiles
        from . import _lib
        _lib.load()         # fills TUNING
        return self._w("pose_masked_rows/f32_split=%d" % _lib.TUNING["f32_split"], params, f32, build)

    def _chain_b_operands(self, path, dt):
        """(Wu, bu, g2, b2, W1, b1, W2, bb2, g3, b3, Wc, bc): feature update, FFN (None without open_forward_ffn) and class head, the
        three MFMA weights as `path` takes them (_mfma_operand) -- the argument order of ops.chain_update_ffn_class ("bf16") and,
        each of the three followed by its scale, of ops.chain_update_ffn_class_f32h ("f32h"); None: the unfused ops' operands"""
        f32, mm, ffn = torch.float32, self._mfma_operand(path, dt), self.open_forward_ffn
        none = (None, 0) if path == "f32h" else (None,)
        vec = lambda key, p, on=True: self._w(key, (p,), f32) if on else None
        return (mm("Wu", self.feature_update_mlp.weight)
                + (vec("bu", self.feature_update_mlp.bias), vec("g2", self.norm2.weight), vec("b2", self.norm2.bias))
                + (mm("W1", self.linear1.weight) if ffn else none) + (vec("b1", self.linear1.bias, ffn),)
                + (mm("W2", self.linear2.weight) if ffn else none)
                + (vec("bb2", self.linear2.bias, ffn), vec("g3", self.norm3.weight, ffn), vec("b3", self.norm3.bias, ffn),
                   vec("Wc", self.class_embed.weight), vec("bc", self.class_embed.bias)))

    def plan(self, dt, Lq=None, levels=None, sampler=None):
        """The LayerPlan of a forward_features call in compute dtype dt on Lq queries per batch element and the pyramid `levels`:
        the ONLY place the kernel paths are decided.  Not cached: a handful of comparisons on switches that may change between
        calls.  Lq None: any query count (inside every window).  levels: an ops.Levels or its (L, S); read, with Lq, by the fp32
        sampler choice alone, which raises without them where the shape decides (ProjAttn.f32_g_form) -- bf16 needs neither.
        sampler: plan for this form instead of the one the shape selects (prepare_caches without a shape)."""
        pa, f32 = self.proj_attn, dt == torch.float32
        if sampler is None:
            L, S = (None, None) if levels is None else (levels.L, levels.S) if hasattr(levels, "L") else levels
            sampler = pa.sampler_form(dt, Lq, L, S)
        d256 = self.d_model == 256      # (the width of the pose MLP's hidden layers and of the FFN's input as well)
        pose_ok = d256 and self.pose_embed.MLP.num_layers == 3
        ffn_ok = d256 and (not self.open_forward_ffn or self.linear1.out_features == 1024)
        if f32:
            # (the library's f32_split knob selects the reference-arithmetic GEMMs: the fused kernels, whose products are split by
            # construction, stand down with it; chain A reads the G-sampler's output in processing order)
            fused = bool(self.use_fused_chains_f32) and f32_split_on()
            chain_a = "f32h" if (fused and pose_ok and sampler == "gfused_f32h") else None
            chain_b = "f32h" if (fused and ffn_ok and self.num_joints <= 32) else None
        else:
            fused = dt == torch.bfloat16 and bool(self.use_fused_chains)
            chain_a = "bf16" if (fused and pose_ok) else None
            chain_b = "bf16" if (fused and ffn_ok and self.num_joints <= 64) else None
        sort = pa.sort_pairs if (Lq is None or Lq <= 65536) else False
        # Skipping is worth 1.7 % at cfg-2 (41 % of the tiles skipped at layer 0, but the GEMM is power-limited: tiles of zero rows
        # were cheap already); below 8192 tokens per image (cfg-4) the extra binning launch costs more than it saves.
        skip_masked = bool(f32 and chain_a is None and self.skip_masked_f32 and d256 and sort
                           and (Lq is None or Lq >= 8192))
        if not sort or (sampler == "gather" and chain_a is None and not skip_masked):
            binning = None      # (nothing reads an order)
        else:
            binning = "first" if (sort == "first" and chain_a == "bf16") else "layer"
        ahead = sampler != "gather" and (f32 or bool(self.use_fused_chains))
        # a layer that attends first projects attend_queries(tgt') + query_pos: tgt' + query_pos is not its query
        query_term = None if self.init_self_attention else chain_a if f32 else "bf16" if ahead else None
        return LayerPlan(dt, sampler, chain_a, chain_b, binning, skip_masked, query_term, ahead, sampler == "gsamp")

    def _operands(self, plan):
        """Every cached operand a forward_features call with this plan reads, built on first use: forward_features takes its
        operands from here, prepare_caches builds them by calling this.  The output projection's and the query term's (read by
        the previous layer's chain B: _next_query_term) are fetched inside ProjAttn through the methods called here."""
        dt, pa = plan.dt, self.proj_attn
        if plan.query_term is not None:
            pa.query_term_weights(dt, plan.query_term)
        if plan.chain_a is not None:
            chain_a, o_masked = self._chain_a_operands(plan.chain_a, dt)
            pose = None
        else:
            pa.output_operands(dt, plan.skip_masked)
            chain_a, o_masked, pose = None, None, self._pose_operands(None, dt)
        return LayerOperands(pa.sampler_operands(plan.sampler, dt), self._self_attn_weights(dt) if self.init_self_attention else None,
                             chain_a, o_masked, pose, self._pose_masked_rows(dt) if plan.skip_masked else None,
                             self._chain_b_operands(plan.chain_b, dt))

    def _self_attn_weights(self, dt):
        """cached operands of attend_queries: ([Wq; Wk] (512, C), its bias, Wv, its bias, out_proj weight, bias, norm2 weight, bias)"""
        f32 = torch.float32
        sa, C = self.self_attn, self.d_model
        if sa.in_proj_weight is None or sa.in_proj_bias is None or sa.bias_k is not None:
            raise NotImplementedError("DQDecoderLayer: self_attn with separate projection weights, without bias or with bias_k / "
                                      "bias_v is not built")
        return (self._w("sa_Wqk", (sa.in_proj_weight,), dt, lambda w: w[:2 * C]), self._w("sa_bqk", (sa.in_proj_bias,), f32, lambda b: b[:2 * C]),
                self._w("sa_Wv", (sa.in_proj_weight,), dt, lambda w: w[2 * C:]), self._w("sa_bv", (sa.in_proj_bias,), f32, lambda b: b[2 * C:]),
                self._w("sa_Wo", (sa.out_proj.weight,), dt), self._w("sa_bo", (sa.out_proj.bias,), f32),
                self._w("g2", (self.norm2.weight,), f32), self._w("b2", (self.norm2.bias,), f32))

    def attend_queries(self, tgt, query_pos, weights=None):
        """The block init_self_attention puts at the head of the layer (dq_decoder.py:532-539), eval mode, on the native kernels:
            norm2(tgt + out_proj(attention(Wq x, Wk x, Wv tgt))),  x = tgt + query_pos
        over the Lq = NQ * J tokens of each batch element -- (B, Lq, C) fp32.  In-projection ([Wq; Wk] as one 512-wide product with
        the sum folded into its load; Wv) and out_proj on mvg_linear in the compute dtype, the attention on mvg_self_attention
        (csrc/mha.hip) where the projections lie, the residual + LayerNorm on mvg_add_layernorm.  In the reference the result is a
        local of generate_features: it stands in for tgt in the projective attention's query and nowhere else (forward_features)."""
        if not tgt.is_cuda:
            raise RuntimeError("Not implemented on the CPU")
        B, Lq, C = tgt.shape
        dt = self.compute_dtype
        Wqk, bqk, Wv, bv, Wo, bo, g2, b2 = weights or self._self_attn_weights(dt)
        t32 = tgt.float().reshape(B * Lq, C).contiguous()
        if query_pos is None:
            qk = ops.linear(t32, Wqk, bqk, out_dtype=dt)
        elif query_pos.shape == tgt.shape:
            qk = ops.linear(t32, Wqk, bqk, out_dtype=dt, add=query_pos.float().reshape(B * Lq, C).contiguous())
        else:
            qk = ops.linear((tgt.float() + query_pos.float()).reshape(B * Lq, C).contiguous(), Wqk, bqk, out_dtype=dt)
        v = ops.linear(t32, Wv, bv, out_dtype=dt)
        qk = qk.view(B, Lq, 2 * C)
        a = ops.self_attention(qk[..., :C], qk[..., C:], v.view(B, Lq, C))
        o = ops.linear(a.view(B * Lq, C), Wo, bo, out_dtype=dt)
        return ops.add_layernorm(t32, o, g2, b2).view(B, Lq, C)

    def _next_query_term(self, nxt, path_b, tgt, query_pos, levels):
        """operands with which this layer's fused chain B also computes xw = (tgt' + query_pos) W^T + b, the query term of the next layer
        `nxt` (its rows are in LDS): (qp, W, b, n) for the bf16 chain, (qp, W, scale, b, n) for the f32h one; None: not taken"""
        dt = self.compute_dtype
        if nxt is None or nxt.compute_dtype != dt or not (query_pos is None or query_pos.shape == tgt.shape):
            return None
        if nxt.plan(dt, tgt.shape[1], levels).query_term != path_b:
            return None
        qp = None if query_pos is None else query_pos.float().reshape(-1, tgt.shape[2]).contiguous()
        return (qp,) + nxt.proj_attn.query_term_weights(dt, path_b)

    def prepare_caches(self, dtype=None, Lq=None, levels=None):
        """Build every cached operand of the inference path on the CURRENT stream, outside any graph capture (some launch a
        kernel: o_masked, the masked rows).  An entry created inside a capture would live in the graph's private pool and stay
        unwritten until the first replay -- WeightCache.get refuses to do that.  DQDecoder calls this before it forks its side
        stream, the sharded runners (mvgformer_amd.dist) before they capture.  With the shape of the forward (Lq, levels): the
        operands of its plan; without: of every plan some shape can select under the current switches."""
        dt = dtype or self.compute_dtype
        for form in ((None,) if levels is not None else self.proj_attn.sampler_forms(dt)):
            self._operands(self.plan(dt, Lq, levels, sampler=form))
        return self

    def _forced_queries(self, indices, B, NQ, device, dtype=torch.uint8):
        """(B, NQ) mask of the queries the filter is told to keep -- all of them (filter_query off, query_filter_method "all"),
        the matcher's mask (indices as a tensor) or the listed ones (indices as a list of per-element index tensors); None: the
        class head decides"""
        if not self.filter_query or self.query_filter_method == "all":
            return torch.ones((B, NQ), dtype=dtype, device=device)
        if torch.is_tensor(indices):
            return _mask_indices(indices, B, NQ, device).to(dtype)
        if indices is None:
            return None
        forced = torch.zeros((B, NQ), dtype=dtype, device=device)
        for b, q in enumerate(indices):
            forced[b, torch.as_tensor(q, dtype=torch.long, device=device)] = 1
        return forced

    # ----------------------------------------------------------------------------- forward
    def forward(self, tgt, query_pos, reference_points, src_views, src_spatial_shapes, level_start_index, meta,
                src_padding_mask=None, rgb_views=None, output_dir="./", frame_id=None, indices=None,
                threshold=0.5, indices_all=None):
        """dq_decoder.py:850-1045.  tgt, query_pos (B,Lq,C); reference_points (B,Lq,1,3) or
        (B,Lq,3) in mm; src_views list of L (V*B,C,H,W) maps, view-major; meta list[V] of dicts.
        Returns (tgt_update (B,Lq,C), new_reference_points (B,Lq,3), refined_2d_abs (B,V,Lq,2),
        projs_2d_abs (B,V,Lq,2), class_prob (B,NQ,2)); 3D / 2D outputs are zero for queries that
        do not pass the filter."""
        if not tgt.is_cuda:
            raise RuntimeError("Not implemented on the CPU")
        self._check_supported()
        with torch.cuda.device(tgt.device):     # kernels go to the current stream of the TENSORS' device
            return self._forward(tgt, query_pos, reference_points, src_views, src_spatial_shapes, level_start_index, meta,
                                 indices, threshold)

    def takes_autograd_path(self, tgt):
        """True when forward() on tgt runs forward_autograd instead of the native kernels: under autograd, or in train() mode with
        active dropout.  The ONE statement of that rule (_forward takes the path by it, DQDecoder.forward refuses by it)."""
        dropping = self.training and max(self.dropout2.p, self.dropout3.p, self.dropout4.p) > 0
        return bool(dropping or (torch.is_grad_enabled()
                                 and (tgt.requires_grad or any(p.requires_grad for p in self.parameters()))))

    def _forward(self, tgt, query_pos, reference_points, src_views, src_spatial_shapes, level_start_index, meta, indices,
                 threshold):
        # The native path has no dropout: it is the eval()-mode layer.  Under autograd, and in train() mode with active
        # dropout (validation inside a training loop without .eval(), MC-dropout), the differentiable torch path runs,
        # which applies dropout2/3/4 like the reference (dq_decoder.py:776, mvp_decoder.py:94-98).
        if self.takes_autograd_path(tgt):
            return self.forward_autograd(tgt, query_pos, reference_points, src_views, src_spatial_shapes,
                                         level_start_index, meta, indices, threshold)
        ctx = (self._run or _NO_RUN).ctx
        if ctx is None:
            ctx = DecoderContext.build(src_views, src_spatial_shapes, level_start_index, meta, self.img_size,
                                       self.compute_dtype, tgt.shape[0])
        st = self.forward_features(tgt, query_pos, reference_points, ctx, threshold, indices)
        if self._any_valid_hook is not None:
            self._any_valid_hook(st["any_valid"])
        return self.forward_triangulate(st, ctx)

    def _lin_bf16(self, x, weight, bias, relu=False):
        from .functions import linear_bf16
        return linear_bf16(x, weight, bias, self._wc, "train16/%x" % id(weight), relu=relu)

    def _img_size_on(self, dev):
        """(2,) f32 image size on `dev`: uploaded once per device (an H2D copy from pageable memory synchronises, and cannot be part
        of a graph capture)"""
        held = self.__dict__.setdefault("_img_dev", {})
        key = (dev, tuple(float(v) for v in self.img_size))     # a reassigned img_size gets its own upload
        t = held.get(key)
        if t is None:
            if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("DQDecoderLayer.forward_autograd: first call on %s inside a HIP-graph capture; run one eager "
                                   "training forward before capturing" % (dev,))
            t = held[key] = torch.tensor(self.img_size, dtype=torch.float32, device=dev)
        return t

    def forward_autograd(self, tgt, query_pos, reference_points, src_views, src_spatial_shapes, level_start_index, meta,
                         indices=None, threshold=0.5):
        """Training path: the same layer as differentiable torch ops (fp32) with the HIP sampling op
        (DeformFunction forward + backward kernels) inside ProjAttn -- what run/train_3d.py needs
        (SURVEY.md section 8 f2).  Dense compute + masking instead of the reference's gather/pad/scatter
        (every step is per-query, so values and gradients of the kept queries are the same).

        training_dtype bfloat16 (set_training_dtype; torch.autocast is not consulted) rounds to bf16 at exactly these points:
          forward
            * the input of every Linear with both widths multiples of 64 (LinearBF16): the ProjAttn value projection rayconv, its
              [sampling_offsets; attention_weights] projection, output_proj, feature_update_mlp, linear1 / linear2 (FFN) and the
              first two pose-MLP layers -- and their weights (cast once per optimizer step); products accumulate in fp32, bias
              and ReLU are applied to the fp32 sum;
            * the value projection's output (the sampling op's value is bf16), and so the sampling op's output (bf16, from fp32
              arithmetic on the widened value);
            * with a bf16 packed pyramid (a DecoderContext built for compute_dtype bf16): the pyramid itself, and the gathered
              reference-point input bf16(bilinear + query);
          backward
            * dy of every LinearBF16 before its dgrad and wgrad (dW, db fp32 sums of bf16 products);
            * the gradient of every bf16 tensor above (value, the sampling output, a bf16 gathered input): autograd hands it back
              in that tensor's dtype;
          everything else -- the 2- and 3-output heads (class_embed, the last pose layer: fp32-accurate split GEMMs), LayerNorm,
          softmax, dropout, sigmoid, the sampling op's locations / weights / gradients (fp32), UncropUndistort (fp32),
          DenseDLT (fp64) -- is the fp32 path's arithmetic."""
        from . import geometry_torch as G
        refuse_live_views((self._run or _NO_RUN).ctx, "DQDecoderLayer.forward_autograd")
        B, Lq, C = tgt.shape
        J = self.num_joints
        NQ = Lq // J
        V = len(meta)
        dev = tgt.device
        img = self._img_size_on(dev)
        X = reference_points.reshape(B, Lq, 3)
        if self.detach_refpoints_cameraprj:
            X = X.detach()                                                    # dq_decoder.py:338-339
        WH = src_spatial_shapes.flip(-1).float()
        x = self.with_pos_embed(self._attend_queries_autograd(tgt, query_pos) if self.init_self_attention else tgt, query_pos)
        # Per-forward constants of the geometry (packed camera records, level table, projection matrices): built once and kept on the
        # DecoderContext when the layer runs inside DQDecoder.forward -- as torch ops per layer they were ~40 launches each.
        ctx = (self._run or _NO_RUN).ctx
        if ctx is not None:
            cams, levels, Pm = ctx.cams, ctx.levels, ctx.proj_matrices()
        else:
            cams, levels = ops.pack_cameras(meta, self.img_size, dev), ops.Levels(src_spatial_shapes, level_start_index)
            Pm = G.proj_matrices_from_records(cams, V, B)
        # all V views as ONE batch of V*B images (image n = v*B + b, the order of src_views): one projection, one ProjAttn
        # call and one pose MLP instead of V of each -- the training step is launch-bound (5 800 launches per step at cfg-2)
        if not X.requires_grad:
            # the reference points do not carry a gradient into the projection (detach_refpoints_cameraprj, every shipped YAML):
            # the inference kernel projects them (one launch, same arithmetic: tests/test_hip_parity.py)
            r_all, ref_lvl, inside_u8 = ops.project(X.float().contiguous(), cams, levels, V, B)
            inside_all = inside_u8.bool()
        else:
            cam_all = {k: torch.cat([meta[v]["camera"][k].to(dev) for v in range(V)], 0)
                       for k in ("R", "T", "fx", "fy", "cx", "cy", "k", "p")}
            center_all = torch.cat([meta[v]["center"].to(dev) for v in range(V)], 0)
            A_crop = torch.cat([G.crop_affine(meta[v]["center"], meta[v]["scale"], self.img_size, dev) for v in range(V)], 0)
            r_all, inside_all = G.project_points(X.repeat(V, 1, 1), cam_all, center_all, A_crop, self.img_size, views=V)
            ref_lvl = r_all.unsqueeze(2) * WH / (WH - 1)                           # dq_decoder.py:570-573
        a_all = self.proj_attn(x.repeat(V, 1, 1), ref_lvl, src_views, None, src_spatial_shapes, level_start_index,
                               packed=None if ctx is None else ctx.feat)
        a_all = inside_all.unsqueeze(-1).to(a_all.dtype) * a_all                   # dq_decoder.py:585-586
        from .functions import linear as lin
        if self.training_dtype == torch.bfloat16:
            lin = self._lin_bf16
        mean = a_all.view(V, B, Lq, C).mean(0)
        tgt_update = self.norm2(tgt + self.dropout2(lin(mean, self.feature_update_mlp.weight, self.feature_update_mlp.bias)))
        if self.open_forward_ffn:           # forward_ffn (mvp_decoder.py:94-98) with the two GEMMs on mvg_linear
            h1 = lin(tgt_update, self.linear1.weight, self.linear1.bias, relu=self.activation_name == "relu")
            if self.activation_name != "relu":
                h1 = self.activation(h1)
            tgt_update = self.norm3(tgt_update + self.dropout4(lin(self.dropout3(h1), self.linear2.weight, self.linear2.bias)))
        prob = lin(tgt_update, self.class_embed.weight, self.class_embed.bias).view(B, NQ, J, 2).sigmoid().mean(2)
        valid = self._forced_queries(indices, B, NQ, dev, torch.bool)    # (a tensor: the matcher's mask, criterion.KNNMatcher.match)
        if valid is None:
            valid = prob[..., 1] > threshold
        # no query kept -> the first one is (dq_decoder.py:620-623), decided on the device (no host sync in the step)
        valid[0, 0] |= ~valid.any()
        hp = a_all                                                              # offset_net (dq_decoder.py:97-111)
        pl = self.pose_embed.MLP.layers
        for i, layer_ in enumerate(pl):
            hp = lin(hp, layer_.weight, layer_.bias, relu=i < len(pl) - 1)
        off, cl = hp.split([2, 1], -1)                                          # (V*B,Lq,2), (V*B,Lq,1)
        ref2d = ((r_all + off / img) * img).view(V, B, Lq, 2).transpose(0, 1)    # (B,V,Lq,2)
        proj2d = (r_all * img).view(V, B, Lq, 2).transpose(0, 1)
        conf = torch.softmax(cl.reshape(V, B, Lq).transpose(0, 1), 1)
        # un-crop + undistortion (dq_decoder.py:414-420, 119-204): one launch forward (with every point's Jacobian), one small
        # product backward (geometry_torch.UncropUndistort) -- as torch ops ~80 launches forward and ~160 backward per layer.
        # Triangulation (dq_decoder.py:929-967): one launch each way over the dense token grid (geometry_torch.DenseDLT).  Only the
        # matched queries are triangulated, like the reference: an unmatched query with a degenerate DLT (homogeneous w == 0, an
        # Inf 2D point) would otherwise put 0 * inf = NaN into the gradients of the parameters all queries share.
        ud = G.UncropUndistort.apply(ref2d, cams, V, B)
        new_ref = G.DenseDLT.apply(ud, conf, Pm, valid.to(torch.uint8), J)
        vm2 = valid.view(B, 1, NQ, 1, 1)
        zero = torch.zeros((), device=dev)
        ref2d_o = torch.where(vm2, ref2d.view(B, V, NQ, J, 2), zero).reshape(B, V, Lq, 2)
        proj2d_o = torch.where(vm2, proj2d.view(B, V, NQ, J, 2), zero).reshape(B, V, Lq, 2)
        return tgt_update, new_ref, ref2d_o, proj2d_o, prob

    def _attend_queries_autograd(self, tgt, query_pos):
        """attend_queries as differentiable torch ops through the layer's own self_attn module (dq_decoder.py:532-539): torch's
        attention op with need_weights=False (no Lq x Lq probabilities are returned or kept for the caller), attention dropout
        and dropout2 as in the reference.  fp32 whatever training_dtype says.  With set_self_attention_training("native") the
        block runs on the HIP training kernels instead (_attend_queries_native), in training_dtype."""
        if self.self_attention_training == "native":
            return self._attend_queries_native(tgt, query_pos)
        f32 = torch.float32
        t = tgt.to(f32)
        qk = self.with_pos_embed(t, None if query_pos is None else query_pos.to(f32)).transpose(0, 1)
        with torch.autocast(device_type=tgt.device.type, enabled=False):
            tgt2 = self.self_attn(qk, qk, t.transpose(0, 1), need_weights=False)[0].transpose(0, 1)
        return self.norm2(t + self.dropout2(tgt2))

    def _attend_queries_native(self, tgt, query_pos):
        """_attend_queries_autograd on the project's own kernels: [Wq; Wk] on tgt + query_pos and Wv on tgt as fp32
        functions.linear (LinearF32S), functions.self_attention on the column blocks where they lie (csrc/mha.hip: forward with
        lse, deterministic backward; attention dropout inside the kernels while self.training), out_proj as functions.linear,
        norm2(t + dropout2(.)).  training_dtype bfloat16 rounds q, k, v to bf16 and runs the bf16 kernels (P, dP, dS, lse, delta
        fp32; the attention output and dq, dk, dv bf16); the three projections keep fp32 operands."""
        from . import functions as Fn
        if not tgt.is_cuda:
            raise RuntimeError("Not implemented on the CPU")
        sa, f32, C = self.self_attn, torch.float32, self.d_model
        if sa.in_proj_weight is None or sa.in_proj_bias is None or sa.bias_k is not None or sa.bias_v is not None:
            raise NotImplementedError("DQDecoderLayer: self_attn with separate projection weights, without bias or with bias_k / "
                                      "bias_v is not built")
        t = tgt.to(f32)
        x = self.with_pos_embed(t, None if query_pos is None else query_pos.to(f32))
        qk = Fn.linear(x, sa.in_proj_weight[:2 * C], sa.in_proj_bias[:2 * C])
        v = Fn.linear(t, sa.in_proj_weight[2 * C:], sa.in_proj_bias[2 * C:])
        if self.training_dtype == torch.bfloat16:
            qk, v = qk.to(torch.bfloat16), v.to(torch.bfloat16)
        a = Fn.self_attention(qk[..., :C], qk[..., C:], v, dropout_p=sa.dropout, training=self.training)
        tgt2 = Fn.linear(a.to(f32), sa.out_proj.weight, sa.out_proj.bias)
        return self.norm2(t + self.dropout2(tgt2))

    # The layer in two halves, so that a query-sharded run can put its one per-layer exchange (the global
    # "any query valid" flag, mvgformer_amd.dist) between two captured HIP-graph segments.
    def forward_features(self, tgt, query_pos, reference_points, ctx, threshold, indices=None, query_tgt=None):
        """steps 1-4 of dq_decoder.py:850-1045: projection, projective attention, feature update, class
        head + filter, 2D offsets.  Returns the state consumed by forward_triangulate.
        query_tgt: what stands in for tgt in the projective attention's query x = tgt + query_pos; with init_self_attention the
        layer computes it itself (attend_queries).  As in the reference, where the attended tgt is a local of generate_features
        (dq_decoder.py:532-540), the feature update still adds its residual to the layer's own tgt (dq_decoder.py:882)."""
        B, Lq, C = tgt.shape
        J = self.num_joints
        NQ = Lq // J
        dt = self.compute_dtype
        V = ctx.V
        run = self._run or _NO_RUN
        plan = self.plan(dt, Lq, ctx.levels)
        w = self._operands(plan)
        if query_tgt is None and self.init_self_attention:
            query_tgt = self.attend_queries(tgt, query_pos, w.self_attn)

        # 1. projective attention features of every view (generate_features, dq_decoder.py:516-593)
        X = reference_points.detach().reshape(B, Lq, 3).float().contiguous()
        proj_in = run.proj_in.pop(run.i, None)
        if proj_in is not None and proj_in[0].data_ptr() == X.data_ptr() and tuple(proj_in[0].shape) == tuple(X.shape):
            r, ref_lvl, inside = proj_in[1]      # projected by the previous layer's triangulation launch (same arithmetic)
        else:
            r, ref_lvl, inside = ops.project(X, ctx.cams, ctx.levels, V, B, live=ctx.live)
        qt = tgt if query_tgt is None else query_tgt
        x = lambda: self.with_pos_embed(qt.float(), None if query_pos is None else query_pos.float()).contiguous()
        if (query_pos is not None and qt.dtype == torch.float32 and query_pos.dtype == torch.float32 and qt.is_contiguous()
                and query_pos.is_contiguous() and query_pos.shape == qt.shape):
            x.parts = (qt, query_pos)          # lets the fast path fold the add into the query-term GEMM
        xw_in = run.xw_in.pop(run.i, None)     # query term computed by the previous layer's chain B (or None)
        if xw_in is not None and (tuple(xw_in.shape) != (B * Lq, 192) or query_tgt is not None):
            xw_in = None                        # (computed from tgt + query_pos: not this layer's query)
        if ctx.packed_event is not None and not self.proj_attn.products.pending(self.proj_attn):
            # this layer's pyramid products run inline on THIS stream (no side-stream launch reached it) while the pyramid was packed
            # on the side stream (DQDecoder.pack_pyramid): order the read behind the pack and keep the allocator informed
            torch.cuda.current_stream().wait_event(ctx.packed_event)
            ctx.feat.record_stream(torch.cuda.current_stream())
        # processing order of the pairs, shared by the sampler (L1 locality, masked pairs skipped or zero-filled) and what reads its
        # output (all-masked tiles skipped); a G-sampler on its own bins for itself (ProjAttn.native_sample)
        order = None
        if plan.chain_a is not None or plan.skip_masked:
            if plan.binning == "first":         # binned once per forward; a layer called without a run bins per call
                order = run.order
                if order is None or order.numel() != V * B * Lq:
                    order = ops.bin_pairs(ref_lvl, None, ctx.levels)
                    if run is not _NO_RUN:
                        run.order = order
            elif plan.binning:
                order = ops.bin_pairs(ref_lvl, inside.view(-1), ctx.levels)
        if plan.chain_a is not None:
            samp = self.proj_attn.native_sample(x, ref_lvl, ctx.feat, ctx.levels, V, B, pair_mask=inside.view(-1), order=order,
                                                xw=xw_in, operands=(plan.sampler, w.sampler))
            chain_a = ops.chain_attn_pose_f32h if plan.chain_a == "f32h" else ops.chain_attn_pose
            attn, o = chain_a(samp, inside.view(-1), *w.chain_a, order=order, o_masked=w.o_masked)
        else:
            # reference arithmetic: the per-view output projection and pose MLP; with plan.skip_masked over the pairs in processing
            # order, without the tiles whose pairs are all outside their image (their rows are zero / a cached constant either way)
            attn = self.proj_attn.native_forward(x(), ref_lvl, ctx.feat, ctx.levels, V, B, rowmask=inside.view(-1), order=order)

        # 2.+3. update the query features (update_feature 'MLP', dq_decoder.py:763-778 + forward_ffn),
        #       class head + filter (dq_decoder.py:889-908)
        forced = self._forced_queries(indices, B, NQ, tgt.device)
        tgt32 = tgt.float().reshape(B * Lq, C).contiguous()
        if plan.chain_b is not None:
            tgt_out, flag, _ = run.outputs()
            next_proj = self._next_query_term(run.next_layer(), plan.chain_b, tgt, query_pos, ctx.levels)
            if plan.chain_b == "f32h":
                res = ops.chain_update_ffn_class_f32h(
                    attn, V, tgt32, *w.chain_b, threshold, B, NQ, J, forced, self.open_forward_ffn,
                    tgt_out=tgt_out, any_valid=flag, next_query_proj=next_proj, live=ctx.live)
            else:
                res = ops.chain_update_ffn_class(
                    attn, V, tgt32, *w.chain_b, threshold, B, NQ, J, forced, self.open_forward_ffn,
                    tgt_out=tgt_out, any_valid=flag, next_query_proj=next_proj,
                    attn_inside=inside.view(-1) if plan.chain_a == "bf16" else None,   # chain A wrote zeros for the pairs outside their image
                    live=ctx.live)
            tgt_update, prob, valid, any_valid = res[:4]
            if next_proj is not None:
                run.xw_in[run.i + 1] = res[4]
        else:
            Wu, bu, g2, b2, W1, b1, W2, bb2, g3, b3, Wc, bc = w.chain_b
            u = ops.linear(ops.mean_views(attn, V, live=ctx.live), Wu, bu, out_dtype=dt)
            tgt_update = ops.add_layernorm(tgt32, u, g2, b2)
            if self.open_forward_ffn:
                h = ops.linear(tgt_update, W1, b1, out_dtype=dt, relu=True)
                tgt_update = ops.add_layernorm(tgt_update, ops.linear(h, W2, bb2, out_dtype=dt), g3, b3)
            prob, valid, any_valid = ops.class_head(tgt_update, Wc, bc, threshold, B, NQ, J, forced)
        # 4. 2D offsets from the per-view attention features (calculate_2d_offsets, dq_decoder.py:659-717)
        if plan.chain_a is None:
            hcur = attn
            for i in range(len(w.pose) // 2 - 1):
                Wi, bi = w.pose[2 * i:2 * i + 2]
                if plan.skip_masked:
                    hcur = ops.linear_ordered(hcur, Wi, bi, order, inside.view(-1), w.masked_rows[i], relu=True)
                else:
                    hcur = ops.linear(hcur, Wi, bi, out_dtype=dt, relu=True)
            o = ops.rowdot3(hcur, *w.pose[-2:])

        hook = run.after_chain_b.pop(run.i, None)
        if hook is not None:
            hook()      # just-in-time schedule: the next layer's pyramid products run next to this layer's triangulation + the binning
        return dict(r=r, o=o, valid=valid, any_valid=any_valid, tgt_update=tgt_update.view(B, Lq, C), prob=prob,
                    dims=(V, B, NQ, J))

    def forward_triangulate(self, st, ctx):
        """step 5: triangulation + scatter (learnable_triangulate, dq_decoder.py:399-461,1013-1029)."""
        V, B, NQ, J = st["dims"]
        run = self._run or _NO_RUN
        boundary = self.fuse_boundary and run.next_layer() is not None     # the next layer's projection of the new points rides on this launch
        new_ref, ref2d, proj2d, *proj = ops.triangulate(st["r"], st["o"], ctx.cams, st["valid"], st["any_valid"], V, B, NQ, J,
                                                        out=run.outputs()[2], next_levels=ctx.levels if boundary else None,
                                                        live=ctx.live)
        if boundary:
            run.proj_in[run.i + 1] = (new_ref, proj[0])
        return st["tgt_update"], new_ref, ref2d, proj2d, st["prob"]


class MvPDecoder(nn.Module):
    """mvp_decoder.py:267-298 (constructor + coordinate helpers)."""

    def __init__(self, cfg, decoder_layer, num_layers, return_intermediate=False):
        super().__init__()
        if cfg.DECODER.share_layer_weights:
            self.layers = nn.ModuleList([decoder_layer for _ in range(num_layers)])
        else:
            self.layers = _get_clones(decoder_layer, num_layers)
        self.num_layers = num_layers
        self.return_intermediate = return_intermediate
        self.pose_embed = None
        self.class_embed = None
        self.grid_size = torch.tensor(cfg.MULTI_PERSON.SPACE_SIZE)
        self.grid_center = torch.tensor(cfg.MULTI_PERSON.SPACE_CENTER)

    def absolute2norm(self, absolute_coords):
        device = absolute_coords.device
        grid_size = self.grid_size.to(device=device)
        grid_center = self.grid_center.to(device=device)
        return (absolute_coords - grid_center + grid_size / 2.0) / grid_size

    def norm2absolute(self, norm_coords):
        device = norm_coords.device
        grid_size = self.grid_size.to(device=device)
        grid_center = self.grid_center.to(device=device)
        return norm_coords * grid_size + grid_center - grid_size / 2.0


class DQDecoder(MvPDecoder):
    """dq_decoder.py:1101-1172.  (The reference indexes a 4-entry meter list by layer id,
    dq_decoder.py:94,1142, and therefore crashes with more than 4 layers; not inherited.)"""

    def __init__(self, cfg, decoder_layer, num_layers, return_intermediate=False):
        super().__init__(cfg, decoder_layer, num_layers, return_intermediate)
        # The pyramid-side GEMMs of every layer (value planes + G, 73 us per layer) depend only on the packed
        # feature maps: issue all of them on a side stream at the start of the forward (fork/join -> a parallel
        # branch of the captured HIP graph).  They fill in next to the latency-bound query-side kernels:
        # cfg-2 bf16 1.43 -> 1.30 ms per sample on MI355X.  MVG_OVERLAP_PYRAMID=0 runs them inline.
        self.overlap_pyramid = os.environ.get("MVG_OVERLAP_PYRAMID", "1") != "0"
        self.overlap_pyramid_f32 = os.environ.get("MVG_OVERLAP_PYRAMID_F32", "1") != "0"
        # ONE owner of the layers' product buffers, their ready state and the side stream (a deep copy of the decoder shares a fresh one)
        self.products = PyramidProducts()
        for layer in self.layers:
            layer.proj_attn.products = self.products
        # layer l's fused chain B also computes layer l+1's query term xw = (tgt' + query_pos) W^T + b (bf16 path)
        self.fuse_next_query_term = True
        # bf16: layers per grouped launch of the pyramid products behind layer 0's own (0 = one launch per product, rounds 1-4)
        self.pyramid_group = int(os.environ.get("MVG_PYRAMID_GROUP", "3"))
        # pack the pyramid on the side stream in front of its consumers: the first layer's query-side prologue (projection, pair
        # binning, query term) then runs next to the pack instead of behind it
        self.pack_on_side = os.environ.get("MVG_PACK_ON_SIDE", "1") != "0"
        # bf16, one sample per forward: layer l+1's products (one launch, ONE workgroup per CU) are issued behind layer l's chain B, next
        # to its triangulation and the next binning, instead of all up front -- the sampler then finds them in the 256-MB Infinity
        # Cache (137 -> 128 us) and the first sampler has the chip to itself: -2.8 ... -3.1 % at cfg-2, -2 % at cfg-5, +2 % at two samples
        # per forward (profiles/r05_experiments.txt section 10).  MVG_PYRAMID_JIT = 0 | 1 overrides the choice.
        self.pyramid_jit = os.environ.get("MVG_PYRAMID_JIT", "auto")
        self.pyramid_jit_slots = int(os.environ.get("MVG_PYRAMID_JIT_SLOTS", "32"))

    def set_compute_dtype(self, dtype):
        for layer in self.layers:
            layer.set_compute_dtype(dtype)
        return self

    def set_training_dtype(self, dtype):
        """DQDecoderLayer.set_training_dtype on every layer (float32 default, or bfloat16 mixed precision for the autograd path;
        torch.autocast is not consulted)"""
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("training dtype must be float32 or bfloat16")
        for layer in self.layers:
            layer.set_training_dtype(dtype)
        return self

    def set_self_attention_training(self, backend):
        """DQDecoderLayer.set_self_attention_training on every layer ("torch" default, or "native": the init_self_attention
        block's training on the HIP attention kernels)"""
        if backend not in ("torch", "native"):
            raise ValueError("self-attention training backend must be 'torch' or 'native'")
        for layer in self.layers:
            layer.set_self_attention_training(backend)
        return self

    def fork_side_stream(self, device, f32_shape=None):
        """The side stream of the forward, forked from the current stream -- or None when the query-independent work
        runs inline (generic path, share_layer_weights -- one buffer for all layers --, training, CPU,
        MVG_OVERLAP_PYRAMID=0).  f32_shape = (Lq, L, S): needed for the fp32 path, whose pyramid products exist only in its
        G-sampling forms (ProjAttn.sampler_form)."""
        distinct = len({id(l.proj_attn) for l in self.layers}) == len(self.layers)
        shape = f32_shape or (None, None, None)

        def ahead(l):
            dt = l.compute_dtype
            if dt == torch.float32 and not (self.overlap_pyramid_f32 and f32_shape is not None):
                return False
            return l.plan(dt, shape[0], shape[1:]).products_ahead
        if not (self.overlap_pyramid and distinct and device.type == "cuda" and not torch.is_grad_enabled()
                and all(ahead(l) for l in self.layers)):
            return None
        if not torch.cuda.is_current_stream_capturing():
            for l in self.layers:   # cached operands are built here, on the forking stream, never on the side stream
                l.prepare_caches()
        return self.products.fork()

    def launch_pyramid_projections(self, ctx, side=None, forked=False, jit=False):
        """Issue every layer's query-independent GEMMs (ProjAttn.project_pyramid) on the side stream, each followed
        by an event its consumer waits on.  Returns the side stream (pass it to join_pyramid_projections before
        the forward / the captured graph ends) or None when the projections run inline.  forked: `side` already waits for
        whatever produced ctx.feat (pack_pyramid).  jit: the caller runs the whole forward inside ONE fork / join of `side` (not the
        segmented graphs of mvgformer_amd.dist) -- the just-in-time schedule may be used; its hooks go into the layers' DecoderRun."""
        if side is None:
            side = self.fork_side_stream(ctx.feat.device)
            if side is None:
                return None
        elif not forked:
            side.wait_stream(torch.cuda.current_stream())       # the packed pyramid
        ctx.feat.record_stream(side)
        with torch.cuda.stream(side):
            launches = self.pyramid_launches(ctx, jit)
            if launches is None:
                for layer in self.layers:
                    layer.proj_attn.project_pyramid(ctx.feat, record_event=True)
            else:
                # bf16 fast path: layer 0's value planes + G in one launch (the first sampler waits for nothing else), then the
                # remaining layers' products in launches of `pyramid_group` layers: every launch reads the pyramid through the
                # fabric once (ops.pyramid_group_ws); 8 reads of 103 MB per forward at cfg-2 become 2.  These launches fill every
                # CU (2 x 246 registers per SIMD lane) and so does the sampler: next to each other they run one after the other,
                # whatever the issue order -- issuing a group behind the sampler in front of it, or with half the workgroups,
                # measured slower (profiles/r05_experiments.txt section 2).  What does pay (section 10): one launch per layer with ONE
                # workgroup per CU, issued behind the previous layer's chain B (use_jit below).
                use_jit = self._pyramid_jit(ctx, jit)
                for gi, (group, slots) in enumerate(launches):
                    def issue(group=group, slots=slots):
                        jobs = []
                        for layer in group:
                            jobs += layer.proj_attn.pyramid_jobs(ctx.feat)
                        ops.pyramid_group_ws(ctx.feat, jobs, slots=slots)
                        self.products.produced([layer.proj_attn for layer in group])
                    if use_jit and gi > 0:
                        def hook(issue=issue):
                            side.wait_stream(torch.cuda.current_stream())     # behind the previous layer's chain B
                            with torch.cuda.stream(side):
                                issue()
                        self.layers[0]._run.after_chain_b[gi - 1] = hook
                    else:
                        issue()
        return side

    def pack_pyramid(self, ctx, src_views, side):
        """ctx.pack(src_views) -- on the side stream (forked from the current one) when every consumer of the packed pyramid runs
        there (bf16: the pyramid products), so that the first layer's prologue does not queue behind the 46-us pack; follow it
        with launch_pyramid_projections(ctx, side, forked=True)."""
        ctx.packed_event = None
        if side is not None and self.pack_on_side and ctx.dtype == torch.bfloat16:
            with torch.cuda.stream(side):
                ctx.pack(src_views)
                # a consumer on ANOTHER stream (ProjAttn.native_sample's inline products, when a layer's just-in-time hook did not
                # fire) waits on this event; ctx.feat was allocated on `side`
                ctx.packed_event = torch.cuda.Event()
                ctx.packed_event.record()
        else:
            ctx.pack(src_views)
            if side is not None:
                side.wait_stream(torch.cuda.current_stream())

    def _pyramid_jit(self, ctx, jit=True):
        """True when a forward of this context issues one product launch per layer, just in time (launch_pyramid_projections)"""
        return bool(jit and len(self.layers) > 1 and (self.pyramid_jit == "1" or (self.pyramid_jit == "auto" and ctx.B == 1)))

    def pyramid_launches(self, ctx, jit=True):
        """[(layers, workgroups per XCD; 0 = the kernel's default)]: the product launches of one forward in issue order
        (bf16 fast path; None otherwise)"""
        groups = self._pyramid_groups(ctx)
        if groups is None:
            return None
        if self._pyramid_jit(ctx, jit):
            # (layer 0's launch too: with two workgroups per CU it starved the first layer's binning + query-term GEMM, which run next
            # to it -- bin_scatter 57 us instead of 11, the first sampler at 142 us instead of 127: forward -0.9 %)
            return [([l], self.pyramid_jit_slots) for l in self.layers]
        return [(g, 0) for g in groups]

    def _pyramid_groups(self, ctx):
        """layers whose pyramid products share one launch (bf16 fast path), or None for one launch pair per layer"""
        if self.pyramid_group <= 0 or ctx.feat.dtype != torch.bfloat16 or ctx.feat.shape[2] != 256:
            return None
        if not all(l.plan(torch.bfloat16).grouped for l in self.layers):
            return None
        layers = list(self.layers)
        groups = [layers[:1]]
        rest = layers[1:]
        per = min(self.pyramid_group, 4)            # 2 jobs per layer, at most 8 per launch
        while rest:
            # equal-sized launches: 5 remaining layers at 3 per launch run as 3 + 2
            n = -(-len(rest) // -(-len(rest) // per))
            groups.append(rest[:n])
            rest = rest[n:]
        return groups

    def join_pyramid_projections(self, side, keep_results=False):
        """The current stream waits for the side stream.  keep_results: projections not consumed yet stay valid for
        the layers that follow on this stream (the segmented graphs of mvgformer_amd.dist); else they are dropped."""
        self.products.join(side, keep_results)

    def forward(self, tgt, reference_points, src_views, meta, src_spatial_shapes, src_level_start_index,
                src_valid_ratios, query_pos=None, src_padding_mask=None, rgb_views=None, output_dir="./",
                frame_id=None, indices=None, threshold=0.5, indices_all=None, context=None, view_live=None):
        """Returns (hs (layers,B,Lq,C), refs (layers,B,Lq,3), refs2d (layers,B,V,Lq,2),
        projs2d (layers,B,V,Lq,2), [class_prob (B,NQ,2)] * layers) when return_intermediate,
        else (output, reference_points, ref_points_2d).  ``context`` (optional, beyond the reference
        signature): a DecoderContext.prepare(...)d context, so the host-side camera packing is
        hoisted out of a captured HIP graph.  ``view_live`` (optional, beyond the reference signature): the mask of
        DecoderContext.set_live_views, set on the context of this call -- the outputs are, bit for bit, those of a run on the live
        views alone, with zeros in the 2D slots of the others; None leaves a given context's table as it is."""
        if tgt.is_cuda and tgt.device.index != torch.cuda.current_device():
            with torch.cuda.device(tgt.device):     # kernels go to the current stream of the TENSORS' device
                return self.forward(tgt, reference_points, src_views, meta, src_spatial_shapes, src_level_start_index,
                                    src_valid_ratios, query_pos, src_padding_mask, rgb_views, output_dir, frame_id, indices,
                                    threshold, indices_all, context, view_live)
        output = tgt
        layer0 = self.layers[0]
        ctx = context
        side = None
        try:
            deferred_pack = None
            if ctx is None:
                ctx = DecoderContext.prepare(src_spatial_shapes, src_level_start_index, meta, layer0.img_size,
                                             layer0.compute_dtype, tgt.shape[0], src_views[0].device)
                deferred_pack = src_views
            elif src_views is not None:
                # a prepared context is reused across frames (static cameras): the pyramid is re-packed from THIS
                # call's src_views every time (a no-op for levels produced in place in ctx.pyramid_buffers())
                deferred_pack = src_views
            elif ctx.feat is None:
                raise RuntimeError("DQDecoder.forward: context without a packed pyramid and no src_views")
            if view_live is not None:
                ctx.set_live_views(view_live)
            if ctx.live is not None:
                if not tgt.is_cuda:
                    raise NotImplementedError("DQDecoder.forward: a live-view table needs the HIP path")
                # (a later layer's input requires grad exactly when some layer before it took the autograd path or tgt does)
                if any(layer.takes_autograd_path(tgt) for layer in self.layers):
                    refuse_live_views(ctx, "DQDecoder.forward (the layers' forward_autograd)")      # before the pack: no launch
            inter, inter_ref, inter_2d, inter_proj, classes = [], [], [], [], []
            ref_points_2d = None
            with DecoderRun(self.layers, ctx, self.fuse_next_query_term) as run:
                side = self.fork_side_stream(tgt.device, (tgt.shape[1], ctx.levels.L, ctx.levels.S))
                if deferred_pack is not None:
                    self.pack_pyramid(ctx, deferred_pack, side)
                if side is not None:
                    self.launch_pyramid_projections(ctx, side, forked=True, jit=True)
                # the fused chain writes every layer's hidden state straight into its slice of the stacked output
                if self.return_intermediate and not torch.is_grad_enabled() and tgt.is_cuda:
                    run.hs_buf = torch.empty((len(self.layers),) + tuple(tgt.shape), dtype=torch.float32, device=tgt.device)
                if tgt.is_cuda:
                    run.flags = torch.zeros((len(self.layers),), dtype=torch.int32, device=tgt.device)
                if run.hs_buf is not None:
                    nl, Bq, Lq_, Vn = len(self.layers), tgt.shape[0], tgt.shape[1], ctx.V
                    run.geo_buf = (torch.empty((nl, Bq, Lq_, 3), dtype=torch.float32, device=tgt.device),
                                   torch.empty((nl, Bq, Vn, Lq_, 2), dtype=torch.float32, device=tgt.device),
                                   torch.empty((nl, Bq, Vn, Lq_, 2), dtype=torch.float32, device=tgt.device))
                for lid, layer in enumerate(self.layers):
                    run.i = lid
                    output, reference_points, ref_points_2d, projs_2d_absolute, outputs_class = layer(
                        output, query_pos, reference_points[:, :, None] if reference_points.dim() == 3 else reference_points,
                        src_views, src_spatial_shapes, src_level_start_index, meta, src_padding_mask,
                        rgb_views=rgb_views, output_dir=output_dir, frame_id=frame_id, indices=indices,
                        threshold=threshold, indices_all=indices_all)
                    if self.return_intermediate:
                        inter.append(output)
                        inter_ref.append(reference_points)
                        inter_2d.append(ref_points_2d)
                        inter_proj.append(projs_2d_absolute)
                        classes.append(outputs_class)
        finally:
            self.join_pyramid_projections(side)
        if self.return_intermediate:
            def stacked(parts, buf):
                same = buf is not None and all(t.data_ptr() == buf[i].data_ptr() and t.shape == buf[i].shape
                                               for i, t in enumerate(parts))
                return buf if same else torch.stack(parts)
            geo_buf = run.geo_buf or (None, None, None)
            return (stacked(inter, run.hs_buf), stacked(inter_ref, geo_buf[0]), stacked(inter_2d, geo_buf[1]),
                    stacked(inter_proj, geo_buf[2]), classes)
        return output, reference_points, ref_points_2d


# north_star aliases
MultiViewDecoderLayer = DQDecoderLayer
MultiViewDecoder = DQDecoder
