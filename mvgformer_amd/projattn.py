"""ProjAttn -- projective attention module.  Same constructor, parameters, state-dict keys and
forward signature as the reference (lib/models/ops/modules/projattn.py:42-204); the compute
runs on libmvgformer_hip.so.

Two execution paths, both GPU-only (no CPU fallback):
  * inference (autograd off): gather -> MFMA linears -> fused softmax+locations+sampling
    kernel -> MFMA output projection.  Locations / attention weights never touch HBM.
  * training (autograd on): the reference's op chain with torch autograd for the dense parts
    and DeformFunction (HIP forward + backward kernels) for the sampling.
"""
from __future__ import annotations

import math
import warnings

import os

import torch
import torch.nn.functional as F
from torch import nn
from torch.nn.init import constant_, xavier_uniform_

from . import ops
from .functions import DeformFunction


def ops_host_levels_pair(spatial_shapes, level_start_index):
    """(shapes, starts) as host lists, through ops.host_levels' per-tensor cache (no D2H sync after the first look-up)"""
    sc, st = ops.host_levels(spatial_shapes, level_start_index)
    return [[sc[2 * i], sc[2 * i + 1]] for i in range(len(st))], list(st)


def f32_split_on():
    """the library's f32_split knob selects the split fp32 GEMMs (default); 0 (bench.py --f32-gemm exact): reference arithmetic"""
    from . import _lib
    _lib.load()         # fills TUNING and applies MVG_TUNE
    return _lib.TUNING["f32_split"] != 0


def _is_power_of_2(n):
    if (not isinstance(n, int)) or (n < 0):
        raise ValueError("invalid input for _is_power_of_2: {} (type: {})".format(n, type(n)))
    return (n & (n - 1) == 0) and n != 0



class WeightCache:
    """Contiguous copies of module parameters in the compute dtype, rebuilt when a parameter
    is modified in place (``_version``) or replaced."""

    def __init__(self):
        self._store = {}
        self._adopted = {}      # key -> (params, dtype, tensor): entries somebody else keeps up to date (adopt)

    def __deepcopy__(self, memo):
        """adopted entries do not travel with a copy: the buffer belongs to whoever maintains it for the ORIGINAL's parameters (a
        graph may address it); everything else is copied as before"""
        import copy
        new = WeightCache()
        new._store = copy.deepcopy({k: v for k, v in self._store.items() if k not in self._adopted}, memo)
        return new

    def adopt(self, key, params, dtype, tensor):
        """Hand the cache a persistent tensor for `key`, current for `params` as they are now: get() returns THIS tensor while the
        stamp holds.  Whoever rewrites it on the device after the parameters changed (training.TrainOperands, behind the optimizer's
        update kernel) calls restamp().  If the stamp is found stale all the same (a checkpoint load, another optimizer), get()
        rebuilds the entry as usual but INTO the adopted tensor, so its address -- which a captured graph may hold -- stays."""
        params = tuple(params)
        self._adopted[key] = (params, dtype, tensor)
        self._store[key] = (self._stamp(params, dtype), tensor)

    def restamp(self):
        """the adopted entries are current for their parameters' present versions"""
        for key, (params, dtype, tensor) in self._adopted.items():
            self._store[key] = (self._stamp(params, dtype), tensor)

    @staticmethod
    def _stamp(params, dtype):
        return tuple((id(p), p._version, p.device) for p in params) + (dtype,)

    def get(self, key, params, dtype, build=None, sync=True):
        """sync=False: the entry is only read on the stream that builds it (the training path), no wait for the build"""
        stamp = self._stamp(params, dtype)
        hit = self._store.get(key)
        if hit is not None and hit[0] == stamp:
            return hit[1]
        if any(p.is_cuda for p in params) and torch.cuda.is_current_stream_capturing():
            # An entry built inside a capture would sit in the graph's private pool, stamped valid but unwritten until
            # the first replay: an eager forward before that replay (or after the parameters were restored) would read
            # garbage without any error.  Operands are built ahead of a capture: DQDecoderLayer.prepare_caches().
            raise RuntimeError("WeightCache: %r is not cached for the current parameters and a HIP-graph capture is in "
                               "progress; call DQDecoderLayer.prepare_caches() (or run one eager forward with the same "
                               "dtype and weights) before capturing" % key)
        with torch.no_grad():
            t = build(*params) if build is not None else params[0]
            extra = ()
            if isinstance(t, tuple):      # (tensor, host-side scalars ...): e.g. an operand and its power-of-two scale
                t, extra = t[0], tuple(t[1:])
            t = t.detach().to(dtype).contiguous()
            mine = self._adopted.get(key)
            if mine is not None:
                if (len(mine[0]) == len(params) and all(a is b for a, b in zip(mine[0], params)) and mine[1] == dtype
                        and mine[2].shape == t.shape and mine[2].device == t.device):
                    mine[2].copy_(t)
                    t = mine[2]
                else:           # other parameters, dtype or shape under this key: the adoption is over
                    del self._adopted[key]
        # An entry is built on whatever stream is current and then handed out to every stream (the decoder issues
        # query-independent work on a side stream): finish the build before anybody can see the entry.  Rare (first
        # use / parameters changed).
        if t.is_cuda and sync:
            torch.cuda.current_stream(t.device).synchronize()
        out = (t,) + extra if extra else t
        self._store[key] = (stamp, out)
        return out

    def tensors(self):
        """the cached operand tensors (what a captured graph addresses and does not own)"""
        return [t for _, out in self._store.values() for t in (out if isinstance(out, tuple) else (out,)) if torch.is_tensor(t)]


class PyramidProducts:
    """The per-layer pyramid products (value planes and G) of ONE decoder: where they live, whether they are ready, and the side
    stream that makes them ahead of their layers.  DQDecoder creates one and hands it to every layer's ProjAttn; a ProjAttn used on
    its own has a private one.  Run-time state only: a deep copy is a fresh, empty instance (one per copied decoder, through the memo).
    Buffers are kept across calls -- the same key and shape return the same tensors, so nothing is allocated inside a graph capture
    after the warm-up forwards -- in two tables that never share a tensor:
      per layer    bf16 planes (n_img, 8, S, 32) + G (n_img*S, 192), and the fp32 pair (n_img, S, C) + (n_img*S, 192) made AHEAD on
                   the side stream, where every layer's products are alive at once
      per stream   the fp32 pair made INLINE: a layer's products are dead once its sampler ran and the next layer's are written
                   behind it on the same stream -> one pair per (device, stream) for all layers (0.36 GB at cfg-2 instead of 0.36 GB
                   per layer); streams do not share (decoders in flight)
    Ready state of a layer's products: not produced (absent), produced (the event its consumer waits on) or joined (None: the
    consumer's stream has waited for the side stream already)."""

    def __init__(self):
        self._per_layer, self._per_stream, self._ready, self._side = {}, {}, {}, None

    def __deepcopy__(self, memo):
        return PyramidProducts()

    def buffers(self, proj_attn, dtype, n_img, S, C, device, ahead=False, stream=None):
        """(value, G) for one layer's products, allocated or reused.  ahead: made on the side stream (read by the fp32 form alone);
        stream: the key of the inline fp32 pair (default: the current stream of `device`)"""
        if dtype == torch.float32 and not ahead:
            table, key = self._per_stream, (device, torch.cuda.current_stream(device).cuda_stream if stream is None else stream)
        else:
            table, key = self._per_layer, proj_attn
        shape = (n_img, 8, S, 32) if dtype == torch.bfloat16 else (n_img, S, C)
        pair = table.get(key)
        if pair is None or pair[0].dtype != dtype or tuple(pair[0].shape) != shape or pair[0].device != device:
            pair = table[key] = (torch.empty(shape, dtype=dtype, device=device), torch.empty((n_img * S, 192), dtype=dtype, device=device))
        return pair

    def produced(self, proj_attns, event=None):
        """these layers' products are written behind `event` (None: recorded here, on the current stream) into their per-layer buffers"""
        if event is None:
            event = torch.cuda.Event()
            event.record()
        for pa in proj_attns:
            self._ready[pa] = event

    def take(self, proj_attn):
        """(value, G) made ahead for this layer, behind a wait on their event where the stream has not joined yet -- the state stays
        until join() --; None: the layer computes them inline"""
        if proj_attn not in self._ready:
            return None
        event = self._ready[proj_attn]
        if event is not None:
            event.wait()        # the current stream
        return self._per_layer[proj_attn]

    def join(self, side=None, keep=False):
        """The current stream waits for the side stream.  keep: products not consumed yet stay valid, without a further wait, for the
        layers that follow on this stream (the segmented graphs of mvgformer_amd.dist); else they are dropped."""
        if side is not None:
            torch.cuda.current_stream().wait_stream(side)
        self._ready = dict.fromkeys(self._ready) if keep else {}

    def pending(self, proj_attn=None):
        """this layer's (None: some layer's) products are produced or joined, and not dropped yet"""
        return bool(self._ready) if proj_attn is None else proj_attn in self._ready

    def fork(self):
        """the side stream (created on first use), waiting for the current one"""
        if self._side is None:
            self._side = torch.cuda.Stream()
        self._side.wait_stream(torch.cuda.current_stream())
        return self._side

    def tensors(self):
        """every live buffer, once (what a captured graph addresses and does not own)"""
        return [t for table in (self._per_layer, self._per_stream) for pair in table.values() for t in pair]

    def signature(self):
        """(pointer, dtype, shape) of every buffer: changes exactly when one is added or replaced"""
        return tuple((t.data_ptr(), t.dtype, tuple(t.shape)) for t in self.tensors())


class ProjAttn(nn.Module):
    def __init__(self, d_model=256, n_levels=4, n_heads=8, n_points=4, projattn_posembed_mode="use_rayconv"):
        super().__init__()
        if d_model % n_heads != 0:
            raise ValueError("d_model must be divisible by n_heads, but got {} and {}".format(d_model, n_heads))
        if not _is_power_of_2(d_model // n_heads):
            warnings.warn("d_model // n_heads should be a power of 2 (the HIP kernels vectorise over head channels)")
        self.im2col_step = 64
        self.d_model = d_model
        self.n_levels = n_levels
        self.n_heads = n_heads
        self.n_points = n_points
        self.sampling_offsets = nn.Linear(d_model, n_heads * n_levels * n_points * 2)
        self.attention_weights = nn.Linear(d_model, n_heads * n_levels * n_points)
        if projattn_posembed_mode == "use_rayconv":
            self.rayconv = nn.Linear(d_model + 3, d_model)
        elif projattn_posembed_mode == "use_2d_coordconv":
            self.rayconv = nn.Linear(d_model + 2, d_model)
        elif projattn_posembed_mode == "ablation_not_use_rayconv":
            self.rayconv = nn.Linear(d_model, d_model)
        else:
            raise ValueError("invalid projective attention posembed mode")
        self.output_proj = nn.Linear(d_model, d_model)
        self._reset_parameters()
        self.projattn_posembed_mode = projattn_posembed_mode
        self.compute_dtype = torch.float32
        # bf16 inference: weight-stationary pyramid GEMMs + head-plane value layout + G-sampling kernel
        # (False: the generic gather -> linear -> fused-sampling kernels, also the fp32 path)
        self.use_fast_path = True
        # bf16 fast path: sample the pairs in image-space (Morton) order.  "layer"/True: binned per layer; "first":
        # DQDecoderLayer bins once per forward (first layer) and reuses the order; False: query order
        # fp32 path: G-sampling (csrc/msda.hip: msda_gfused_f32_kernel) instead of gather -> Linear -> fused sampling.
        # True / False, or "auto": wherever the offsets / logits Linear has fewer rows on the pyramid (V*S) than on the
        # gathered reference points (V*Lq*L) -- cfg-2: 40 320 vs 46 080 rows per image, 6.80 -> 6.26 ms; cfg-4 (512 queries:
        # 39 900 vs 23 040) and a rank's shard of a query-sharded run keep the gather form.  The two forms agree to fp32
        # rounding, not bit for bit: pin it to True / False where runs with different query counts must match exactly.
        self.g_sampling_f32 = {"0": False, "1": True}.get(os.environ.get("MVG_G_SAMPLING_F32", "auto"), "auto")
        # training path: reference-point features through the HIP sampling op (False: torch grid_sample per level)
        self.ref_gather_native = os.environ.get("MVG_REF_GATHER", "1") != "0"
        # fp32 path: fused kernels on pre-split operands (csrc/f32s.hip): one-pass pyramid products here, chain A / chain B in
        # DQDecoderLayer.  MVG_F32_FUSED=0: the unfused kernels of rounds 1-3 (mvg_linear per GEMM).
        self.f32_fused = os.environ.get("MVG_F32_FUSED", "1") != "0"
        self.sort_pairs = os.environ.get("MVG_SORT_PAIRS", "layer")
        if self.sort_pairs in ("0", "off", "False"):
            self.sort_pairs = False
        self._wc = WeightCache()
        # precision of the autograd path (the layer's set_training_dtype): float32, or bfloat16 operands with fp32 accumulation
        self.training_dtype = torch.float32
        self.products = PyramidProducts()   # buffers and ready state of the pyramid products; DQDecoder hands its layers a common one

    def _reset_parameters(self):
        constant_(self.sampling_offsets.weight.data, 0.)
        thetas = torch.arange(self.n_heads, dtype=torch.float32) * (2.0 * math.pi / self.n_heads)
        grid_init = torch.stack([thetas.cos(), thetas.sin()], -1)
        grid_init = (grid_init / grid_init.abs().max(-1, keepdim=True)[0]).view(self.n_heads, 1, 1, 2) \
            .repeat(1, self.n_levels, self.n_points, 1)
        for i in range(self.n_points):
            grid_init[:, :, i, :] *= i + 1
        with torch.no_grad():
            self.sampling_offsets.bias = nn.Parameter(grid_init.view(-1))
        constant_(self.attention_weights.weight.data, 0.)
        constant_(self.attention_weights.bias.data, 0.)
        xavier_uniform_(self.rayconv.weight.data)
        constant_(self.rayconv.bias.data, 0.)
        xavier_uniform_(self.output_proj.weight.data)
        constant_(self.output_proj.bias.data, 0.)

    # ------------------------------------------------------------------ native building blocks
    def fused_supported(self, feat_lvls):
        return (self.projattn_posembed_mode == "ablation_not_use_rayconv" and self.d_model == 256 and
                self.n_heads == 8 and self.n_points == 8 and self.n_levels == 1 and 1 <= feat_lvls <= 4)

    @property
    def g_geometry(self):
        """what every G-sampling kernel and every operand of that form is built for: 192 [offsets; logits] rows on 256 channels"""
        return (3 * self.n_heads * self.n_levels * self.n_points == 192 and self.d_model == 256
                and self.projattn_posembed_mode == "ablation_not_use_rayconv")      # (rayconv is 256 -> 256 in that mode alone)

    def uses_fast_path(self, dt):
        return dt == torch.bfloat16 and bool(self.use_fast_path) and self.g_geometry

    def f32_fused_active(self):
        """the fused fp32 kernels on split operands (csrc/f32s.hip) are in use: MVG_F32_FUSED and the library's f32_split knob
        (bench.py --f32-gemm exact, mvg_set_tuning("f32_split", 0)) both select them; with either off the fp32 path is the
        reference-arithmetic decomposition (fmaf-chain GEMMs, one launch each)"""
        return self.g_geometry and bool(self.f32_fused) and f32_split_on()

    def f32_g_form(self, Lq, L, S):
        """fp32 path: G-sampling (the offsets / logits Linear applied to the pyramid) rather than gather-then-Linear -- by
        MVG_G_SAMPLING_F32, else whenever the gathered rows (Lq * L per image) outnumber the pyramid's (S)"""
        if self.g_sampling_f32 != "auto":
            return bool(self.g_sampling_f32) and self.g_geometry
        # with the one-pass pyramid kernel (mvg_pyramid_f32h) the G form moves fewer bytes at every shipped shape: the gather
        # form re-fetched 2.6 x its algorithmic bytes at cfg-4 (profiles/r03_bench_cfg4_fp32.json)
        if not self.g_geometry or self.f32_fused_active():
            return self.g_geometry
        if Lq is None or L is None or S is None:
            raise ValueError("ProjAttn.f32_g_form: g_sampling_f32='auto' without the fused fp32 kernels decides by the shape (Lq, L, S)")
        return Lq * L >= S

    def sampler_form(self, dt, Lq, L, S):
        """which sampler native_sample runs: "gsamp" (bf16 G-sampling, msda_gsamp), "gfused_f32h" / "gfused_f32" (fp32 G-sampling,
        msda_gfused_f32, on the products of mvg_pyramid_f32h / of two plain linears) or "gather" (gather + linear + msda_fused)"""
        if self.uses_fast_path(dt):
            return "gsamp"
        if dt == torch.float32 and self.f32_g_form(Lq, L, S):
            return "gfused_f32h" if self.f32_fused_active() else "gfused_f32"
        return "gather"

    def sampler_forms(self, dt):
        """every form some shape can select under the current switches"""
        if dt == torch.float32 and self.g_geometry and self.g_sampling_f32 == "auto" and not self.f32_fused_active():
            return ("gfused_f32", "gather")     # the only case in which the shape decides (f32_g_form)
        return (self.sampler_form(dt, None, None, None),)

    def weights(self, dtype):
        """(Wv, bv, W_oa, b_oa, Wp, bp): value / [offsets|logits] / output projections."""
        wc = self._wc
        cat = lambda a, b: torch.cat([a, b], 0)
        return (wc.get("Wv", (self.rayconv.weight,), dtype),
                wc.get("bv", (self.rayconv.bias,), torch.float32),
                wc.get("Woa", (self.sampling_offsets.weight, self.attention_weights.weight), dtype, cat),
                wc.get("boa", (self.sampling_offsets.bias, self.attention_weights.bias), torch.float32, cat)) + self.output_operands(dtype)[:2]

    def sampler_operands(self, form, dt, query=True):
        """every cached operand one sampler form reads (native_sample and the pyramid products in front of it):
        ([offsets; logits] weight and bias of the query side -- None with query=False --, the pyramid side's operands)"""
        wc = self._wc
        if form == "gather":
            w = self.weights(dt)
            return w[2:4], w[:2]
        bv = wc.get("bv", (self.rayconv.bias,), torch.float32)
        if form == "gsamp":     # value fragments, bias, G fragments (ops.value_proj_planes_ws / feat_linear_ws / pyramid_group_ws)
            Wv_f = wc.get("Wv_frag", (self.rayconv.weight,), dt, lambda w: ops.swizzle_weight(w.to(dt)))
            pyramid = (Wv_f, bv, self.query_term_weights(dt)[0])
        elif form == "gfused_f32h":     # bias + ((value planes, scale), (G planes, scale)) of mvg_pyramid_f32h
            pyramid = (bv,) + self.pyramid_planes_f32h()
        else:                           # two plain linears (the second on the query side's weight)
            pyramid = (wc.get("Wv", (self.rayconv.weight,), dt), bv)
        return (self._fast_query_weights(dt) if query else None), pyramid

    def output_operands(self, dt, skip_masked=False):
        """(Wp, bp, zero row): output projection of native_forward; the row of a skipped tile only where tiles are skipped"""
        wc, bias = self._wc, self.output_proj.bias
        return (wc.get("Wp", (self.output_proj.weight,), dt), wc.get("bp", (bias,), torch.float32),
                wc.get("zero_row", (bias,), torch.float32, lambda b: torch.zeros_like(b)) if skip_masked else None)

    def project_pyramid(self, feat, record_event=False):
        """The two query-independent GEMMs of a layer: value planes (projattn.py:169) and G = feat @ [Wo; Wa]^T
        (the pyramid side of projattn.py:180-181).  Neither depends on the queries, so DQDecoder runs them for
        every layer on a side stream next to the latency-bound query-side kernels (record_event=True: the
        consumer waits on the event); both land in buffers kept across calls (PyramidProducts)."""
        dt = feat.dtype
        n_img, S, Cc = feat.shape
        if dt == torch.float32:      # fp32 G-sampling form: plain (rows, 256) / (rows, 192) fp32 products
            f32h = self.f32_fused_active()
            (Wq, _), pyramid = self.sampler_operands("gfused_f32h" if f32h else "gfused_f32", dt)
            vp, G = self.products.buffers(self, dt, n_img, S, Cc, feat.device, ahead=record_event)
            if f32h:
                # two-part fp16 operands, three products (csrc/f32s.hip: pyramid_ws_f32h_kernel)
                bv, (Wv_pl, sv), (Wg_pl, sg) = pyramid
                ops.pyramid_f32h(feat, Wv_pl, sv, bv, Wg_pl, sg, 192, value=vp, G=G)   # projattn.py:169 + 180-181
            else:
                ops.linear(feat.view(n_img * S, Cc), *pyramid, out=vp.view(n_img * S, Cc))     # projattn.py:169
                ops.linear(feat.view(n_img * S, Cc), Wq, None, out=G)
        else:
            # the 103-MB value write first, G (gathered at random by the sampler) last: G is then the fresher
            # resident of the 256-MB Infinity Cache when the sampler starts
            vp = self.project_values(feat)
            G = self.products.buffers(self, dt, n_img, S, Cc, feat.device)[1]
            ops.feat_linear_ws(feat, self.sampler_operands("gsamp", dt, query=False)[1][2], 192, out=G)
        if record_event:
            self.products.produced((self,))
        return vp, G

    def pyramid_jobs(self, feat):
        """this layer's two products as jobs of ops.pyramid_group_ws (value planes, G), into the buffers project_pyramid uses"""
        n_img, S, Cc = feat.shape
        Wv_f, bv, Wg_f = self.sampler_operands("gsamp", feat.dtype, query=False)[1]
        vp, G = self.products.buffers(self, torch.bfloat16, n_img, S, Cc, feat.device)
        return [(Wv_f, bv, vp, True), (Wg_f, None, G, False)]

    def project_values(self, feat):
        """value = rayconv(input_flatten) (projattn.py:169) as bf16 head planes vh[img][head][s][32]."""
        n_img, S, Cc = feat.shape
        Wv_f, bv, _ = self.sampler_operands("gsamp", feat.dtype, query=False)[1]
        vp = self.products.buffers(self, torch.bfloat16, n_img, S, Cc, feat.device)[0]
        ops.value_proj_planes_ws(feat, Wv_f, bv, vp)
        return vp

    def native_forward(self, x, r, feat, levels, V, B, rowmask=None, order=None):
        """Inference path on packed inputs.  x (B,Lq,C) f32 = tgt+query_pos; r (V*B,Lq,L,2) the
        per-level reference points; feat (V*B,S,C) channels-last pyramid in the compute dtype.
        Returns (V*B*Lq, C).  order (with rowmask, fp32): the pairs' processing order (ops.bin_pairs: masked pairs last) --
        tiles of the output projection without an unmasked row are not computed (their rows are zero either way)."""
        samp = self.native_sample(x, r, feat, levels, V, B, pair_mask=rowmask, order=order)
        Wp, bp, zero = self.output_operands(feat.dtype, order is not None and rowmask is not None and feat.dtype == torch.float32)
        if zero is not None:
            return ops.linear_ordered(samp, Wp, bp, order, rowmask, zero, rowmask=rowmask)
        return ops.linear(samp, Wp, bp, out_dtype=feat.dtype, rowmask=rowmask)   # projattn.py:203 (+ dq_decoder.py:585)

    def query_term_weights(self, dt, path="bf16"):
        """operands of xw = (tgt + query_pos) @ [Woff; Wattn]^T + b as the fused chain B of the PREVIOUS layer takes them, rows in
        gsamp_column_order and zero-padded to 256: (weight fragments (256,256) bf16, bias (256,) f32, n = 192) for the "bf16" chain,
        (two-part fp16 planes, their scale, bias, n) for the "f32h" one."""
        perm = lambda a, b: torch.cat([a, b], 0)[ops.gsamp_column_order(a.device)]
        if path == "f32h":
            W = self.pyramid_planes_f32h()[1]       # the G operand of mvg_pyramid_f32h is the same weight
        else:
            pad = lambda a, b: ops.swizzle_weight(torch.cat([perm(a, b), a.new_zeros(64, a.shape[1])], 0).to(dt))
            W = (self._wc.get("Woa_frag", (self.sampling_offsets.weight, self.attention_weights.weight), dt, pad),)
        bpad = lambda a, b: torch.cat([perm(a, b), a.new_zeros(64)], 0)
        bn = self._wc.get("boa_pad", (self.sampling_offsets.bias, self.attention_weights.bias), torch.float32, bpad)
        return W + (bn, 192)

    def pyramid_planes_f32h(self):
        """operands of mvg_pyramid_f32h: ((value planes, scale), (G planes, scale)) -- two fp16 parts of each weight times a power of two"""
        f16 = torch.float16
        perm = lambda a, b: ops.split_swizzle_weight_h2(torch.cat([a, b], 0)[ops.gsamp_column_order(a.device)])
        return (self._wc.get("Wv_f32h", (self.rayconv.weight,), f16, ops.split_swizzle_weight_h2),
                self._wc.get("Woa_f32h", (self.sampling_offsets.weight, self.attention_weights.weight), f16, perm))

    def _fast_query_weights(self, dt):
        """[offsets; logits] Linear in the column order of the G-sampling kernel (ops.gsamp_column_order)."""
        perm = lambda a, b: torch.cat([a, b], 0)[ops.gsamp_column_order(a.device)]
        W = self._wc.get("Woa_perm", (self.sampling_offsets.weight, self.attention_weights.weight), dt, perm)
        b = self._wc.get("boa_perm", (self.sampling_offsets.bias, self.attention_weights.bias), torch.float32, perm)
        return W, b

    def native_sample(self, x, r, feat, levels, V, B, pair_mask=None, order=None, xw=None, operands=None):
        """everything of native_forward up to (not including) output_proj: (V*B*Lq, C) sampled values.
        x (B,Lq,C) f32 = tgt + query_pos, or a callable returning it (only evaluated when needed: with xw given --
        the query term (B*Lq,192) precomputed by the previous layer -- the bf16 fast path never touches x).
        pair_mask (V*B*Lq) u8: rows the caller is going to multiply by 0 (reference point outside the image,
        dq_decoder.py:585-586); the bf16 fast path returns zeros for them instead of sampling.
        operands: (sampler_form, sampler_operands of it) when the caller holds them already (DQDecoderLayer's plan)."""
        dt = feat.dtype
        n_img, S, Cc = feat.shape
        if operands is None:
            form = self.sampler_form(dt, r.shape[1], levels.L, S)
            operands = form, self.sampler_operands(form, dt)
        form, ((Wq, bq), pyramid) = operands
        parts = getattr(x, "parts", None)        # (tgt, query_pos) when the caller has not formed tgt + query_pos yet
        g16 = form == "gsamp"
        if callable(x) and (form == "gather" or (xw is None and not (g16 and parts is not None))):
            x = x()
        if form == "gather":
            ain = ops.gather_ref(feat, r, x, levels, V, B)                       # projattn.py:148-153,180 (+query)
            oa = ops.linear(ain, Wq, bq, out_dtype=torch.float32)                # projattn.py:180-181
            value = ops.linear(feat.view(n_img * S, Cc), *pyramid, out_dtype=dt)    # projattn.py:169
            return ops.msda_fused(value.view(n_img, S, Cc), oa, r, levels)       # projattn.py:184-200
        # Linear(bilinear(feat) + x) = bilinear(Linear(feat)) + Linear(x): project the pyramid once (G) instead of V*Lq*L gathered
        # rows (fp32: no `ain` (236 MB) / `oa` (177 MB) per layer), compute the query term once per layer (xw), gather offsets /
        # logits inside the sampler (csrc/msda.hip).  Processing order of the pairs: given by the caller (DQDecoderLayer shares
        # it with chain A) or binned here -- in front of the query term in bf16, behind it in fp32.
        binned = order is None and self.sort_pairs and r.shape[1] <= 65536
        if binned and g16:
            order = ops.bin_pairs(r, pair_mask, levels)
        if xw is None:      # else: already computed by the previous layer's fused chain B
            if g16 and parts is not None:   # first layer: tgt + query_pos formed inside the GEMM's loader (mvg_linear_sum)
                xw = ops.linear(parts[0].reshape(-1, Cc), Wq, bq, out_dtype=torch.float32, add=parts[1].reshape(-1, Cc))
            else:
                xw = ops.linear(x.reshape(-1, Cc), Wq, bq, out_dtype=torch.float32)
        if binned and not g16:
            order = ops.bin_pairs(r, pair_mask, levels)
        # the two pyramid products: computed here, or ahead of time on the side stream (DQDecoder.launch_pyramid_projections)
        vp, G = self.products.take(self) or self.project_pyramid(feat)
        sample = ops.msda_gsamp if g16 else ops.msda_gfused_f32
        return sample(vp, G, xw, r, levels, B, pair_mask=pair_mask, order=order)   # projattn.py:148-200

    # ------------------------------------------------------------------------------- forward
    def _step(self, n):
        """im2col_step handed to the op for a batch of n images.  The reference calls the op once per view with the per-view
        batch B (dq_decoder.py:552-593) and its kernel chunks the batch by im2col_step = 64 (deform_cuda.cu:61-86); here all
        V views go through as ONE batch of V * B images and the kernels never chunk, so the argument is only the op's
        compatibility check: a step that divides n whenever the reference's per-view call would have passed."""
        return n if n <= self.im2col_step else math.gcd(n, self.im2col_step)

    def _ref_gather(self, flat, loc, shapes, starts):
        """bilinear features of every level at its reference point: flat (n, S, C) channels-last pyramid, loc (n, Lq, L, 2)
        in [0, 1] map coordinates (align_corners=False, zero padding -- grid_sample's and the op's common convention)
        -> (n, Lq, L, C), differentiable in flat and loc through DeformFunction."""
        n, Lq, nl, _ = loc.shape
        M = self.n_heads
        C = flat.shape[-1]
        locs = loc.view(n, Lq, 1, 1, nl, 1, 2).expand(n, Lq, nl, M, nl, 1, 2).reshape(n, Lq * nl, M, nl, 1, 2)
        onehot = torch.eye(nl, dtype=flat.dtype, device=flat.device).view(1, 1, nl, 1, nl, 1)
        w = onehot.expand(n, Lq, nl, M, nl, 1).reshape(n, Lq * nl, M, nl, 1)
        out = DeformFunction.apply(flat.view(n, -1, M, C // M), shapes.contiguous(), starts.contiguous(), locs.contiguous(),
                                   w.contiguous(), self._step(n))
        return out.view(n, Lq, nl, C)

    def forward(self, query, reference_points, src_views, camera_ray_embeds, input_spatial_shapes,
                input_level_start_index, input_padding_mask=None, packed=None):
        """Reference signature (projattn.py:115-117).  query (n_views, Lq, C); reference_points
        (n_views, Lq, n_levels, 2) already rescaled per level; src_views list of (n_views,C,H,W).
        packed (beyond the reference signature): the channels-last pyramid (n_views, S, C) the decoder packed from src_views."""
        if not query.is_cuda:
            raise RuntimeError("Not implemented on the CPU")                  # deform.h:49
        if query.device.index != torch.cuda.current_device():
            with torch.cuda.device(query.device):   # kernels go to the current stream of the TENSORS' device
                return self.forward(query, reference_points, src_views, camera_ray_embeds, input_spatial_shapes,
                                    input_level_start_index, input_padding_mask, packed)
        n_views, Len_q, c = query.shape
        feat_lvls = len(src_views)
        if self.projattn_posembed_mode != "ablation_not_use_rayconv":
            raise NotImplementedError("projattn_posembed_mode=%r: only 'ablation_not_use_rayconv' (every shipped "
                                      "YAML) is built" % self.projattn_posembed_mode)
        if reference_points.shape[-1] != 2:
            raise ValueError("Last dim of reference_points must be 2, but get {} instead."
                             .format(reference_points.shape[-1]))
        if not torch.is_grad_enabled() and input_padding_mask is None and self.fused_supported(feat_lvls):
            levels = ops.Levels(input_spatial_shapes, input_level_start_index)
            feat = ops.pack_pyramid(src_views, levels, self.compute_dtype)
            out = self.native_forward(query.float().contiguous(), reference_points.float().contiguous(), feat, levels,
                                      1, n_views)
            return out.view(n_views, Len_q, c).to(query.dtype)
        sample_grid = torch.clamp(reference_points * 2.0 - 1.0, -1.1, 1.1)
        # bf16 mixed-precision training (DQDecoderLayer.set_training_dtype): the Linears on LinearBF16, a bf16 value for the
        # sampling op, and a bf16 packed pyramid taken as it is (its consumers round to bf16 anyway)
        bf = self.training_dtype == torch.bfloat16
        if (packed is not None and (packed.dtype == torch.float32 or (bf and packed.dtype == torch.bfloat16))
                and packed.shape[0] == n_views and packed.shape[2] == c and not any(s.requires_grad for s in src_views)):
            # the channels-last pyramid the decoder packed once per forward IS cat + permute of the maps (projattn.py:160); only
            # when no gradient flows into the feature maps (the packing kernel is not differentiable)
            input_flatten = packed
        else:
            input_flatten = torch.cat([s.flatten(2) for s in src_views], dim=-1).permute(0, 2, 1)
        # (from the host copy of the level table, kept on the tensor object: no D2H read per forward, none inside a graph capture)
        assert sum(h * w for h, w in ops_host_levels_pair(input_spatial_shapes, input_level_start_index)[0]) == input_flatten.shape[1]
        xin = None
        if (self.ref_gather_native and (input_flatten.dtype == torch.float32 or bf) and not input_flatten.requires_grad
                and not reference_points.requires_grad and c % 4 == 0):
            # neither the maps nor the reference points carry a gradient (run/train_3d.py with a frozen backbone and
            # detach_refpoints_cameraprj, every shipped YAML): the inference path's gather kernel forms feats + query in one launch
            # (the sampling op with one-hot level weights sampled every level three times: 380 us against ~100); the only gradient,
            # d / d query, is the sum over the levels
            from .functions import RefGatherAdd
            levels = ops.Levels(*ops_host_levels_pair(input_spatial_shapes, input_level_start_index))
            xin = RefGatherAdd.apply(query.contiguous(), input_flatten.contiguous(), reference_points.detach().float().contiguous(), levels)
        elif self.ref_gather_native and input_flatten.dtype == torch.float32:
            # reference-point features through the sampling op itself (forward AND deterministic backward kernels) instead
            # of L grid_sample launches on the NCHW maps (projattn.py:134-141; 17 % of a training step): the channels-last
            # pyramid is the op's value with M heads of C / M channels, token (q, l) samples level l at the clamped
            # reference point with weight 1 (one point per level, the other levels' weights are 0).
            input_flatten = input_flatten.contiguous()
            feats = self._ref_gather(input_flatten, (sample_grid + 1.0) * 0.5, input_spatial_shapes, input_level_start_index)
        else:
            feats = torch.stack([F.grid_sample(src_views[l], sample_grid[:, :, l:l + 1, :], align_corners=False).squeeze(-1)
                                 .permute(0, 2, 1) for l in range(feat_lvls)], dim=2)
        from .functions import linear as lin
        if bf:
            from .functions import linear_bf16
            wc = self._wc
            value = linear_bf16(input_flatten, self.rayconv.weight, self.rayconv.bias, wc, "train16/Wv", out_bf16=True)
        else:
            value = lin(input_flatten, self.rayconv.weight, self.rayconv.bias)
        if input_padding_mask is not None:
            value = value.masked_fill(input_padding_mask[..., None], float(0))
        value = value.view(n_views, -1, self.n_heads, self.d_model // self.n_heads)
        if xin is None:
            xin = feats + query.unsqueeze(2)
        n_off = self.sampling_offsets.out_features
        w_oa = torch.cat([self.sampling_offsets.weight, self.attention_weights.weight], 0)               # one GEMM for both heads
        b_oa = torch.cat([self.sampling_offsets.bias, self.attention_weights.bias], 0)
        if bf:
            oa = linear_bf16(xin, w_oa, b_oa, wc, "train16/Woa", params=(self.sampling_offsets.weight, self.attention_weights.weight),
                             build=lambda a, b: torch.cat([a, b], 0))
        else:
            oa = lin(xin, w_oa, b_oa)
        sampling_offsets = oa[..., :n_off].reshape(n_views, Len_q, self.n_heads, feat_lvls, self.n_points, 2)
        attention_weights = oa[..., n_off:].reshape(n_views, Len_q, self.n_heads, feat_lvls * self.n_points)
        attention_weights = F.softmax(attention_weights, -1).view(n_views, Len_q, self.n_heads, feat_lvls,
                                                                  self.n_points)
        offset_normalizer = torch.stack([input_spatial_shapes[..., 1], input_spatial_shapes[..., 0]], -1)
        sampling_locations = reference_points[:, :, None, :, None, :] \
            + sampling_offsets / offset_normalizer[None, None, None, :, None, :]
        output = DeformFunction.apply(value.contiguous(), input_spatial_shapes.contiguous(),
                                      input_level_start_index.contiguous(), sampling_locations.contiguous(),
                                      attention_weights.contiguous(), self._step(n_views))
        if bf:
            return linear_bf16(output, self.output_proj.weight, self.output_proj.bias, wc, "train16/Wp")
        return lin(output, self.output_proj.weight, self.output_proj.bias)


# north_star alias
MSDeformAttn = ProjAttn
