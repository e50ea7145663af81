"""The whole training step -- DecoderHead.forward_train, total_loss, backward(), FusedAdam.step(loss=total) -- captured ONCE as a HIP
graph and replayed per iteration (single GPU): the training counterpart of serving.GraphedDecoder.

  TrainOperands      the (W16, W16^T) bf16 copies of the weights that the bf16 training path multiplies by, in persistent buffers
                     that the device rewrites behind the optimizer's update kernel (csrc/operands.hip, one launch)
  GraphedTrainStep   static inputs + the captured step: load() / set_cameras() / replay() / eager()

Why the operands: in bf16 training every LinearBF16 reads cached bf16 copies of its fp32 master weight, built by torch casts on the
host's order and keyed on Parameter._version (projattn.WeightCache).  A replay runs no host code, so a captured step would go on
multiplying by the weights of the step it was captured at.  TrainOperands owns the copies, registers them with the layers' caches
(WeightCache.adopt) and FusedAdam (attach_operands) launches their refresh inside the step -- and so inside the graph.

    ops16 = TrainOperands(head)                        # bf16 training only
    optimizer.attach_operands(ops16)
    step = GraphedTrainStep(head, optimizer, weight_dict, src_views, meta, operands=ops16).capture()
    for batch in loader:
        step.load(src_views=batch.maps, meta=batch.meta)         # device copies, no synchronisation
        step.set_cameras(batch.meta)                             # only when calibration / crop changed
        total, loss_dict, grad_norm, out = step.replay()         # static tensors, overwritten by the next replay

capture() runs its warm-up as real optimizer steps on the first batch (see its docstring).  Static per runner: shapes (views, batch, maps, ground-truth slots), the head's set of trainable parameters and their .grad tensors
(FusedAdam with zero_grad=True zeroes them in place), the optimizer's tables.  A replay may follow: new feature maps and ground
truth (load), new cameras (set_cameras), new group hyper-parameters (a scheduler step, then optimizer.prepare()), parameters
written outside the graph (a checkpoint load, then refresh_operands()).  Dropout stays torch's: under capture its Philox offset
advances per replay."""
from __future__ import annotations

import torch

from . import ops
from .caller import level_tables, total_loss
from .decoder import DecoderContext, refuse_live_views

TILE = ops.OPERANDS_TILE
RECORD_WORDS = ops.OPERANDS_RECORD_WORDS


def _decoder_of(model):
    return model.decoder if hasattr(model, "decoder") else model


def operand_specs(model):
    """[(cache, key, params)]: one entry per weight that DQDecoderLayer.forward_autograd / ProjAttn.forward hand to linear_bf16 under
    training_dtype bfloat16 -- the WeightCache it is looked up in, its key (the transposed copy: key + '^T') and the parameters
    the entry is stamped with (two for ProjAttn's concatenated [sampling_offsets; attention_weights]).  No device is touched."""
    specs, seen = [], set()
    for layer in _decoder_of(model).layers:
        if id(layer) in seen:           # share_layer_weights: one layer object at every position
            continue
        seen.add(id(layer))
        pa = layer.proj_attn
        specs.append((pa._wc, "train16/Wv", (pa.rayconv.weight,)))
        specs.append((pa._wc, "train16/Woa", (pa.sampling_offsets.weight, pa.attention_weights.weight)))
        specs.append((pa._wc, "train16/Wp", (pa.output_proj.weight,)))
        mine = [layer.feature_update_mlp.weight]
        if layer.open_forward_ffn:
            mine += [layer.linear1.weight, layer.linear2.weight]
        mine += [layer.class_embed.weight] + [l.weight for l in layer.pose_embed.MLP.layers]
        specs += [(layer._wc, "train16/%x" % id(w), (w,)) for w in mine]
    out = []
    for cache, key, params in specs:
        K = params[0].shape[1]
        N = sum(p.shape[0] for p in params)
        if any(p.dim() != 2 or p.shape[1] != K for p in params):
            raise RuntimeError("TrainOperands: %s is not a stack of (n, %d) matrices" % (key, K))
        if N % 64 == 0 and K % 64 == 0:         # functions.linear_bf16's rule; the 2- and 3-output heads stay on fp32 operands
            out.append((cache, key, params))
    return out


def build_tables(entries):
    """entries: [(params, w16 (N, K) bf16, w16t (K, N) bf16)] -> (record table (n_records, 8) int64, tile table (n_tiles, 2)
    int32) of mvg_refresh_operands as HOST tensors (include/mvg_decoder.h).  One record per parameter: the rows of a concatenated
    weight go to a row offset of w16 and a column offset of w16t."""
    records, tiles = [], []
    for params, w16, w16t in entries:
        N, K = w16.shape
        if tuple(w16t.shape) != (K, N) or not w16.is_contiguous() or not w16t.is_contiguous() \
                or w16.dtype != torch.bfloat16 or w16t.dtype != torch.bfloat16:
            raise RuntimeError("TrainOperands: destinations must be contiguous bf16 (N, K) / (K, N)")
        row = 0
        for p in params:
            if p.dtype != torch.float32 or p.dim() != 2 or p.shape[1] != K or p.stride(1) != 1 or p.device != w16.device:
                raise RuntimeError("TrainOperands: sources must be fp32 (n, K) matrices with unit column stride on the "
                                   "destinations' device")
            n = p.shape[0]
            if row + n > N:
                raise RuntimeError("TrainOperands: the sources have more rows than their destination")
            rec = len(records)
            records.append((p.data_ptr(), n, K, p.stride(0), w16.data_ptr() + row * K * 2, K, w16t.data_ptr() + row * 2, N))
            n_tiles = -(-n // TILE) * -(-K // TILE)
            tiles += [(rec, t) for t in range(n_tiles)]
            row += n
        if row != N:
            raise RuntimeError("TrainOperands: the sources do not fill their destination")
    return (torch.tensor(records, dtype=torch.int64).reshape(-1, RECORD_WORDS),
            torch.tensor(tiles, dtype=torch.int32).reshape(-1, 2))


class TrainOperands:
    """Persistent (W16, W16^T) buffers for every weight of operand_specs(model), on the parameters' device; adopted by the layers'
    WeightCaches, so linear_bf16 multiplies by THESE tensors.  refresh() rewrites all of them from the current master weights in
    one launch on the current stream and re-stamps the cache entries.  Build it after the model is on its device; moving or
    replacing parameters afterwards needs a new one."""

    def __init__(self, model):
        self.entries = []           # (cache, key, params, w16, w16t)
        for cache, key, params in operand_specs(model):
            dev = params[0].device
            N, K = sum(p.shape[0] for p in params), params[0].shape[1]
            w16 = torch.zeros((N, K), dtype=torch.bfloat16, device=dev)
            w16t = torch.zeros((K, N), dtype=torch.bfloat16, device=dev)
            self.entries.append((cache, key, params, w16, w16t))
        devs = {e[3].device for e in self.entries}
        if len(devs) > 1:
            raise RuntimeError("TrainOperands: parameters on %s; one device per instance" % sorted(map(str, devs)))
        self.device = devs.pop() if devs else None
        self.record_table_host, self.tile_table_host = build_tables([(p, a, b) for _, _, p, a, b in self.entries])
        self.record_table = self.tile_table = None
        if self.device is not None and self.device.type == "cuda":
            # one upload; the launch reads the tables from device memory, so no kernel argument depends on the parameter set
            self.record_table = self.record_table_host.to(self.device)
            self.tile_table = self.tile_table_host.to(self.device)
            self.refresh()
            for cache, key, params, w16, w16t in self.entries:
                cache.adopt(key, params, torch.bfloat16, w16)
                cache.adopt(key + "^T", params, torch.bfloat16, w16t)

    def launch(self):
        """the refresh alone, on the current stream (FusedAdam.step calls it behind its update kernel, then restamp())"""
        if self.record_table is None:
            raise RuntimeError("Not implemented on the CPU")
        with torch.cuda.device(self.device):
            ops.refresh_operands(self.record_table, self.tile_table)

    def restamp(self):
        for cache in {id(e[0]): e[0] for e in self.entries}.values():
            cache.restamp()

    def refresh(self):
        """all copies from the current master weights: one launch, no host synchronisation; after any write to the parameters that
        did not go through the attached optimizer's step (a checkpoint load)"""
        self.launch()
        self.restamp()
        return self

    def tensors(self):
        return [t for e in self.entries for t in e[3:5]] + [self.record_table, self.tile_table]


def _clone_meta(meta, dev):
    mv = lambda t: t.detach().to(dev).clone() if torch.is_tensor(t) else t      # noqa: E731
    return [{k: ({kk: mv(vv) for kk, vv in v.items()} if isinstance(v, dict) else mv(v)) for k, v in m.items()} for m in meta]


class GraphedTrainStep:
    """One training step of `head` (a caller.DecoderHead with its criterion set) under `optimizer` (an optim.FusedAdam built with
    zero_grad=True) as one HIP graph.  src_views / meta give the shapes and the first batch; they are copied into static buffers.
    operands: the TrainOperands attached to the optimizer -- required when the decoder trains in bf16, unused in fp32 (LinearF32S
    reads the master weights)."""

    GROUND_TRUTH = ("joints_3d", "joints_3d_vis", "num_person")

    def __init__(self, head, optimizer, weight_dict, src_views, meta, spatial_shapes=None, level_start_index=None, threshold=0.1,
                 operands=None):
        from .optim import FusedAdam
        dev = src_views[0].device
        if dev.type != "cuda":
            raise RuntimeError("Not implemented on the CPU")
        if not isinstance(optimizer, FusedAdam):
            raise TypeError("GraphedTrainStep: the optimizer must be an optim.FusedAdam (its step runs on the device, without a "
                            "host read-back), got %s" % type(optimizer).__name__)
        if not optimizer.zero_grad_after_step:
            raise ValueError("GraphedTrainStep: the FusedAdam must be built with zero_grad=True: the update kernel then zeroes the "
                             "gradients in place and the .grad addresses in its tables stay valid from replay to replay")
        if head.criterion is None:
            raise RuntimeError("GraphedTrainStep: the head has no criterion (set_criterion / factory.build_training_head)")
        self.head, self.opt, self.weight_dict, self.thr, self.dev = head, optimizer, dict(weight_dict), float(threshold), dev
        self.operands = operands
        self.bf16 = any(l.training_dtype == torch.bfloat16 for l in head.decoder.layers)
        with torch.no_grad():
            self.src_views = [s.detach().clone() for s in src_views]
        self.meta = _clone_meta(meta, dev)
        if spatial_shapes is None:
            spatial_shapes, level_start_index = level_tables(self.src_views)
        self.spatial_shapes, self.level_start_index = spatial_shapes.to(dev), level_start_index.to(dev)
        self.V = len(meta)
        self.batch = self.src_views[0].shape[0] // self.V
        layer0 = head.decoder.layers[0]
        self.ctx = DecoderContext.prepare(self.spatial_shapes, self.level_start_index, self.meta, layer0.img_size,
                                          layer0.compute_dtype, self.batch, dev)
        self.graph, self.outputs = None, None
        self._pinned, self._grad_ptrs = [], None

    # ------------------------------------------------------------------ inputs (device-side copies on the current stream)
    def load(self, src_views=None, meta=None):
        """new feature maps and / or ground truth (meta[0]: joints_3d, joints_3d_vis, num_person; every meta[v]: joints_vis)"""
        with torch.no_grad():
            if src_views is not None:
                for dst, s in zip(self.src_views, src_views):
                    dst.copy_(s, non_blocking=True)
            if meta is not None:
                if len(meta) != self.V:
                    raise RuntimeError("load: %d views, the runner was built for %d" % (len(meta), self.V))
                for k in self.GROUND_TRUTH:
                    self.meta[0][k].copy_(meta[0][k], non_blocking=True)
                for mine, m in zip(self.meta, meta):
                    mine["joints_vis"].copy_(m["joints_vis"], non_blocking=True)
        return self

    def set_cameras(self, meta):
        """new calibration / crop for the same number of images: refills the packed camera records in place (host packing + one
        small H2D copy) and, from them, the projection matrices the captured step reads; no re-capture"""
        self.ctx.set_cameras(meta, self.head.decoder.layers[0].img_size)
        with torch.no_grad():
            for mine, m in zip(self.meta, meta):        # what the eager path may read from the meta dicts themselves
                for k in ("camera", "center", "scale", "rotation"):
                    if k not in m or k not in mine:
                        continue
                    if isinstance(m[k], dict):
                        for kk, vv in m[k].items():
                            mine[k][kk].copy_(vv)
                    elif torch.is_tensor(m[k]):
                        mine[k].copy_(m[k])
        return self

    def refresh_operands(self):
        """after a write to the parameters outside the graph (a checkpoint load): one launch, no re-capture"""
        if self.operands is not None:
            self.operands.refresh()
        return self

    # ------------------------------------------------------------------ the step
    def _step(self):
        refuse_live_views(self.ctx, "GraphedTrainStep")
        out, loss_dict = self.head.forward_train(self.src_views, self.meta, self.spatial_shapes, self.level_start_index,
                                                 threshold=self.thr, context=self.ctx)
        total = total_loss(loss_dict, self.weight_dict)
        total.backward()
        norm = self.opt.step(loss=total)
        return total.detach(), loss_dict, norm, out

    def eager(self):
        """the identical step without the graph"""
        return self._step()

    def _grads(self):
        return tuple((id(p), None if p.grad is None else p.grad.data_ptr()) for g in self.opt.param_groups for p in g["params"])

    def _check(self):
        if self.bf16:
            if self.operands is None or self.opt.operands is not self.operands:
                raise RuntimeError("GraphedTrainStep: bf16 training needs a training.TrainOperands, attached to the optimizer "
                                   "(optimizer.attach_operands(ops)) and passed as operands=: a replay runs no host code, so the "
                                   "bf16 copies of the weights must be rewritten on the device inside the captured step")

    def capture(self, warmup=3):
        """Warm up, then capture the step.  The `warmup` (at least 1) warm-up steps are REAL training steps on the batch the runner
        holds: parameters, moments and the optimizer's step count move by `warmup` steps (they allocate every .grad, size the
        buffers and build the caches; there is no way to do that without running the step).  The captured step itself is
        recorded, not executed.  To start training from an exact state, capture first and then write that state back in place
        (parameters, exp_avg / exp_avg_sq, the step count) followed by refresh_operands(); or accept the head start."""
        self._check()
        with torch.cuda.device(self.dev):
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(max(1, warmup)):     # allocates every .grad, sizes the buffers, builds the caches and constants
                    self._step()
            torch.cuda.current_stream().wait_stream(side)
            self.opt.prepare()                      # tables for the gradients as they are now, group hyper-parameters
            if self.operands is not None:
                self.operands.refresh()
            before = self._grads()
            torch.cuda.synchronize(self.dev)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                outputs = self._step()
            self.outputs = outputs
            self._grad_ptrs = self._grads()
            # everything the graph addresses by raw pointer and does not own
            self._pinned = self._graph_operands()
            if self._grad_ptrs != before:
                self.graph = None
                raise RuntimeError("GraphedTrainStep: a .grad tensor was (re)allocated during the capture; the optimizer's tables "
                                   "hold the old addresses")
        return self

    def _graph_operands(self):
        keep = self.ctx.tensors() + self.head.decoder.products.tensors()
        keep += self.src_views + [self.spatial_shapes, self.level_start_index]
        for layer in self.head.decoder.layers:
            keep += layer._wc.tensors() + layer.proj_attn._wc.tensors()
            keep += list(layer.__dict__.get("_img_dev", {}).values())
        if self.operands is not None:
            keep += self.operands.tensors()
        tables = self.opt._tables
        keep += [tables[1], tables[2], tables[3], self.opt._groups_dev, self.opt._state_dev]
        for g in self.opt.param_groups:
            for p in g["params"]:
                keep += [p, p.grad] + [t for t in self.opt.state.get(p, {}).values() if torch.is_tensor(t)]
        return [t for t in keep if t is not None]

    def replay(self):
        """one training step on the loaded inputs: (total loss, loss dict, gradient norm before clipping, out dict) -- the graph's
        static tensors, overwritten by the next replay"""
        refuse_live_views(self.ctx, "GraphedTrainStep")
        if self.graph is None:
            self.capture()
        if self._grads() != self._grad_ptrs:
            raise RuntimeError("GraphedTrainStep: a parameter's .grad moved since the capture (set to None, or replaced): the "
                               "captured step and the optimizer's tables address the old tensors; capture() again")
        self.graph.replay()
        self.opt.mark_updated()
        return self.outputs
