"""Frame-by-frame inference with the decoder forward captured ONCE as a HIP graph (single GPU).

The reference runs ``model(views, meta)`` eagerly per frame (lib/core/function.py:360-396): ~25 kernel launches per decoder layer,
several host synchronisations.  Here the whole ``DQDecoder.forward`` -- pyramid packing, the side-stream GEMM train, all layers,
triangulation, output stacking -- has static shapes and no host synchronisation, so it is captured once and replayed per frame:
one graph launch on the host (what ``bench.py`` times).  The graph holds raw pointers into its input buffers, the decoder's
weight caches and its per-layer value / G buffers: ``GraphedDecoder`` owns the inputs and, from the capture on, holds a
reference to every one of those tensors (``_pinned``) -- an eager call of the same decoder with another batch, resolution or
compute dtype re-allocates the product buffers (``PyramidProducts``) and rebuilds cache entries, and without the references the
graph would go on reading and writing recycled memory.  ``replay()`` also compares the buffers' signature with the captured one and
re-captures when the decoder has moved on to other buffers.

    runner = GraphedDecoder(decoder, meta, spatial_shapes, level_start_index, batch=1, num_queries=1024, threshold=0.1)
    for frame in stream:
        runner.load(src_views=frame.feature_maps, tgt=..., query_pos=..., reference_points=...)   # device copies, no sync
        hs, refs, refs2d, projs2d, class_probs = runner.replay()

Static per runner: the cameras (``meta``; call ``set_cameras`` when they change -- a 960-byte host-packed record per image, no
re-capture), map shapes, batch, query count, threshold and the decoder's weights (``refresh_weights()`` after an optimizer step
or a checkpoint load re-captures).  A backbone that writes its deconvolution outputs into ``runner.pyramid_views`` (channels-last,
compute dtype) makes ``load(src_views=...)`` unnecessary.

``postprocess=dict(...)`` continues the captured region behind the decoder with the classification filter and the NMS
(``ops.pose_nms``) into static buffers, and ``evaluation``, ``tracking``, ``track_evaluation`` and ``refine`` hang further device
stages behind the NMS, inside the same graph.  All of that -- the options and their defaults, the buffers, the launch order --
belongs to ``postprocess.PostProcess`` (described there); the runner builds one as ``runner.post``, captures ``post.run`` behind the
decoder, pins ``post.tensors()`` and puts ``post.snapshot()`` back after the warm-up forwards of a capture, which therefore score,
age and count nothing.  ``replay()`` still returns the five decoder outputs; ``runner.pred`` is the packed predictions
(B, NQ, J, 5), and the pipeline's static tensors and stage objects are attributes of the runner under the same names
(``detections``, ``evaluator``, ``ground_truth``, ``tracker``, ``track_ids``, ``track_poses``, ``track_evaluator``, ``person_id``,
``refiner``, ``refined``, ``bone_lengths``, ``bone_estimator``, ``bone_source``; None for a stage that was not asked for):

        runner.replay()
        dets, count, keep = runner.detections
        n = int(count[0, 0])                # the frame's one read-back
        poses = dets[0, :n]                 # (n, J, 5) on the device

``load(ground_truth=(joints_3d, joints_3d_vis, num_person[, person_id]))`` fills the static inputs of the two scorers, and
``set_cameras`` refills the refiner's projection matrices along with the camera records.
"""
from __future__ import annotations

import torch

from .decoder import DecoderContext


class GraphedDecoder:
    def __init__(self, decoder, meta, spatial_shapes, level_start_index, batch, num_queries, threshold=0.1, device=None,
                 producer_writes_in_place=False, channels=256, postprocess=None, convert_joint_format_indices=None, evaluation=None,
                 tracking=None, refine=None, track_evaluation=None, live_views=False):
        layer0 = decoder.layers[0]
        dev = torch.device(device) if device is not None else next(decoder.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("Not implemented on the CPU")
        self.dec, self.thr, self.dev = decoder, float(threshold), dev
        self.dtype = layer0.compute_dtype
        J, C = layer0.num_joints, channels
        self.V = len(meta)
        Lq = num_queries * J
        self.spatial_shapes = spatial_shapes.to(dev)
        self.level_start_index = level_start_index.to(dev)
        self.meta = meta
        self.ctx = DecoderContext.prepare(self.spatial_shapes, self.level_start_index, meta, layer0.img_size, self.dtype, batch, dev)
        # live_views: the graph is captured with the kernels that read the context's live-view table (all views live until
        # load(view_live=...) says otherwise); without it the graph holds the launches without a table
        self.live_views = bool(live_views)
        if self.live_views:
            self.ctx.set_live_views([True] * self.V)
        # static inputs
        self.tgt = torch.zeros((batch, Lq, C), dtype=torch.float32, device=dev)
        self.query_pos = torch.zeros((batch, Lq, C), dtype=torch.float32, device=dev)
        self.reference_points = torch.zeros((batch, Lq, 3), dtype=torch.float32, device=dev)
        self.in_place = bool(producer_writes_in_place)
        if self.in_place:       # the producer's output buffers ARE the packed pyramid (no per-frame pack kernels)
            self.pyramid_views = self.ctx.pyramid_buffers(channels=C, device=dev)
            self.src_views = self.pyramid_views
        else:                   # the reference's hand-over format: NCHW fp32 maps, view-major
            shapes = [(int(h), int(w)) for h, w in self.spatial_shapes.tolist()]
            self.src_views = [torch.zeros((self.V * batch, C, h, w), dtype=torch.float32, device=dev) for h, w in shapes]
            self.pyramid_views = None
        self.graph, self.outputs = None, None
        self._pinned, self._captured = [], None
        # optional device-side post-processing behind the decoder, inside the same graph: one pipeline object owns all of it
        self.post, self.pred, self._graph_pred = None, None, None
        stages = dict(postprocess=postprocess, evaluation=evaluation, tracking=tracking, track_evaluation=track_evaluation,
                      refine=refine)
        if any(v is not None for v in stages.values()):
            from .postprocess import PostProcess
            self.post = PostProcess(batch, num_queries, J, self.thr, dev, convert_joint_format_indices=convert_joint_format_indices,
                                    **stages).set_cameras(self.ctx.cams, self.V).set_live_views(self.ctx.live)
        for name in ("postprocess", "detections", "evaluator", "ground_truth", "tracker", "track_ids", "track_poses",
                     "track_evaluator", "person_id", "refiner", "refined", "bone_lengths", "bone_estimator", "bone_source"):
            setattr(self, name, getattr(self.post, name, None))         # static tensors and objects: bound once

    # ------------------------------------------------------------------ inputs (device-side copies on the current stream)
    def load(self, src_views=None, tgt=None, query_pos=None, reference_points=None, ground_truth=None, view_live=None):
        """ground_truth: see ``postprocess.PostProcess.load_ground_truth`` (a runner built with ``evaluation`` or
        ``track_evaluation``).  view_live: the mask of ``DecoderContext.set_live_views`` -- (B, V) or (V,) bool on the host -- for a
        runner built with ``live_views=True``: validated on the host and copied into the table's static buffers (two small H2D
        copies; no re-capture, nothing inside ``replay()``).  It stays in force until the next one."""
        if view_live is not None:
            if not self.live_views:
                raise RuntimeError("GraphedDecoder.load: view_live needs a runner built with live_views=True (the graph is "
                                   "captured with the kernels that read the table)")
            self.ctx.set_live_views(view_live)
        with torch.no_grad():
            if ground_truth is not None:
                if self.post is None:
                    raise ValueError("GraphedDecoder: ground_truth needs a runner built with evaluation=dict(...) or "
                                     "track_evaluation=dict(...)")
                self.post.load_ground_truth(ground_truth)
            if src_views is not None:
                for dst, s in zip(self.src_views, src_views):
                    dst.copy_(s, non_blocking=True)
            for dst, s in ((self.tgt, tgt), (self.query_pos, query_pos), (self.reference_points, reference_points)):
                if s is not None:
                    dst.copy_(s.reshape(dst.shape), non_blocking=True)
        return self

    def set_cameras(self, meta):
        """new calibration / crop for the same number of images: refills the packed camera records in place (host packing +
        one small H2D copy); the captured graph reads them through the same pointer."""
        self.ctx.set_cameras(meta, self.dec.layers[0].img_size)
        if self.post is not None:
            self.post.set_cameras(self.ctx.cams, self.V)
        self.meta = meta
        return self

    # ------------------------------------------------------------------ capture / replay
    def _forward(self):
        self.ctx.feat = None          # re-packed from the static source buffers (a no-op for levels produced in place)
        outputs = self.dec(self.tgt, self.reference_points, self.src_views, self.meta, self.spatial_shapes, self.level_start_index,
                           None, query_pos=self.query_pos, threshold=self.thr, context=self.ctx)
        if self.post is not None:
            self.pred = self.post.run(outputs)
        return outputs

    def capture(self, warmup=2):
        with torch.no_grad():
            # the warm-up forwards score whatever is loaded: the accumulators are put back, so a (re-)capture counts no frame
            saved = None if self.post is None else self.post.snapshot()
            for _ in range(max(1, warmup)):         # builds the weight caches, sizes the per-layer buffers
                self._forward()
            if saved is not None:
                self.post.restore(saved)
            torch.cuda.synchronize(self.dev)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.outputs = self._forward()
        self._graph_pred = self.pred            # allocated from the graph's pool: static, like the outputs
        # everything the graph addresses by raw pointer and does not own: the per-layer pyramid products and the cached operands
        self._pinned = self._graph_operands()
        self._captured = self.dec.products.signature()
        return self

    def _graph_operands(self):
        keep = self.ctx.tensors() + self.dec.products.tensors()
        if self.post is not None:
            keep += self.post.tensors()
        for l in self.dec.layers:
            keep += l._wc.tensors() + l.proj_attn._wc.tensors()
        return keep

    def refresh_weights(self):
        """after the decoder's parameters changed: cached operands are version-checked, the graph is re-captured"""
        self.graph = None
        return self.capture()

    def replay(self):
        """one decoder forward on the loaded inputs; returns the graph's static output tensors (overwritten by the next replay)"""
        if self.graph is None or self.dec.products.signature() != self._captured:
            # never captured, or the decoder was run with other shapes / another dtype since (its per-layer buffers were
            # re-allocated): the old graph is still safe to replay (its buffers are pinned) but no longer the decoder's state
            self.capture()
        self.graph.replay()
        self.pred = self._graph_pred
        return self.outputs

    def eager(self):
        """the same forward without the graph (reference for tests; identical results).  With ``postprocess`` it takes the same
        path as the capture: ``pred`` is this call's packed predictions, ``detections`` the same static buffers, and with
        ``evaluation`` the frame is scored into ``evaluator`` like a replayed one, with ``tracking`` it updates ``tracker``."""
        with torch.no_grad():
            return self._forward()
