"""Frame-by-frame inference with the decoder forward captured ONCE as a HIP graph (single GPU).

The reference runs ``model(views, meta)`` eagerly per frame (lib/core/function.py:360-396): ~25 kernel launches per decoder layer,
several host synchronisations.  Here the whole ``DQDecoder.forward`` -- pyramid packing, the side-stream GEMM train, all layers,
triangulation, output stacking -- has static shapes and no host synchronisation, so it is captured once and replayed per frame:
one graph launch on the host (what ``bench.py`` times).  The graph holds raw pointers into its input buffers, the decoder's
weight caches and its per-layer value / G buffers: ``GraphedDecoder`` owns the inputs and, from the capture on, holds a
reference to every one of those tensors (``_pinned``) -- an eager call of the same decoder with another batch, resolution or
compute dtype re-allocates ``ProjAttn._vp / _G`` and rebuilds cache entries, and without the references the graph would go on
reading and writing recycled memory.  ``replay()`` also compares the buffers' addresses with the captured ones and re-captures
when the decoder has moved on to other buffers.

    runner = GraphedDecoder(decoder, meta, spatial_shapes, level_start_index, batch=1, num_queries=1024, threshold=0.1)
    for frame in stream:
        runner.load(src_views=frame.feature_maps, tgt=..., query_pos=..., reference_points=...)   # device copies, no sync
        hs, refs, refs2d, projs2d, class_probs = runner.replay()

Static per runner: the cameras (``meta``; call ``set_cameras`` when they change -- a 960-byte host-packed record per image, no
re-capture), map shapes, batch, query count, threshold and the decoder's weights (``refresh_weights()`` after an optimizer step
or a checkpoint load re-captures).  A backbone that writes its deconvolution outputs into ``runner.pyramid_views`` (channels-last,
compute dtype) makes ``load(src_views=...)`` unnecessary.

``postprocess=dict(dist_thr=0.3, num_nearby_joints_thr=7, max_dets=-1, dets_rows=None)`` continues the captured region behind the
decoder: ``caller.decoder_outputs_to_dict`` -> ``caller.pack_predictions`` (torch ops) -> ``ops.pose_nms`` (classification filter +
nearby-joints NMS, three launches, no synchronisation) into static buffers.  ``replay()`` still returns the five decoder outputs;
``runner.pred`` is the packed predictions (B, NQ, J, 5) and ``runner.detections`` = ``(dets, count, keep)``: the kept rows in keep
order, ``count[b] = [kept, skipped]`` and the kept row indices -- static tensors, overwritten by the next replay:

        runner.replay()
        dets, count, keep = runner.detections
        n = int(count[0, 0])                # the frame's one read-back
        poses = dets[0, :n]                 # (n, J, 5) on the device

``evaluation=dict(kind="panoptic" | "pcp", capacity=..., max_persons=10, actors=4, recall_threshold=500, alpha=0.5)`` (requires
``postprocess``) continues behind the NMS with ``evaluate.DeviceEvaluator.update`` on static ground-truth inputs
(``load(ground_truth=(joints_3d, joints_3d_vis, num_person))``): the kept poses of every replayed frame are scored on the device
and accumulated in ``runner.evaluator``; nothing is read back per frame, the metrics once (``runner.evaluator.panoptic()`` /
``.pcp()``).  The warm-up forwards of a capture leave the accumulators as they were.

``tracking=dict(max_tracks=32, max_dist=500.0, max_misses=10, min_hits=1)`` (requires ``postprocess``) continues behind the NMS
(and behind the evaluator, if there is one; neither reads the other's output) with ``tracking.PoseTracker.update``, one more
launch: every replay associates the kept poses with the tracks of the frames before.  ``runner.track_ids`` = ``(ids, slots)``,
(B, dets_rows) int32 per row of ``runner.detections[0]``, static and overwritten by the next replay; ``runner.tracker`` holds the
state (``.tracks()``, ``.state()``, ``.reset()``).  The warm-up forwards of a capture leave the tracks as they were.  One more
key, ``motion=True`` or ``motion=dict(dt=1.0, q=25.0, r=400.0, v0=2500.0)``, turns on the tracker's constant-velocity motion model
(``tracking.PoseTracker(motion=...)``: two more launches in the graph, the four values fixed at capture): ``runner.track_poses``
(B, dets_rows, J, 3) fp32 is then the filtered pose of every row of ``runner.detections[0]``, static like ``track_ids``.

``track_evaluation=dict(dist_thr=500.0, max_persons=10, max_ids=1024)`` (requires ``tracking``) continues right behind the tracker
with ``tracking.TrackEvaluator.update``, one more launch: the ids of every replayed frame are scored against the ground-truth
identities (``load(ground_truth=(joints_3d, joints_3d_vis, num_person[, person_id]))``, the static inputs ``evaluation`` reads;
a frame with ``num_person < 0`` has no annotation and is skipped) and the CLEAR-MOT counts and the identity overlap table are
accumulated in ``runner.track_evaluator``; ``.report()`` is the one read-back (MOTA, MOTP, IDF1, mostly tracked / lost).  The
warm-up forwards of a capture count no frame.

``refine=dict(bone_lengths=<J-1 values, mm>, n_steps=1, method="ST")`` (requires ``postprocess``) continues behind the NMS with
``structural.StructuralRefiner.update``, two more launches, independent of ``evaluation`` and ``tracking`` (which keep reading
``dets`` unchanged): the kept queries are re-solved from the last layer's 2D points in all views under the given bone lengths of
the 15-joint tree.  ``runner.refined`` = ``(poses (B, dets_rows, J, 3) fp32, status (B, dets_rows) int32)`` per row of
``runner.detections[0]`` (status 0: solved; rows behind the count: zeros, -1) and ``runner.bone_lengths`` (J-1) fp32 are static
tensors: new lengths written into ``runner.bone_lengths`` take effect at the next replay, without re-capture.  The projection
matrices come from the packed camera records and follow ``set_cameras``.
"""
from __future__ import annotations

import torch

from .decoder import DecoderContext


class GraphedDecoder:
    def __init__(self, decoder, meta, spatial_shapes, level_start_index, batch, num_queries, threshold=0.1, device=None,
                 producer_writes_in_place=False, channels=256, postprocess=None, convert_joint_format_indices=None, evaluation=None,
                 tracking=None, refine=None, track_evaluation=None):
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
        self._pinned, self._captured_ptrs = [], None
        # optional device-side post-processing behind the decoder (classification filter + NMS), inside the same graph
        self.NQ, self.J = num_queries, J
        self.convert_joint_format_indices = convert_joint_format_indices
        self.postprocess, self._nms, self.pred, self._graph_pred, self.detections = None, None, None, None, None
        if postprocess is not None:
            from . import ops
            unknown = set(postprocess) - {"dist_thr", "num_nearby_joints_thr", "max_dets", "dets_rows"}
            if unknown:
                raise TypeError("GraphedDecoder: unknown postprocess keys %s" % sorted(unknown))
            self.postprocess = dict(dist_thr=0.3, num_nearby_joints_thr=7, max_dets=-1, dets_rows=None)
            self.postprocess.update(postprocess)
            j_out = J if convert_joint_format_indices is None else len(convert_joint_format_indices)
            if convert_joint_format_indices is not None and not torch.is_tensor(convert_joint_format_indices):
                # a list would be copied to the device inside the captured region (caller.decoder_outputs_to_dict), which a
                # capturing stream refuses: the Shelf / Campus joint map lives on the device from here on
                self.convert_joint_format_indices = torch.as_tensor(list(convert_joint_format_indices), dtype=torch.long, device=dev)
            self._nms = ops.pose_nms_buffers(batch, num_queries, j_out, self.postprocess["dets_rows"], dev)
            self.detections = (self._nms["dets"], self._nms["count"], self._nms["keep"])
        # optional scoring of the kept poses against ground truth behind the NMS, inside the same graph
        self.evaluator, self.ground_truth = None, None
        if evaluation is not None:
            from .evaluate import DeviceEvaluator
            if postprocess is None:
                raise ValueError("GraphedDecoder: evaluation scores the rows the NMS keeps; it requires postprocess")
            unknown = set(evaluation) - {"kind", "capacity", "max_persons", "actors", "recall_threshold", "alpha"}
            if unknown:
                raise TypeError("GraphedDecoder: unknown evaluation keys %s" % sorted(unknown))
            self.evaluator = DeviceEvaluator(device=dev, **evaluation)
            self.ground_truth = self.evaluator.ground_truth_buffers(batch, self._nms["dets"].shape[2])
        # optional person identities across the replayed frames behind the NMS, inside the same graph
        self.tracker, self.track_ids, self.track_poses = None, None, None
        if tracking is not None:
            from .tracking import PoseTracker
            if postprocess is None:
                raise ValueError("GraphedDecoder: tracking follows the rows the NMS keeps; it requires postprocess")
            unknown = set(tracking) - {"max_tracks", "max_dist", "max_misses", "min_hits", "motion"}
            if unknown:
                raise TypeError("GraphedDecoder: unknown tracking keys %s" % sorted(unknown))
            dets = self._nms["dets"]
            self.tracker = PoseTracker(batch=batch, rows=dets.shape[1], num_joints=dets.shape[2], device=dev, **tracking)
            self.track_ids = (self.tracker.buffers["ids"], self.tracker.buffers["slots"])
            self.track_poses = self.tracker.row_poses       # None without tracking["motion"]
        # optional scoring of the track ids against ground truth identities right behind the tracker, inside the same graph
        self.track_evaluator, self.person_id = None, None
        if track_evaluation is not None:
            from .tracking import TrackEvaluator
            if tracking is None:
                raise ValueError("GraphedDecoder: track_evaluation scores the ids of the tracker; it requires tracking")
            unknown = set(track_evaluation) - {"dist_thr", "max_persons", "max_ids"}
            if unknown:
                raise TypeError("GraphedDecoder: unknown track_evaluation keys %s" % sorted(unknown))
            given = dict(track_evaluation)
            if self.evaluator is not None:      # one set of ground-truth buffers serves both: the evaluator's person slots
                given.setdefault("max_persons", self.evaluator.max_persons)
                if given["max_persons"] < self.evaluator.max_persons:
                    raise ValueError("GraphedDecoder: track_evaluation max_persons = %d below the %d person slots of evaluation"
                                     % (given["max_persons"], self.evaluator.max_persons))
            self.track_evaluator = TrackEvaluator(batch=batch, device=dev, **given)
            fresh = self.track_evaluator.ground_truth_buffers(batch, self._nms["dets"].shape[2])
            if self.ground_truth is None:
                self.ground_truth = fresh[:3]
            self._slot_identity = fresh[3][:, :self.ground_truth[0].shape[1]].contiguous()      # slot g = identity g
            self.person_id = self._slot_identity.clone()
        # optional structural triangulation of the kept queries (fixed bone lengths) behind the NMS, inside the same graph
        self.refiner, self.refined, self.bone_lengths, self._Pm = None, None, None, None
        if refine is not None:
            from .geometry_torch import proj_matrices_from_records
            from .structural import PANOPTIC15_PARENT, StructuralRefiner
            if postprocess is None:
                raise ValueError("GraphedDecoder: refine re-solves the rows the NMS keeps; it requires postprocess")
            unknown = set(refine) - {"bone_lengths", "n_steps", "method"}
            if unknown:
                raise TypeError("GraphedDecoder: unknown refine keys %s" % sorted(unknown))
            if convert_joint_format_indices is not None or J != len(PANOPTIC15_PARENT):
                raise ValueError("GraphedDecoder: refine solves on the 15-joint tree of the decoder's own joints; it cannot be "
                                 "combined with convert_joint_format_indices")
            rows = self._nms["dets"].shape[1]
            if rows > num_queries:              # postprocess["dets_rows"] is the caller's: keep has num_queries columns, no more
                raise ValueError("GraphedDecoder: refine with dets_rows = %d > num_queries = %d" % (rows, num_queries))
            self.refiner = StructuralRefiner(batch=batch, rows=rows, parent=PANOPTIC15_PARENT, device=dev, **refine)
            self.refined = (self.refiner.poses, self.refiner.status)
            self.bone_lengths = self.refiner.bone_lengths
            self._Pm = proj_matrices_from_records(self.ctx.cams, self.V, batch).contiguous()

    # ------------------------------------------------------------------ inputs (device-side copies on the current stream)
    def load(self, src_views=None, tgt=None, query_pos=None, reference_points=None, ground_truth=None):
        """ground_truth = (joints_3d (B, G, J, 3), joints_3d_vis (B, G, J), num_person (B)) with G <= max_persons, for a runner
        built with ``evaluation`` or ``track_evaluation``: copied into the static inputs both read; person slots behind G are not
        scored.  An optional fourth element person_id (B, G) int32 gives the slots' identities to ``track_evaluation`` (without
        it, slot g is identity g); num_person < 0 marks a frame without annotation, which ``track_evaluation`` skips."""
        with torch.no_grad():
            if ground_truth is not None:
                if self.evaluator is None and self.track_evaluator is None:
                    raise ValueError("GraphedDecoder: ground_truth needs a runner built with evaluation=dict(...) or "
                                     "track_evaluation=dict(...)")
                j3d, vis, num = ground_truth[:3]
                if len(ground_truth) > 3 and self.track_evaluator is None:
                    raise ValueError("GraphedDecoder: person_id needs a runner built with track_evaluation=dict(...)")
                if j3d.shape[1] > self.ground_truth[0].shape[1]:
                    raise ValueError("GraphedDecoder: %d person slots, built for max_persons = %d"
                                     % (j3d.shape[1], self.ground_truth[0].shape[1]))
                if self.person_id is not None:
                    self.person_id.copy_(self._slot_identity)
                    if len(ground_truth) > 3 and ground_truth[3] is not None:
                        self.person_id[:, :j3d.shape[1]].copy_(ground_truth[3], non_blocking=True)
                self.ground_truth[0][:, :j3d.shape[1]].copy_(j3d, non_blocking=True)
                self.ground_truth[1][:, :vis.shape[1]].copy_(vis, non_blocking=True)
                self.ground_truth[2].copy_(num, non_blocking=True)
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
        fresh = DecoderContext.prepare(self.spatial_shapes, self.level_start_index, meta, self.dec.layers[0].img_size, self.dtype,
                                       self.tgt.shape[0], self.dev)
        if fresh.cams.shape != self.ctx.cams.shape:
            raise RuntimeError("set_cameras: %s camera records, the runner was built for %s"
                               % (tuple(fresh.cams.shape), tuple(self.ctx.cams.shape)))
        self.ctx.cams.copy_(fresh.cams)
        if self._Pm is not None:
            from .geometry_torch import proj_matrices_from_records
            self._Pm.copy_(proj_matrices_from_records(self.ctx.cams, self.V, self.tgt.shape[0]))
        self.meta = meta
        return self

    # ------------------------------------------------------------------ capture / replay
    def _forward(self):
        self.ctx.feat = None          # re-packed from the static source buffers (a no-op for levels produced in place)
        outputs = self.dec(self.tgt, self.reference_points, self.src_views, self.meta, self.spatial_shapes, self.level_start_index,
                           None, query_pos=self.query_pos, threshold=self.thr, context=self.ctx)
        if self.postprocess is not None:
            from . import caller, ops
            out = caller.decoder_outputs_to_dict(*outputs, self.NQ, self.J, self.convert_joint_format_indices)
            self.pred = caller.pack_predictions(out, self.thr)                       # function.py:386-396
            pp = self.postprocess
            ops.pose_nms(self.pred, pp["dist_thr"], pp["num_nearby_joints_thr"], pp["max_dets"], pp["dets_rows"], out=self._nms)
            if self.evaluator is not None:
                self.evaluator.update(self._nms["dets"], self._nms["count"], *self.ground_truth)
            if self.tracker is not None:
                self.tracker.update(self._nms["dets"], self._nms["count"])
            if self.track_evaluator is not None:
                self.track_evaluator.update(self.tracker, self._nms["dets"], self._nms["count"], *self.ground_truth,
                                            person_id=self.person_id)
            if self.refiner is not None:
                self.refiner.update(outputs[2][-1], self.ctx.cams, self._Pm, self._nms["keep"], self._nms["count"])
        return outputs

    def capture(self, warmup=2):
        with torch.no_grad():
            # the warm-up forwards score whatever is loaded: the accumulators are put back, so a (re-)capture counts no frame
            saved = None if self.evaluator is None else {k: t.clone() for k, t in self.evaluator.buffers.items()}
            tracks = None if self.tracker is None else self.tracker.snapshot()      # nor do they age or create tracks
            scores = None if self.track_evaluator is None else self.track_evaluator.snapshot()
            for _ in range(max(1, warmup)):         # builds the weight caches, sizes the per-layer buffers
                self._forward()
            if scores is not None:
                self.track_evaluator.restore(scores)
            if saved is not None:
                for k, t in self.evaluator.buffers.items():
                    t.copy_(saved[k])
            if tracks is not None:
                self.tracker.restore(tracks)
            torch.cuda.synchronize(self.dev)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.outputs = self._forward()
        self._graph_pred = self.pred            # allocated from the graph's pool: static, like the outputs
        # everything the graph addresses by raw pointer and does not own: the per-layer pyramid products and the cached operands
        self._pinned = self._graph_operands()
        self._captured_ptrs = self._buffer_ptrs()
        return self

    def _buffer_ptrs(self):
        return tuple((None if t is None else (t.data_ptr(), t.dtype, tuple(t.shape)))
                     for l in self.dec.layers for t in (l.proj_attn._vp, l.proj_attn._G))

    def _graph_operands(self):
        keep = [self.ctx.cams, self.ctx.feat, getattr(self.ctx, "_buffer", None)]
        if self._nms is not None:
            keep += list(self._nms.values())
        if self.evaluator is not None:
            keep += list(self.evaluator.buffers.values()) + list(self.ground_truth)
        if self.track_evaluator is not None:
            keep += list(self.track_evaluator.buffers.values()) + list(self.ground_truth) + [self.person_id]
        if self.tracker is not None:
            keep += list(self.tracker.buffers.values()) + list((self.tracker.motion_buffers or {}).values())
        if self.refiner is not None:
            keep += list(self.refiner.buffers.values()) + [self.refiner.bone_lengths, self._Pm]
        for l in self.dec.layers:
            keep += [l.proj_attn._vp, l.proj_attn._G]
            for wc in (l._wc, l.proj_attn._wc):
                keep += [entry[1] for entry in wc._store.values()]
        return [t for t in keep if t is not None]

    def refresh_weights(self):
        """after the decoder's parameters changed: cached operands are version-checked, the graph is re-captured"""
        self.graph = None
        return self.capture()

    def replay(self):
        """one decoder forward on the loaded inputs; returns the graph's static output tensors (overwritten by the next replay)"""
        if self.graph is None or self._buffer_ptrs() != self._captured_ptrs:
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
