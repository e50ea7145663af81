"""Everything that runs behind ``DQDecoder.forward`` on the device, as one object: ``PostProcess`` owns the option checking, the
static buffers, the ground-truth inputs, the launch order and the save / restore of whatever accumulates.  It is the only place
in the package where the chain is written; ``serving.GraphedDecoder`` captures ``run`` into its HIP graph behind the decoder and
``validate --graph 0`` calls ``run_packed`` behind the eager head.

    post = PostProcess(batch=1, num_queries=1024, num_joints=15, threshold=0.1, device="cuda", postprocess={}, tracking={})
    post.set_cameras(cams, V)                       # packed camera records (ops.pack_cameras); only ``refine`` reads them
    post.load_ground_truth((joints_3d, joints_3d_vis, num_person))      # only with ``evaluation`` / ``track_evaluation``
    pred = post.run(decoder_outputs)                # launches only: no synchronisation, fixed shapes
    dets, count, keep = post.detections

A stage is an object with ``update(...)`` (launches only, fixed shapes), ``tensors()`` (every device tensor ``update`` addresses
besides its arguments) and, if it accumulates over frames, ``snapshot()`` / ``restore(saved)``.  A new stage is added in ONE place,
the constructor below: its keys in ``OPTIONS``, then its object, its launch and the static tensors it publishes.

``postprocess=dict(dist_thr=0.3, num_nearby_joints_thr=7, max_dets=-1, dets_rows=None)``: ``caller.decoder_outputs_to_dict`` ->
``caller.pack_predictions`` (torch ops) -> ``ops.pose_nms`` (classification filter + nearby-joints NMS, three launches) into
static buffers.  ``run`` returns the packed predictions (B, NQ, J, 5); ``detections`` = ``(dets, count, keep)``: the kept rows in
keep order, ``count[b] = [kept, skipped]`` and the kept row indices -- static tensors, overwritten by the next run.

``evaluation=dict(kind="panoptic" | "pcp", capacity=..., max_persons=10, actors=4, recall_threshold=500, alpha=0.5)`` (requires
``postprocess``) continues behind the NMS with ``evaluate.DeviceEvaluator.update`` on the static ground-truth inputs: the kept
poses of every frame are scored on the device and accumulated in ``evaluator``; nothing is read back per frame, the metrics once
(``evaluator.panoptic()`` / ``.pcp()``).

``tracking=dict(max_tracks=32, max_dist=500.0, max_misses=10, min_hits=1)`` (requires ``postprocess``) continues behind the NMS
(and behind the evaluator, if there is one; neither reads the other's output) with ``tracking.PoseTracker.update``, one more
launch: every run associates the kept poses with the tracks of the frames before.  ``track_ids`` = ``(ids, slots)``,
(B, dets_rows) int32 per row of ``detections[0]``, static and overwritten by the next run; ``tracker`` holds the state
(``.tracks()``, ``.state()``, ``.reset()``).  One more key, ``motion=True`` or ``motion=dict(dt=1.0, q=25.0, r=400.0, v0=2500.0)``,
turns on the tracker's constant-velocity motion model (two more launches, the four values fixed at construction):
``track_poses`` (B, dets_rows, J, 3) fp32 is then the filtered pose of every row of ``detections[0]``, static like ``track_ids``.

``track_evaluation=dict(dist_thr=500.0, max_persons=10, max_ids=1024)`` (requires ``tracking``) continues right behind the tracker
with ``tracking.TrackEvaluator.update``, one more launch: the ids of every frame are scored against the ground-truth identities
(the static inputs ``evaluation`` reads, plus ``person_id``; a frame with ``num_person < 0`` has no annotation and is skipped) and
the CLEAR-MOT counts and the identity overlap table are accumulated in ``track_evaluator``; ``.report()`` is the one read-back
(MOTA, MOTP, IDF1, mostly tracked / lost).  With ``evaluation`` as well there is one set of ground-truth tensors, with the
evaluator's person slots: ``max_persons`` defaults to the evaluator's and may not be below it.

``refine=dict(bone_lengths=<J-1 values, mm>, n_steps=1, method="ST")`` (requires ``postprocess``) continues behind the NMS with
``structural.StructuralRefiner.update``, two more launches, independent of ``evaluation`` and ``tracking`` (which keep reading
``dets`` unchanged): the kept queries are re-solved from the last layer's 2D points in all views under the given bone lengths of
the 15-joint tree.  ``refined`` = ``(poses (B, dets_rows, J, 3) fp32, status (B, dets_rows) int32)`` per row of ``detections[0]``
(status 0: solved; rows behind the count: zeros, -1) and ``bone_lengths`` (J-1) fp32 are static tensors: new lengths written into
``bone_lengths`` take effect at the next run.  The projection matrices ``Pm`` come from the packed camera records and follow
``set_cameras``.  With a live-view table (``set_live_views``: the decoder context's, ``serving.GraphedDecoder(live_views=True)``) the
solver gets view weights ``conf`` (B, V, NQ*J) fp32 -- ``1 / n_live[b]`` for the live views of stream b, 0 for the others, built from
the table by launches -- so that a dead view's (zero) 2D points add exact zeros to its sums.

``refine=dict(bone_lengths="track", window=8, min_frames=4, fallback=None | <J-1 values>, n_steps=1, method="ST")`` (requires
``tracking`` as well) puts ``structural.BoneLengthEstimator.update`` behind the tracker (and ``track_evaluation``) and in front of
the refiner, one more launch: every track's bone lengths are the median over its last ``window`` raw detections, and a row is
solved under its own track's lengths once the track has ``min_frames`` samples, until then under ``fallback`` or, without one,
the lengths the row has itself.  ``bone_lengths`` is then the (B, dets_rows, J-1) fp32 row tensor the solver reads,
``bone_source`` (B, dets_rows) int32 where each row's lengths came from (0 track, 1 fallback, 2 the row itself, -1 no detection)
and ``bone_estimator`` holds the histories (``.lengths()``, ``.reset()``).
"""
from __future__ import annotations

import torch

NMS_DEFAULTS = dict(dist_thr=0.3, num_nearby_joints_thr=7, max_dets=-1, dets_rows=None)
# option -> (its allowed keys, the option it cannot do without, why)
OPTIONS = {
    "postprocess": (set(NMS_DEFAULTS), None, None),
    "evaluation": ({"kind", "capacity", "max_persons", "actors", "recall_threshold", "alpha"}, "postprocess",
                   "evaluation scores the rows the NMS keeps"),
    "tracking": ({"max_tracks", "max_dist", "max_misses", "min_hits", "motion"}, "postprocess",
                 "tracking follows the rows the NMS keeps"),
    "track_evaluation": ({"dist_thr", "max_persons", "max_ids"}, "tracking", "track_evaluation scores the ids of the tracker"),
    "refine": ({"bone_lengths", "n_steps", "method", "window", "min_frames", "fallback"}, "postprocess",
               "refine re-solves the rows the NMS keeps"),
}
# refine's bone_lengths="track" and the keys that belong to it alone
TRACK_LENGTHS = "track"
TRACK_LENGTH_KEYS = ("window", "min_frames", "fallback")


def check_options(given):
    """given: option name -> dict or None, for every name of OPTIONS"""
    for name, (allowed, needs, why) in OPTIONS.items():
        if given[name] is None:
            continue
        if needs is not None and given[needs] is None:
            raise ValueError("PostProcess: %s; it requires %s" % (why, needs))
        unknown = set(given[name]) - allowed
        if unknown:
            raise TypeError("PostProcess: unknown %s keys %s" % (name, sorted(unknown)))
    if given["postprocess"] is None:
        raise ValueError("PostProcess: nothing to run; it requires postprocess")
    refine = given["refine"]
    if refine is not None:
        lengths = refine.get("bone_lengths")
        if isinstance(lengths, str):
            if lengths != TRACK_LENGTHS:
                raise ValueError("PostProcess: refine bone_lengths = %r; the one name it knows is %r" % (lengths, TRACK_LENGTHS))
            if given["tracking"] is None:
                raise ValueError("PostProcess: refine with bone_lengths = %r estimates the lengths per track; it requires tracking"
                                 % TRACK_LENGTHS)
        else:
            stray = sorted(k for k in TRACK_LENGTH_KEYS if k in refine)
            if stray:
                raise TypeError("PostProcess: refine keys %s belong to bone_lengths = %r" % (stray, TRACK_LENGTHS))


class PostProcess:
    def __init__(self, batch, num_queries, num_joints, threshold, device, postprocess=None, convert_joint_format_indices=None,
                 evaluation=None, tracking=None, track_evaluation=None, refine=None):
        from . import ops
        check_options(dict(postprocess=postprocess, evaluation=evaluation, tracking=tracking, track_evaluation=track_evaluation,
                           refine=refine))
        dev = torch.device(device)
        self.NQ, self.J, self.thr = num_queries, num_joints, float(threshold)
        self.postprocess = dict(NMS_DEFAULTS, **postprocess)
        j_out = num_joints if convert_joint_format_indices is None else len(convert_joint_format_indices)
        if convert_joint_format_indices is not None and not torch.is_tensor(convert_joint_format_indices):
            # a list would be copied to the device inside the captured region (caller.decoder_outputs_to_dict), which a
            # capturing stream refuses: the Shelf / Campus joint map lives on the device from here on
            convert_joint_format_indices = torch.as_tensor(list(convert_joint_format_indices), dtype=torch.long, device=dev)
        self.convert_joint_format_indices = convert_joint_format_indices
        self.nms = ops.pose_nms_buffers(batch, num_queries, j_out, self.postprocess["dets_rows"], dev)
        dets, count, keep = self.detections = (self.nms["dets"], self.nms["count"], self.nms["keep"])
        rows = dets.shape[1]
        self.stages = []                            # (stage object, its launch: refs2d -> None) in launch order
        self.cams, self.Pm = None, None             # set_cameras
        self.live = None                            # set_live_views
        # scoring of the kept poses against ground truth
        self.evaluator = None
        if evaluation is not None:
            from .evaluate import DeviceEvaluator
            self.evaluator = DeviceEvaluator(device=dev, **evaluation)
            self.stages.append((self.evaluator, lambda refs2d: self.evaluator.update(dets, count, *self.ground_truth)))
        # person identities across the frames
        self.tracker, self.track_ids, self.track_poses = None, None, None
        if tracking is not None:
            from .tracking import PoseTracker
            self.tracker = PoseTracker(batch=batch, rows=rows, num_joints=j_out, device=dev, **tracking)
            self.track_ids = (self.tracker.buffers["ids"], self.tracker.buffers["slots"])
            self.track_poses = self.tracker.row_poses       # None without tracking["motion"]
            self.stages.append((self.tracker, lambda refs2d: self.tracker.update(dets, count)))
        # scoring of the track ids against ground truth identities, right behind the tracker
        self.track_evaluator = None
        if track_evaluation is not None:
            from .tracking import TrackEvaluator
            given = dict(track_evaluation)
            if self.evaluator is not None:      # one set of ground-truth buffers serves both: the evaluator's person slots
                given.setdefault("max_persons", self.evaluator.max_persons)
                if given["max_persons"] < self.evaluator.max_persons:
                    raise ValueError("PostProcess: track_evaluation max_persons = %d below the %d person slots of evaluation"
                                     % (given["max_persons"], self.evaluator.max_persons))
            self.track_evaluator = TrackEvaluator(batch=batch, device=dev, **given)
            self.stages.append((self.track_evaluator, lambda refs2d: self.track_evaluator.update(
                self.tracker, dets, count, *self.ground_truth, person_id=self.person_id)))
        # structural triangulation of the kept queries (fixed bone lengths)
        self.refiner, self.refined, self.bone_lengths = None, None, None
        self.bone_estimator, self.bone_source = None, None
        if refine is not None:
            from .structural import PANOPTIC15_PARENT, BoneLengthEstimator, StructuralRefiner
            if convert_joint_format_indices is not None or num_joints != len(PANOPTIC15_PARENT):
                raise ValueError("PostProcess: refine solves on the 15-joint tree of the decoder's own joints; it cannot be "
                                 "combined with convert_joint_format_indices")
            if rows > num_queries:              # postprocess["dets_rows"] is the caller's: keep has num_queries columns, no more
                raise ValueError("PostProcess: refine with dets_rows = %d > num_queries = %d" % (rows, num_queries))
            refine = dict(refine)
            if isinstance(refine.get("bone_lengths"), str):         # check_options: it is TRACK_LENGTHS and there is a tracker
                # the lengths of every row's track, estimated behind the tracker (and its scorer) and in front of the refiner
                given = {k: refine.pop(k) for k in TRACK_LENGTH_KEYS if k in refine}
                self.bone_estimator = BoneLengthEstimator(batch=batch, rows=rows, max_tracks=self.tracker.max_tracks,
                                                          parent=PANOPTIC15_PARENT, device=dev, **given)
                self.bone_source = self.bone_estimator.row_source
                refine["bone_lengths"] = self.bone_estimator.row_length
                self.stages.append((self.bone_estimator, lambda refs2d: self.bone_estimator.update(dets, count, self.tracker)))
            self.refiner = StructuralRefiner(batch=batch, rows=rows, parent=PANOPTIC15_PARENT, device=dev, **refine)
            self.refined = (self.refiner.poses, self.refiner.status)
            self.bone_lengths = self.refiner.bone_lengths
            self.stages.append((self.refiner, lambda refs2d: self.refiner.update(refs2d, self.cams, self.Pm, keep, count,
                                                                                 conf=self.view_weights(refs2d))))
        # the static ground-truth inputs, shared by the two scorers: slot g is identity g until load_ground_truth says otherwise
        self.ground_truth, self.person_id = None, None
        scorer = self.evaluator or self.track_evaluator
        if scorer is not None:
            self.ground_truth = scorer.ground_truth_buffers(batch, j_out)[:3]
        if self.track_evaluator is not None:
            self.person_id = torch.arange(self.ground_truth[0].shape[1], dtype=torch.int32, device=dev).repeat(batch, 1)

    # ------------------------------------------------------------------ inputs (device-side copies on the current stream)
    def load_ground_truth(self, ground_truth):
        """ground_truth = (joints_3d (B, G, J, 3), joints_3d_vis (B, G, J), num_person (B)) with G <= max_persons, for a pipeline
        built with ``evaluation`` or ``track_evaluation``: copied into the static inputs both read; person slots behind G are not
        scored.  An optional fourth element person_id (B, G) int32 gives the slots' identities to ``track_evaluation`` (without
        it, slot g is identity g); num_person < 0 marks a frame without annotation, which ``track_evaluation`` skips."""
        if self.ground_truth is None:
            raise ValueError("PostProcess: ground_truth needs a runner built with evaluation=dict(...) or "
                             "track_evaluation=dict(...)")
        j3d, vis, num = ground_truth[:3]
        if len(ground_truth) > 3 and self.track_evaluator is None:
            raise ValueError("PostProcess: person_id needs a runner built with track_evaluation=dict(...)")
        if j3d.shape[1] > self.ground_truth[0].shape[1]:
            raise ValueError("PostProcess: %d person slots, built for max_persons = %d"
                             % (j3d.shape[1], self.ground_truth[0].shape[1]))
        with torch.no_grad():
            if self.person_id is not None:
                self.person_id.copy_(torch.arange(self.person_id.shape[1], dtype=torch.int32, device=self.person_id.device))
                if len(ground_truth) > 3 and ground_truth[3] is not None:
                    self.person_id[:, :j3d.shape[1]].copy_(ground_truth[3], non_blocking=True)
            self.ground_truth[0][:, :j3d.shape[1]].copy_(j3d, non_blocking=True)
            self.ground_truth[1][:, :vis.shape[1]].copy_(vis, non_blocking=True)
            self.ground_truth[2].copy_(num, non_blocking=True)
        return self

    def set_cameras(self, cams, V):
        """cams: the packed camera records (V * B, CAM_STRIDE) the refiner un-distorts with, kept by reference; its static
        projection matrices ``Pm`` (B, V, 3, 4) are refilled from them in place (the same pointer from the first call on)"""
        self.cams = cams
        if self.refiner is not None:
            from .geometry_torch import proj_matrices_from_records
            fresh = proj_matrices_from_records(cams, V, self.refiner.batch)
            if self.Pm is None:
                self.Pm = fresh.contiguous()
            else:
                self.Pm.copy_(fresh)
        return self

    def set_live_views(self, live):
        """live: the decoder context's live-view table (``DecoderContext.live``: view_idx (B, V) i32, n_live (B) i32 on the device),
        kept by reference, or None; only ``refine`` reads it (``view_weights``)"""
        if live is not None:
            view_idx, n_live = live
            if (view_idx.dtype != torch.int32 or n_live.dtype != torch.int32 or view_idx.dim() != 2
                    or tuple(n_live.shape) != (view_idx.shape[0],)):
                raise ValueError("PostProcess: live = (view_idx (B, V) int32, n_live (B) int32) expected")
        self.live = live
        return self

    def view_weights(self, refs2d):
        """the refiner's conf (B, V, NQ*J) fp32 from the live-view table -- 1 / n_live[b] (an fp32 division) for the live views of
        stream b, 0 for the others -- or None without a table.  Torch launches on the table's device tensors: no read-back."""
        if self.live is None:
            return None
        view_idx, n_live = self.live
        B, V, Lq = refs2d.shape[:3]
        if tuple(view_idx.shape) != (B, V):
            raise ValueError("PostProcess: live-view table for %s, 2D points of (%d, %d)" % (tuple(view_idx.shape), B, V))
        views = torch.arange(V, dtype=torch.int32, device=view_idx.device)
        live = (view_idx.unsqueeze(2) == views.view(1, 1, V)).any(1)                  # (B, V): view v is in the row of stream b
        w = live.to(torch.float32) / n_live.to(torch.float32).unsqueeze(1)
        return w.unsqueeze(2).expand(B, V, Lq).contiguous()

    # ------------------------------------------------------------------ the chain: launches only
    def run(self, outputs):
        """the five outputs of ``DQDecoder.forward`` -> the packed predictions (B, NQ, J, 5), every stage launched behind them"""
        from . import caller
        out = caller.decoder_outputs_to_dict(*outputs, self.NQ, self.J, self.convert_joint_format_indices)
        return self.run_packed(caller.pack_predictions(out, self.thr), outputs[2][-1])                # function.py:386-396

    def run_packed(self, pred, refs2d):
        """for a caller that has them already (``caller.DecoderHead.forward``): pred (B, NQ, J, 5) contiguous as
        ``caller.pack_predictions`` leaves it and the last layer's 2D points (B, V, NQ*J, 2), which only ``refine`` reads"""
        from . import ops
        pp = self.postprocess
        ops.pose_nms(pred, pp["dist_thr"], pp["num_nearby_joints_thr"], pp["max_dets"], pp["dets_rows"], out=self.nms)
        for _, launch in self.stages:
            launch(refs2d)
        return pred

    # ------------------------------------------------------------------ what a graph capture needs
    def snapshot(self):
        """the state of every stage that accumulates: a capture's warm-up forwards score, age and count whatever is loaded"""
        return [(s, s.snapshot()) for s, _ in self.stages if hasattr(s, "snapshot")]

    def restore(self, saved):
        for stage, state in saved:
            stage.restore(state)
        return self

    def tensors(self):
        """every device tensor a captured ``run`` addresses by raw pointer and does not allocate itself"""
        own = list(self.nms.values()) + list(self.ground_truth or ()) + [self.person_id, self.Pm] + list(self.live or ())
        return [t for t in own + [t for s, _ in self.stages for t in s.tensors()] if t is not None]
