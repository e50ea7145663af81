"""Persistent person identities for the serving path: ``PoseTracker`` associates the poses ``ops.pose_nms`` keeps in a frame with
the tracks of the frames before, on the device (``ops.track_update``, csrc/track.hip: one launch per frame).

The association is a minimum-cost assignment between the live tracks and the frame's detections, cost = mean joint distance to
the track's last pose, where a pair further apart than ``max_dist`` costs ``max_dist`` -- what leaving both unmatched costs -- so
the matching is the global optimum, not a greedy nearest choice.  A matched track takes the detection's pose and score; an
unmatched track ages and is dropped after more than ``max_misses`` misses in a row; an unmatched detection opens a track in the
lowest free slot, with the stream's next id.  There is no re-identification of a dropped track.

    tracker = PoseTracker(batch=1, rows=1024, num_joints=15, max_tracks=32)
    for frame in stream:
        _, count, dets = ops.pose_nms(pred, out=nms)
        ids, slots = tracker.update(dets, count)          # static (B, R) int32 tensors, nothing read back
    tracker.tracks()                                      # one read-back: the live tracks of every stream

``motion=True`` (or a dict with ``dt, q, r, v0``) puts a constant-velocity Kalman filter around the update, two more launches per
frame (``ops.track_predict`` before it, ``ops.track_correct`` behind it): every track carries a position and a velocity per joint
and axis and one 2 x 2 covariance; the update associates against the PREDICTED poses, a matched track's pose is the filtered one,
an unmatched track coasts on at its velocity.  ``tracker.row_poses`` (B, R, J, 3) is the filtered pose of every row of ``dets``,
``tracker.motion()`` reads velocities and covariances back.  Without ``motion`` nothing else is launched or allocated.

``update`` has fixed shapes and launches only, so it can be captured in a HIP graph (``serving.GraphedDecoder(tracking=...)``).
"""
from __future__ import annotations

import collections
import contextlib
import math

import torch

__all__ = ["PoseTracker", "Track"]

Track = collections.namedtuple("Track", "id slot hits misses born score pose")

MOTION_DEFAULTS = dict(dt=1.0, q=25.0, r=400.0, v0=2500.0)


class PoseTracker:
    """batch: independent streams (batch elements); rows: R of the ``dets`` (B, R, J, 5) it will be given; max_tracks <= 64 slots
    per stream; max_dist in the unit of the poses (mm; 500 is the recall distance of the evaluation); a track's id is reported
    once it has ``min_hits`` hits (``slots`` reports it from its first frame).

    motion: None (no motion model), True, or a dict with keys from dt (time between two updates; 1.0 = a frame), q (variance of
    the random acceleration, unit^2 / dt^4), r (variance of a detected coordinate, unit^2) and v0 (variance of a new track's
    velocity, unit^2 / dt^2).  The defaults -- 25.0, 400.0 and 2500.0: accelerations of 5 mm / frame^2, detections good to 20 mm,
    people no faster than about 50 mm per frame -- are a CHOICE made for poses in mm at video rate, not a measurement: they were
    tuned on no recorded sequence, and no accuracy is claimed for them."""

    def __init__(self, batch=1, rows=1024, num_joints=15, max_tracks=32, max_dist=500.0, max_misses=10, min_hits=1, device="cuda",
                 motion=None):
        from . import ops
        self.batch, self.rows, self.num_joints, self.max_tracks = int(batch), int(rows), int(num_joints), int(max_tracks)
        self.max_dist, self.max_misses, self.min_hits = float(max_dist), int(max_misses), int(min_hits)
        if not (0.0 <= self.max_dist <= ops.LAP_BIG) or self.max_misses < 0 or self.min_hits < 0:
            raise ValueError("PoseTracker: 0 <= max_dist <= %g, max_misses >= 0 and min_hits >= 0 expected (got %r, %r, %r)"
                             % (ops.LAP_BIG, max_dist, max_misses, min_hits))
        self.motion_params = None
        if motion is not None and motion is not False:
            given = {} if motion is True else dict(motion)
            unknown = set(given) - set(MOTION_DEFAULTS)
            if unknown:
                raise TypeError("PoseTracker: unknown motion keys %s" % sorted(unknown))
            p = {k: float(given.get(k, v)) for k, v in MOTION_DEFAULTS.items()}
            if not (0.0 < p["dt"] < math.inf and 0.0 <= p["q"] <= ops.LAP_BIG and 0.0 < p["r"] <= ops.LAP_BIG
                    and 0.0 <= p["v0"] <= ops.LAP_BIG):
                raise ValueError("PoseTracker: motion needs a finite dt > 0, 0 <= q, 0 < r and 0 <= v0, none above %g (got %r)"
                                 % (ops.LAP_BIG, p))
            self.motion_params = p
        self.device = torch.device(device)
        self.buffers = ops.track_buffers(self.batch, self.max_tracks, self.num_joints, self.rows, self.device)
        self.motion_buffers = None if self.motion_params is None else \
            ops.track_motion_buffers(self.batch, self.max_tracks, self.num_joints, self.rows, self.device)

    @property
    def row_poses(self):
        """(B, R, J, 3) fp32, static: the filtered pose of every row of the last ``dets``, zeros for rows without a track; None
        without the motion model"""
        return None if self.motion_buffers is None else self.motion_buffers["row_pose"]

    def update(self, dets, count=None):
        """dets (B, R, J, 5) fp32 and count (B, 2) int32 or None as ``ops.pose_nms`` leaves them -> (ids, slots), (B, R) int32,
        static tensors that the next update overwrites.  Launches only: one, or three with the motion model (predict, the same
        update, correct)."""
        from . import ops
        with torch.cuda.device(dets.device) if dets.is_cuda else contextlib.nullcontext():
            if self.motion_params is None:
                return ops.track_update(dets, count, self.buffers, self.max_dist, self.max_misses, self.min_hits)
            p = self.motion_params
            ops.track_predict(self.buffers, self.motion_buffers, p["dt"], p["q"])
            out = ops.track_update(dets, count, self.buffers, self.max_dist, self.max_misses, self.min_hits)
            ops.track_correct(self.buffers, self.motion_buffers, p["r"], p["v0"])
            return out

    def _all_buffers(self):
        return dict(self.buffers, **(self.motion_buffers or {}))

    def reset(self):
        """forget every track and counter (device fills)"""
        for k, t in self._all_buffers().items():
            t.fill_(-1 if k in ("id", "ids", "slots") else 0)
        return self

    def snapshot(self):
        """clones of the state buffers, the motion model's included (``restore`` puts them back: a graph capture's warm-up
        forwards must not age tracks)"""
        return {k: t.clone() for k, t in self._all_buffers().items()}

    def restore(self, saved):
        for k, t in self._all_buffers().items():
            t.copy_(saved[k])
        return self

    def state(self):
        """the named counters of the state block as ints (a read-back)"""
        from . import ops
        return dict(zip(ops.TRACK_STATE, self.buffers["state"].cpu().tolist()))

    def tracks(self):
        """one read-back -> per batch element the live tracks in slot order, each a Track(id, slot, hits, misses, born, score, pose
        (J, 3) numpy fp32); with the motion model the pose is the filtered one (the prediction, for a track that missed)"""
        keys = ("id", "hits", "misses", "born", "score", "pose")
        host = {k: self.buffers[k].cpu().numpy() for k in keys}
        return [[Track(int(host["id"][b, t]), t, int(host["hits"][b, t]), int(host["misses"][b, t]), int(host["born"][b, t]),
                       float(host["score"][b, t]), host["pose"][b, t].copy())
                 for t in range(self.max_tracks) if host["id"][b, t] >= 0] for b in range(self.batch)]

    def motion(self):
        """one read-back -> per batch element {slot: (velocity (J, 3) numpy fp64 in unit / dt, (pxx, pxv, pvv))} of the live tracks"""
        if self.motion_buffers is None:
            raise RuntimeError("PoseTracker.motion: built without motion=")
        packed = torch.cat([self.buffers["id"].double().reshape(-1), self.motion_buffers["var"].reshape(-1),
                            self.motion_buffers["mean"][:, :, :, 1].reshape(-1)]).cpu().numpy()
        B, T, J = self.batch, self.max_tracks, self.num_joints
        ident = packed[:B * T].reshape(B, T)
        var = packed[B * T:4 * B * T].reshape(B, T, 3)
        vel = packed[4 * B * T:].reshape(B, T, J, 3)
        return [{t: (vel[b, t].copy(), tuple(float(p) for p in var[b, t])) for t in range(T) if ident[b, t] >= 0} for b in range(B)]
