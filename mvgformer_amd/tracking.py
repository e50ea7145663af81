"""Persistent person identities for the serving path: ``PoseTracker`` associates the poses ``ops.pose_nms`` keeps in a frame with
the tracks of the frames before, on the device (``ops.track_update``, csrc/track.hip: one launch per frame).

The association is a minimum-cost assignment between the live tracks and the frame's detections, cost = mean joint distance to
the track's last pose, where a pair further apart than ``max_dist`` costs ``max_dist`` -- what leaving both unmatched costs -- so
the matching is the global optimum, not a greedy nearest choice.  A matched track takes the detection's pose and score; an
unmatched track ages and is dropped after more than ``max_misses`` misses in a row; an unmatched detection opens a track in the
lowest free slot, with the stream's next id.  There is no motion model and no re-identification of a dropped track.

    tracker = PoseTracker(batch=1, rows=1024, num_joints=15, max_tracks=32)
    for frame in stream:
        _, count, dets = ops.pose_nms(pred, out=nms)
        ids, slots = tracker.update(dets, count)          # static (B, R) int32 tensors, nothing read back
    tracker.tracks()                                      # one read-back: the live tracks of every stream

``update`` has fixed shapes and launches only, so it can be captured in a HIP graph (``serving.GraphedDecoder(tracking=...)``).
"""
from __future__ import annotations

import collections
import contextlib

import torch

__all__ = ["PoseTracker", "Track"]

Track = collections.namedtuple("Track", "id slot hits misses born score pose")


class PoseTracker:
    """batch: independent streams (batch elements); rows: R of the ``dets`` (B, R, J, 5) it will be given; max_tracks <= 64 slots
    per stream; max_dist in the unit of the poses (mm; 500 is the recall distance of the evaluation); a track's id is reported
    once it has ``min_hits`` hits (``slots`` reports it from its first frame)."""

    def __init__(self, batch=1, rows=1024, num_joints=15, max_tracks=32, max_dist=500.0, max_misses=10, min_hits=1, device="cuda"):
        from . import ops
        self.batch, self.rows, self.num_joints, self.max_tracks = int(batch), int(rows), int(num_joints), int(max_tracks)
        self.max_dist, self.max_misses, self.min_hits = float(max_dist), int(max_misses), int(min_hits)
        if not (0.0 <= self.max_dist <= ops.LAP_BIG) or self.max_misses < 0 or self.min_hits < 0:
            raise ValueError("PoseTracker: 0 <= max_dist <= %g, max_misses >= 0 and min_hits >= 0 expected (got %r, %r, %r)"
                             % (ops.LAP_BIG, max_dist, max_misses, min_hits))
        self.device = torch.device(device)
        self.buffers = ops.track_buffers(self.batch, self.max_tracks, self.num_joints, self.rows, self.device)

    def update(self, dets, count=None):
        """dets (B, R, J, 5) fp32 and count (B, 2) int32 or None as ``ops.pose_nms`` leaves them -> (ids, slots), (B, R) int32,
        static tensors that the next update overwrites.  Launches only."""
        from . import ops
        with torch.cuda.device(dets.device) if dets.is_cuda else contextlib.nullcontext():
            return ops.track_update(dets, count, self.buffers, self.max_dist, self.max_misses, self.min_hits)

    def reset(self):
        """forget every track and counter (device fills)"""
        for k, t in self.buffers.items():
            t.fill_(-1 if k in ("id", "ids", "slots") else 0)
        return self

    def snapshot(self):
        """clones of the state buffers (``restore`` puts them back: a graph capture's warm-up forwards must not age tracks)"""
        return {k: t.clone() for k, t in self.buffers.items()}

    def restore(self, saved):
        for k, t in self.buffers.items():
            t.copy_(saved[k])
        return self

    def state(self):
        """the named counters of the state block as ints (a read-back)"""
        from . import ops
        return dict(zip(ops.TRACK_STATE, self.buffers["state"].cpu().tolist()))

    def tracks(self):
        """one read-back -> per batch element the live tracks in slot order, each a Track(id, slot, hits, misses, born, score, pose
        (J, 3) numpy fp32)"""
        keys = ("id", "hits", "misses", "born", "score", "pose")
        host = {k: self.buffers[k].cpu().numpy() for k in keys}
        return [[Track(int(host["id"][b, t]), t, int(host["hits"][b, t]), int(host["misses"][b, t]), int(host["born"][b, t]),
                       float(host["score"][b, t]), host["pose"][b, t].copy())
                 for t in range(self.max_tracks) if host["id"][b, t] >= 0] for b in range(self.batch)]
