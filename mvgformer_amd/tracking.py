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

``TrackEvaluator`` scores the ids against ground truth on the device, one more launch behind the tracker's (``ops.track_eval``):
CLEAR-MOT counts (MOTA, MOTP) and the person x track-id overlap table IDF1 is computed from at the one read-back
(``serving.GraphedDecoder(tracking=..., track_evaluation=...)``).
"""
from __future__ import annotations

import collections
import contextlib
import math

import torch

__all__ = ["PoseTracker", "Track", "TrackEvaluator", "max_weight_assignment"]

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
    tuned on no recorded sequence, and no accuracy is claimed for them (``TrackEvaluator`` below is the instrument; the one table
    measured with it, profiles/track_eval.txt, is on synthetic sequences, not on Panoptic)."""

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

    def tensors(self):
        """every device tensor ``update`` addresses besides its arguments (what a captured graph must keep alive)"""
        return list(self._all_buffers().values())

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


def max_weight_assignment(table):
    """table (n, m) of non-negative integers -> (total, col_of_row): the one-to-one assignment of rows to columns of maximum total
    weight (col_of_row[r] = -1 for a row left out because n > m), by shortest augmenting paths with integer potentials, the inner
    loop over the columns vectorised.  The identity overlap tables it is for have at most 64 rows."""
    import numpy as np
    w = np.asarray(table, dtype=np.int64)
    if w.ndim != 2:
        raise ValueError("max_weight_assignment: a 2-D table expected")
    rows, cols = w.shape
    col_of_row = np.full((rows,), -1, np.int64)
    if rows == 0 or cols == 0:
        return 0, col_of_row
    flipped = rows > cols
    if flipped:
        w = w.T
    n, m = w.shape
    cost = -w                                            # minimise; every row gets a column (n <= m, weights >= 0: no loss)
    big = np.iinfo(np.int64).max // 4
    u, v = np.zeros(n + 1, np.int64), np.zeros(m + 1, np.int64)
    p, way = np.zeros(m + 1, np.int64), np.zeros(m + 1, np.int64)     # p[j]: the row of column j, 1-based, 0 = none
    for i in range(1, n + 1):
        p[0], j0 = i, 0
        minv, used = np.full(m + 1, big, np.int64), np.zeros(m + 1, bool)
        for _ in range(m + 1):                           # every step uses one more column
            used[j0] = True
            i0 = p[j0]
            cur = cost[i0 - 1] - u[i0] - v[1:]
            better = ~used[1:] & (cur < minv[1:])
            minv[1:][better] = cur[better]
            way[1:][better] = j0
            masked = np.where(used, big, minv)
            j1 = int(np.argmin(masked[1:])) + 1
            delta = masked[j1]
            u[p[used]] += delta                          # the rows of the used columns are distinct
            v[used] -= delta
            minv[~used] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    total = 0
    for j in range(1, m + 1):
        if p[j] > 0:
            r, c = (j - 1, p[j] - 1) if flipped else (p[j] - 1, j - 1)
            col_of_row[r] = c
            total += int(w[p[j] - 1, j - 1])
    return total, col_of_row


def _ratio(num, den):
    return float(num) / float(den) if den else math.nan


class TrackEvaluator:
    """CLEAR-MOT and identity scores of a ``PoseTracker``'s ids against ground truth, accumulated on the device
    (``ops.track_eval``, csrc/track.hip: one launch per frame behind the tracker, nothing read back, fp64, no atomics).

        scorer = TrackEvaluator(batch=1, max_persons=10)
        for frame in stream:
            ids, slots = tracker.update(dets, count)
            scorer.update(tracker, dets, count, joints_3d, joints_3d_vis, num_person)      # launch only
        scorer.report()["total"]["mota"]                                                    # one read-back

    batch: streams; max_persons: identities per stream (<= 64), at least the person slots of the ground truth; max_ids: columns
    of the person x track id overlap table IDF1 is computed from (<= 4096; ids at or above it are counted in ``id_overflow``);
    dist_thr: the distance within which a pose can be a person's, in the unit of the poses (500 mm: the evaluation's recall
    distance).  The rules are the contract of ``mvg_track_eval`` in include/mvg_decoder.h."""

    def __init__(self, batch=1, max_persons=10, max_ids=1024, dist_thr=500.0, device="cuda"):
        from . import ops
        self.batch, self.max_persons, self.max_ids, self.dist_thr = int(batch), int(max_persons), int(max_ids), float(dist_thr)
        if not (0.0 <= self.dist_thr <= ops.LAP_BIG):
            raise ValueError("TrackEvaluator: 0 <= dist_thr <= %g expected (got %r)" % (ops.LAP_BIG, dist_thr))
        self.device = torch.device(device)
        self.buffers = ops.track_eval_buffers(self.batch, self.max_persons, self.max_ids, self.device)
        self._next_id = None           # the last tracker's next_id: what report() names when ids overflowed the table

    def ground_truth_buffers(self, batch, num_joints):
        """zeroed static inputs (joints_3d, joints_3d_vis, num_person, person_id) for ``max_persons`` person slots (graph capture);
        person_id is the identity map, slot g = identity g"""
        from .evaluate import ground_truth_buffers
        ident = torch.arange(self.max_persons, dtype=torch.int32, device=self.device).repeat(batch, 1).contiguous()
        return (*ground_truth_buffers(batch, self.max_persons, num_joints, self.device), ident)

    def update(self, tracker, dets, count, joints_3d, joints_3d_vis, num_person, person_id=None):
        """score the frame ``tracker.update(dets, count)`` has just associated: the tracker's ids (and, with its motion model, its
        filtered ``row_poses`` instead of the detections' poses) against joints_3d (B, G, J, 3), joints_3d_vis (B, G, J) fp32 and
        num_person (B) int32 (< 0: the frame has no annotation and is skipped); person_id (B, G) int32 or None.  Launch only."""
        from . import ops
        if joints_3d.dim() == 4 and joints_3d.shape[1] > self.max_persons:
            raise ValueError("TrackEvaluator: %d person slots, built for max_persons = %d" % (joints_3d.shape[1], self.max_persons))
        self._next_id = tracker.buffers["next_id"]
        with torch.cuda.device(dets.device) if dets.is_cuda else contextlib.nullcontext():
            ops.track_eval(dets, count, tracker.buffers["ids"], joints_3d, joints_3d_vis, num_person, self.buffers, self.dist_thr,
                           row_pose=tracker.row_poses, person_id=person_id)
        return self

    def reset(self):
        """forget every count (device fills)"""
        for k, t in self.buffers.items():
            t.fill_(-1 if k == "last_track" else 0)
        return self

    def tensors(self):
        """every device tensor ``update`` addresses besides its arguments (what a captured graph must keep alive)"""
        return list(self.buffers.values())

    def snapshot(self):
        """clones of the state buffers (``restore`` puts them back: a graph capture's warm-up forwards must count no frame)"""
        return {k: t.clone() for k, t in self.buffers.items()}

    def restore(self, saved):
        for k, t in self.buffers.items():
            t.copy_(saved[k])
        return self

    def state(self):
        """the named counters summed over the streams, as ints (a read-back)"""
        from . import ops
        return dict(zip(ops.TRACK_EVAL_STATE, self.buffers["counters"].sum(dim=0).cpu().tolist()))

    def _read(self):
        """every buffer in ONE copy to the host -> dict of numpy arrays (plus next_id of the last tracker, if any)"""
        import numpy as np
        named = dict(self.buffers)
        if self._next_id is not None:
            named["next_id"] = self._next_id
        raw = torch.cat([t.reshape(-1).view(torch.uint8) for t in named.values()]).cpu().numpy()
        out, at = {}, 0
        for k, t in named.items():
            size = t.numel() * t.element_size()
            out[k] = np.frombuffer(raw[at:at + size].tobytes(), dtype=str(t.dtype).replace("torch.", "")).reshape(tuple(t.shape))
            at += size
        return out

    @staticmethod
    def _scores(c, dist_sum, idtp, seen, covered):
        """the ratios of one stream or of the sum over the streams; a ratio is NaN when its denominator is 0"""
        tracked = [(int(cv), int(sn)) for cv, sn in zip(covered.reshape(-1).tolist(), seen.reshape(-1).tolist()) if sn > 0]
        out = dict(c)
        out.update(dist_sum=float(dist_sum),
                   mota=1.0 - _ratio(c["misses"] + c["false_pos"] + c["switches"], c["gt"]),
                   motp=_ratio(dist_sum, c["matches"]), idtp=idtp,
                   idf1=None if c["id_overflow"] > 0 else _ratio(2 * idtp, c["gt"] + c["hyp"]),
                   identities=len(tracked),
                   mostly_tracked=sum(1 for cv, sn in tracked if 5 * cv >= 4 * sn),       # covered / seen >= 0.8
                   mostly_lost=sum(1 for cv, sn in tracked if 5 * cv <= sn))              # covered / seen <= 0.2
        return out

    def report(self):
        """one read-back -> {"streams": [per stream], "total": summed over the streams}, each the named counters, dist_sum, mota =
        1 - (misses + false_pos + switches) / gt, motp = dist_sum / matches, idtp = the maximum-weight one-to-one assignment of
        identities to track ids on the overlap table (``max_weight_assignment``, on the host), idf1 = 2 idtp / (gt + hyp),
        identities (those seen), mostly_tracked / mostly_lost (covered / seen >= 0.8 / <= 0.2).  A ratio is NaN when its
        denominator is 0.  With ids that did not fit the table (id_overflow > 0) idf1 is None and "max_ids_needed" says which
        ``max_ids`` the run needs."""
        import numpy as np
        from . import ops
        host = self._read()
        streams = []
        for b in range(self.batch):
            c = dict(zip(ops.TRACK_EVAL_STATE, (int(x) for x in host["counters"][b])))
            table = host["overlap"][b]
            used = np.flatnonzero(table.any(axis=0))                             # only the ids that were ever near a person
            idtp = max_weight_assignment(table[:, used])[0] if len(used) else 0
            streams.append(self._scores(c, host["dist_sum"][b], idtp, host["seen"][b], host["covered"][b]))
        total_c = {k: sum(s[k] for s in streams) for k in ops.TRACK_EVAL_STATE}
        dist_sum = 0.0
        for b in range(self.batch):
            dist_sum += float(host["dist_sum"][b])
        total = self._scores(total_c, dist_sum, sum(s["idtp"] for s in streams), host["seen"], host["covered"])
        out = dict(streams=streams, total=total, dist_thr=self.dist_thr, max_persons=self.max_persons, max_ids=self.max_ids)
        if total_c["id_overflow"] > 0:
            out["note"] = ("track ids at or above max_ids = %d were met %d times: the overlap table is incomplete and idf1 is not "
                           "reported; " % (self.max_ids, total_c["id_overflow"]))
            if "next_id" in host:
                out["max_ids_needed"] = int(host["next_id"].max())
                out["note"] += "rerun with max_ids >= %d" % out["max_ids_needed"]
            else:       # the buffers were not filled through update(tracker, ...): the ids the tracker gave out are not known here
                out["max_ids_needed"] = None
                out["note"] += "rerun with max_ids above the largest track id (the tracker's next_id)"
        return out
