"""Structural triangulation for the serving path: re-solve a person's joints from their 2D observations in all views under the
constraint that every bone has a given length (the reference's lib/structural/, ``triangulation_method`` 'st'), on the device
(``ops.structural_triangulate``, csrc/structural.hip: one launch, one wavefront per person, fp64).

A skeleton is a tree over the joints: ``parent[i]`` is the joint that joint i hangs from, joint 0 is the root (``parent[0] = -1``),
in any index order; bone k (k = 1 .. J-1) ends at joint k and its length is entry k-1 of a bone-length vector.

    refiner = StructuralRefiner(batch=1, rows=1024, bone_lengths=lengths_mm)
    keep, count, dets = ops.pose_nms(pred, out=nms)
    poses, status = refiner.update(refs2d, cams, Pm, keep, count)      # static (B, rows, J, 3) / (B, rows), nothing read back

``update`` has fixed shapes and launches only, so it can be captured in a HIP graph (``serving.GraphedDecoder(refine=...)``).  With
the view weights left uniform and lengths supplied by the user this is a CAPABILITY -- holding a skeleton fixed -- and no accuracy
result: no checkpoint or dataset stands behind it.
"""
from __future__ import annotations

import contextlib

import torch

__all__ = ["PANOPTIC15_PARENT", "H36M17_PARENT", "bone_lengths", "StructuralRefiner"]      # what `import *` brings, pinned by a test;
# BoneLengthEstimator (below) is imported by name

# the 15-joint CMU Panoptic skeleton of the decoder (root: joint 0) and the 17-joint Human3.6M one
PANOPTIC15_PARENT = (-1, 0, 0, 0, 3, 4, 2, 6, 7, 0, 9, 10, 2, 12, 13)
H36M17_PARENT = (-1, 2, 0, 0, 3, 4, 1, 0, 7, 16, 11, 12, 8, 8, 13, 14, 8)


def bone_lengths(poses, parent):
    """poses (..., J, 3) -> (..., J-1): the length of the bone that ends at joint k at index k-1; any device, the dtype of poses"""
    J = len(parent)
    if poses.shape[-2:] != (J, 3):
        raise ValueError("bone_lengths: poses (..., %d, 3) expected for this tree, got %s" % (J, tuple(poses.shape)))
    up = torch.as_tensor(list(parent[1:]), dtype=torch.long, device=poses.device)
    return (poses[..., 1:, :] - poses.index_select(-2, up)).norm(dim=-1)


class StructuralRefiner:
    """batch, rows: B and R of the (B, R, J, 3) poses it writes; row r of element b is the query ``keep[b, r]`` the NMS kept.
    bone_lengths: J-1 values in the unit of the projection matrices' translations (mm), shared by every person; they live in the
    static tensor ``self.bone_lengths`` and may be overwritten between updates.  Or a static (B, rows, J-1) fp32 device tensor of
    per-person lengths, row r for row r of the poses (``BoneLengthEstimator.row_length``): kept by reference and handed to the
    solver in its per-person form.  n_steps (1 .. 8) and method ("ST", or "LS" for the unconstrained least squares in the same
    bone coordinates) are fixed at construction."""

    def __init__(self, batch=1, rows=1024, parent=PANOPTIC15_PARENT, bone_lengths=None, n_steps=1, method="ST", device="cuda"):
        from . import ops
        self.parent = tuple(int(p) for p in parent)
        self.batch, self.rows, self.num_joints = int(batch), int(rows), len(self.parent)
        self.n_steps, self.method = int(n_steps), str(method)
        ops.structural_check(self.parent, self.n_steps, self.method)
        if bone_lengths is None:
            raise ValueError("StructuralRefiner: bone_lengths (%d values) are required" % (self.num_joints - 1))
        self.device = torch.device(device)
        if torch.is_tensor(bone_lengths) and bone_lengths.dim() == 3:
            # per-person lengths, a static tensor somebody else writes (BoneLengthEstimator.row_length): taken by reference
            want = (self.batch, self.rows, self.num_joints - 1)
            if tuple(bone_lengths.shape) != want or bone_lengths.dtype != torch.float32 or not bone_lengths.is_contiguous() \
                    or bone_lengths.device.type != self.device.type:
                raise ValueError("StructuralRefiner: per-person bone lengths must be a contiguous float32 tensor of shape %s on %s, "
                                 "got %s %s on %s" % (want, self.device, bone_lengths.dtype, tuple(bone_lengths.shape),
                                                      bone_lengths.device))
            self.bone_lengths = bone_lengths
        else:
            lengths = torch.as_tensor(bone_lengths, dtype=torch.float32).reshape(-1)
            if lengths.numel() != self.num_joints - 1:
                raise ValueError("StructuralRefiner: %d bone lengths for a tree of %d joints (%d expected)"
                                 % (lengths.numel(), self.num_joints, self.num_joints - 1))
            self.bone_lengths = lengths.to(self.device).contiguous()
        self.buffers = ops.structural_buffers(self.batch, self.rows, self.num_joints, self.device)

    @property
    def poses(self):
        return self.buffers["poses"]

    @property
    def status(self):
        return self.buffers["status"]

    def tensors(self):
        """every device tensor ``update`` addresses besides its arguments (what a captured graph must keep alive)"""
        return list(self.buffers.values()) + [self.bone_lengths]

    def update(self, refs2d, cams, Pm, keep, count, conf=None):
        """conf (B, V, NQ*J) fp32 or None: the views' weights in the solver's sums (ops.structural_triangulate); a view with weight 0
        adds exact zeros.
        refs2d (B, V, NQ*J, 2) fp32 network-image px (the last layer's), cams the packed camera records, Pm (B, V, 3, 4) fp32, keep
        (B, NQ) int32 and count (B, 2) int32 as ``ops.pose_nms`` leaves them -> (poses, status), static tensors that the next update
        overwrites: row r < count[b, 0] holds query keep[b, r], the others zeros and status -1.  Two launches."""
        from . import _lib as L, ops
        L.require_cuda(refs2d, cams, Pm, keep, count)
        with torch.cuda.device(refs2d.device) if refs2d.is_cuda else contextlib.nullcontext():
            B, V = refs2d.shape[:2]
            ud, _ = ops.uncrop_undistort_jac(refs2d, cams, V, B)
            return ops.structural_triangulate(ud, conf, Pm, self.parent, self.bone_lengths, rows=keep[:, :self.rows], count=count,
                                              n_steps=self.n_steps, method=self.method, out=self.buffers)


class BoneLengthEstimator:
    """The bone lengths of every tracked person, estimated on the device from the frames the tracker has followed them
    (``ops.track_bones``, csrc/bones.hip: one launch per frame behind ``tracking.PoseTracker.update``, nothing read back, no
    atomics): every track slot keeps the lengths of its track's last ``window`` detections and their median; a slot that changes
    hands starts over.  ``row_length`` (B, rows, J-1) fp32 -- per row of the detections the median of its track once the track has
    ``min_frames`` samples, else ``fallback`` (J-1 values) or, without one, the row's own lengths -- is what a ``StructuralRefiner``
    takes as per-person ``bone_lengths``; ``row_source`` (B, rows) int32 says which of the three it was (0, 1, 2; -1: no detection).

        estimator = BoneLengthEstimator(batch=1, rows=1024, max_tracks=32)
        refiner = StructuralRefiner(batch=1, rows=1024, bone_lengths=estimator.row_length)
        ids, slots = tracker.update(dets, count)
        estimator.update(dets, count, tracker)                             # launch only
        poses, status = refiner.update(refs2d, cams, Pm, keep, count)

    The samples are taken from the raw detections, never from the tracker's filtered poses or the refiner's output: the estimate
    does not feed on itself.  batch, rows and max_tracks are those of the tracker it follows."""

    def __init__(self, batch=1, rows=1024, max_tracks=32, parent=PANOPTIC15_PARENT, window=8, min_frames=4, fallback=None,
                 device="cuda"):
        from . import ops
        self.parent = tuple(int(p) for p in parent)
        ops.structural_check(self.parent)
        self.batch, self.rows, self.max_tracks, self.num_joints = int(batch), int(rows), int(max_tracks), len(self.parent)
        self.window, self.min_frames = int(window), int(min_frames)
        if not 1 <= self.window <= ops.BONES_MAX_W or self.min_frames < 1:
            raise ValueError("BoneLengthEstimator: 1 <= window <= %d and min_frames >= 1 expected (got %r, %r)"
                             % (ops.BONES_MAX_W, window, min_frames))
        self.device = torch.device(device)
        self.fallback = None
        if fallback is not None:
            values = torch.as_tensor(fallback, dtype=torch.float32).reshape(-1)
            if values.numel() != self.num_joints - 1:
                raise ValueError("BoneLengthEstimator: %d fallback lengths for a tree of %d joints (%d expected)"
                                 % (values.numel(), self.num_joints, self.num_joints - 1))
            self.fallback = values.to(self.device).contiguous()
        self.buffers = ops.track_bones_buffers(self.batch, self.max_tracks, self.num_joints, self.rows, self.window, self.device)

    @property
    def row_length(self):
        return self.buffers["row_length"]

    @property
    def row_source(self):
        return self.buffers["row_source"]

    def update(self, dets, count, tracker):
        """dets (B, R, J, 5) fp32 and count (B, 2) int32 or None as ``tracker.update(dets, count)`` has just associated them ->
        (row_length, row_source), static tensors that the next update overwrites.  One launch."""
        from . import ops
        with torch.cuda.device(dets.device) if dets.is_cuda else contextlib.nullcontext():
            return ops.track_bones(dets, count, tracker.buffers, self.parent, self.buffers, self.min_frames, self.fallback)

    def tensors(self):
        """every device tensor ``update`` addresses besides its arguments (what a captured graph must keep alive)"""
        return list(self.buffers.values()) + ([] if self.fallback is None else [self.fallback])

    def reset(self):
        """forget every history (device fills)"""
        for k, t in self.buffers.items():
            t.fill_(-1 if k in ("owner", "row_source") else 0)
        return self

    def snapshot(self):
        """clones of the buffers (``restore`` puts them back: a graph capture's warm-up forwards must leave no history)"""
        return {k: t.clone() for k, t in self.buffers.items()}

    def restore(self, saved):
        for k, t in self.buffers.items():
            t.copy_(saved[k])
        return self

    def lengths(self):
        """one read-back -> per stream {track id: (lengths (J-1) numpy fp32, seen)} of the slots that hold a live track's history"""
        K = self.num_joints - 1
        packed = torch.cat([self.buffers["owner"].reshape(-1).double(), self.buffers["seen"].reshape(-1).double(),
                            self.buffers["length"].reshape(-1).double()]).cpu().numpy()
        B, T = self.batch, self.max_tracks
        owner, seen = packed[:B * T].reshape(B, T), packed[B * T:2 * B * T].reshape(B, T)
        length = packed[2 * B * T:].reshape(B, T, K)
        return [{int(owner[b, t]): (length[b, t].astype("float32"), int(seen[b, t])) for t in range(T) if owner[b, t] >= 0}
                for b in range(B)]
