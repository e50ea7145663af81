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

__all__ = ["PANOPTIC15_PARENT", "H36M17_PARENT", "bone_lengths", "StructuralRefiner"]

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
    static tensor ``self.bone_lengths`` and may be overwritten between updates.  n_steps (1 .. 8) and method ("ST", or "LS" for the
    unconstrained least squares in the same bone coordinates) are fixed at construction."""

    def __init__(self, batch=1, rows=1024, parent=PANOPTIC15_PARENT, bone_lengths=None, n_steps=1, method="ST", device="cuda"):
        from . import ops
        self.parent = tuple(int(p) for p in parent)
        self.batch, self.rows, self.num_joints = int(batch), int(rows), len(self.parent)
        self.n_steps, self.method = int(n_steps), str(method)
        ops.structural_check(self.parent, self.n_steps, self.method)
        if bone_lengths is None:
            raise ValueError("StructuralRefiner: bone_lengths (%d values) are required" % (self.num_joints - 1))
        self.device = torch.device(device)
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

    def update(self, refs2d, cams, Pm, keep, count):
        """refs2d (B, V, NQ*J, 2) fp32 network-image px (the last layer's), cams the packed camera records, Pm (B, V, 3, 4) fp32, keep
        (B, NQ) int32 and count (B, 2) int32 as ``ops.pose_nms`` leaves them -> (poses, status), static tensors that the next update
        overwrites: row r < count[b, 0] holds query keep[b, r], the others zeros and status -1.  Two launches."""
        from . import _lib as L, ops
        L.require_cuda(refs2d, cams, Pm, keep, count)
        with torch.cuda.device(refs2d.device) if refs2d.is_cuda else contextlib.nullcontext():
            B, V = refs2d.shape[:2]
            ud, _ = ops.uncrop_undistort_jac(refs2d, cams, V, B)
            return ops.structural_triangulate(ud, None, Pm, self.parent, self.bone_lengths, rows=keep[:, :self.rows], count=count,
                                              n_steps=self.n_steps, method=self.method, out=self.buffers)
