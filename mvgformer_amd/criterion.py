"""Training criterion on the device: the ground-truth matcher and the per-layer losses of the reference
(lib/models/matcher.py HungarianMatcher with method KNN / multiple, lib/models/multi_view_pose_transformer.py SetCriterion, the
per-layer sum of lib/models/dq_transformer.py:653-731) on the fused HIP kernels of csrc/criterion.hip.

  KNNMatcher            constructor and forward(outputs, meta) of the reference's matcher; match() is the sync-free form
  HungarianMatcher      the reference's matcher class in full: methods hungarian / hungarian-dis on mvg_hungarian_match (one
                        launch, no .cpu(), no scipy), KNN / multiple delegated to mvg_knn_match
  SetCriterion          forward(outputs, meta, outputs_origin=None) -> (loss_dict, indices), the reference's keys
  criterion_all_layers  all decoder layers of a step in one mvg_criterion call: summed dict + dict_losses_layers + loss_init
  total_loss            lib/core/function.py:127-128

Shelf / Campus joint format (DECODER.convert_joint_format_indices of configs/shelf_campus/*.yaml): the decoder's queries keep
their 15 Panoptic joints, the ground truth has 14.  KNNMatcher.match, SetCriterion.table and criterion_all_layers take the
indices as `joint_map` and hand them to the kernels (mvg_knn_match_jm / mvg_criterion_jm), which read prediction joint
joint_map[j] for converted joint j and write the gradients back in the 15-joint shape: no gathered copy of the predictions, no
index / index_put launch, the same launch counts as without a map.  SetCriterion.forward is the reference's signature: its
callers pass already converted tensors, it takes no map.

Hungarian assignment (DECODER.match_method 'hungarian', the reference's default, and 'hungarian-dis') is built in
HungarianMatcher / ops.hungarian_match / factory.build_matcher_from_cfg.  It is reached through those names only: KNNMatcher,
ops.knn_match and build_criterion_from_cfg without a matcher keep refusing the Hungarian methods with NotImplementedError.
SetCriterion.forward hands the layer's own logits to a matcher that sets `uses_logits`; criterion_all_layers(init_poses=None)
with a HungarianMatcher matches every layer on its own outputs (gt_match: False) in one matcher launch.

Not built (no shipped YAML uses them): use_ce_match, aux_loss / enc_outputs, per-bone and 3D-projection losses, views flagged
'padding', match_coord_* other than 'abs' / 'norm'.  They raise; nothing falls back to torch or scipy."""
from __future__ import annotations

import torch
from torch import nn

from . import ops
from .functions import CriterionFunction

LOSS_KEYS = ("loss_ce", "class_error", "class_recall", "class_precision", "cardinality_error", "loss_pose_perjoint",
             "loss_pose_perprojection_2d")
METRIC_KEYS = ("class_error", "class_recall", "class_precision", "cardinality_error")


def layer_weights(decay_method, num_layers, device=None):
    """weights of the per-layer losses in the step's sum (dq_transformer.py:692-705), created on `device` (no host copy)"""
    if decay_method == "none":
        return torch.ones((num_layers,), device=device)
    if decay_method == "linear":
        return torch.linspace(0, 1, num_layers + 1, device=device)[1:]
    if decay_method == "exp":
        w = 2 ** torch.arange(1, num_layers + 1, device=device)
        return w / w[-1]
    if decay_method == "last":
        w = torch.zeros((num_layers,), device=device)
        w[-1:].fill_(1)
        return w
    raise ValueError("decay_method %r (none | linear | exp | last)" % (decay_method,))


def total_loss(loss_dict, weight_dict):
    """sum of the weighted losses the optimiser steps on (lib/core/function.py:127-128)"""
    return sum(loss_dict[k] * weight_dict[k] for k in loss_dict.keys() if k in weight_dict).sum()


def _check_meta(meta):
    if any("padding" in m for m in meta):
        raise NotImplementedError("views flagged 'padding' are not supported by the fused criterion")


class KNNMatcher(nn.Module):
    """The reference's matcher for match_method KNN / multiple on the device (mvg_knn_match: one launch, no .cpu())."""

    def __init__(self, match_coord_est, match_coord_gt, cost_class: float = 1, cost_pose: float = 1, cost_giou: float = 1,
                 method="KNN", method_value=None):
        super().__init__()
        if method in ("hungarian", "hungarian-dis"):
            raise NotImplementedError("match method %r: KNNMatcher does not solve the Hungarian assignment "
                                      "(criterion.HungarianMatcher does)" % method)
        if method not in ops.MATCH_METHODS:
            raise ValueError("unknown match method %r" % (method,))
        if match_coord_est != "abs" or match_coord_gt != "norm":
            raise NotImplementedError("match_coord_est %r / match_coord_gt %r (every shipped YAML: 'abs' / 'norm')"
                                      % (match_coord_est, match_coord_gt))
        # KNN and multiple use the pose distance alone (matcher.py:182-195); the cost weights are kept for the interface
        self.cost_class, self.cost_pose, self.cost_giou = cost_class, cost_pose, cost_giou
        self.match_coord_est, self.match_coord_gt = match_coord_est, match_coord_gt
        self.method, self.method_value = method, method_value
        self.grid_size = self.grid_center = None              # set by SetCriterion, as in the reference

    def match(self, poses, meta, method=None, value=None, joint_map=None, num_joints=None):
        """poses (B, NQ*J, 3) abs mm -> (pair_query, pair_gt, pair_count, matched) device tensors; no host synchronisation.
        joint_map: the ground truth's joint j is joint joint_map[j] of the poses, which have num_joints joints per query"""
        if self.grid_size is None:
            raise RuntimeError("KNNMatcher.grid_size / grid_center are not set (SetCriterion sets them)")
        return ops.knn_match(poses.float(), meta[0]["joints_3d"].float(), meta[0]["num_person"],
                             [float(v) for v in self.grid_size], [float(v) for v in self.grid_center],
                             method or self.method, self.method_value if value is None else value, joint_map=joint_map,
                             num_joints=num_joints)

    @torch.no_grad()
    def forward(self, outputs, meta, method=None, value=None):
        """the reference's return value: list[B] of (query_idx, gt_idx) int64 tensors, on the device.  Cutting the pair list to
        each element's length needs pair_count on the host: this form synchronises once, match() does not."""
        pq, pg, pc, _ = self.match(outputs["pred_poses"]["outputs_coord"], meta, method, value)
        return [(pq[b, :n].long(), pg[b, :n].long()) for b, n in enumerate(pc.tolist())]


class HungarianMatcher(nn.Module):
    """The reference's matcher (lib/models/matcher.py HungarianMatcher: class name, constructor signature and defaults) on the
    device.  Methods 'hungarian' (C = cost_pose * pose + cost_class * class) and 'hungarian-dis' (C = pose) run
    mvg_hungarian_match: one launch for all batch elements -- and all layers, if the poses carry a leading layer axis --, no
    .cpu(), no scipy, capturable in a HIP graph.  Methods 'KNN' and 'multiple' delegate to ops.knn_match.  KNNMatcher and
    ops.knn_match keep refusing the Hungarian methods: this class is the way to them."""

    uses_logits = True                                        # SetCriterion.forward passes the layer's logits to match()

    def __init__(self, match_coord_est="abs", match_coord_gt="norm", cost_class: float = 1, cost_pose: float = 1,
                 cost_giou: float = 1, method="hungarian", method_value=None):
        super().__init__()
        if method not in ops.HUNGARIAN_METHODS and method not in ops.MATCH_METHODS:
            raise ValueError("unknown match method %r" % (method,))
        if match_coord_est != "abs" or match_coord_gt != "norm":
            raise NotImplementedError("match_coord_est %r / match_coord_gt %r (every shipped YAML: 'abs' / 'norm')"
                                      % (match_coord_est, match_coord_gt))
        assert cost_class != 0 or cost_pose != 0 or cost_giou != 0, "all costs cant be 0"      # matcher.py:52
        self.cost_class, self.cost_pose, self.cost_giou = cost_class, cost_pose, cost_giou
        self.match_coord_est, self.match_coord_gt = match_coord_est, match_coord_gt
        self.method, self.method_value = method, method_value
        self.grid_size = self.grid_center = None              # set by SetCriterion, as in the reference

    def match(self, poses, meta, method=None, value=None, joint_map=None, num_joints=None, logits=None):
        """poses (B, NQ*J, 3) or (Lm, B, NQ*J, 3) abs mm, logits shaped to match or None (= logit 1 for every query) ->
        (pair_query, pair_gt, pair_count, matched) device tensors, a leading Lm kept; no host synchronisation.  The first
        arguments and the results are KNNMatcher.match's."""
        if self.grid_size is None:
            raise RuntimeError("HungarianMatcher.grid_size / grid_center are not set (SetCriterion sets them)")
        method = method or self.method
        size, center = [float(v) for v in self.grid_size], [float(v) for v in self.grid_center]
        gt, num_person = meta[0]["joints_3d"].float(), meta[0]["num_person"]
        if method in ops.HUNGARIAN_METHODS:
            return ops.hungarian_match(poses.float(), gt, num_person, size, center,
                                       logits=None if logits is None else logits.float(), method=method,
                                       cost_class=self.cost_class, cost_pose=self.cost_pose, joint_map=joint_map,
                                       num_joints=num_joints)
        if poses.dim() != 3:
            raise ValueError("match method %r takes poses (B, NQ*J, 3)" % (method,))
        return ops.knn_match(poses.float(), gt, num_person, size, center, method, self.method_value if value is None else value,
                             joint_map=joint_map, num_joints=num_joints)

    @torch.no_grad()
    def forward(self, outputs, meta, method=None, value=None):
        """the reference's return value: list[B] of (query_idx, gt_idx) int64 tensors, on the device, for the Hungarian methods
        in scipy's order (ascending query).  Cutting the pair list to each element's length needs pair_count on the host: this
        form synchronises once, match() does not."""
        pq, pg, pc, _ = self.match(outputs["pred_poses"]["outputs_coord"], meta, method, value, logits=outputs.get("pred_logits"))
        return [(pq[b, :n].long(), pg[b, :n].long()) for b, n in enumerate(pc.tolist())]


class SetCriterion(nn.Module):
    """losses 'labels', 'cardinality', 'joints' of the reference's SetCriterion with the 2D projection loss on, loss_joint_type l1
    and absolute coordinates (every shipped YAML)."""

    def __init__(self, num_classes, matcher, weight_dict, losses, cfg, focal_alpha=0.25, root_idx=2):
        super().__init__()
        if num_classes != 2:
            raise NotImplementedError("num_classes = %r (the head has two logits)" % (num_classes,))
        if sorted(losses) != ["cardinality", "joints", "labels"]:
            raise NotImplementedError("losses %r (built: joints + labels + cardinality)" % (losses,))
        d = cfg.DECODER
        unsupported = {"use_loss_pose_perbone": False, "use_loss_pose_perprojection": False, "loss_pose_normalize": False,
                       "use_ce_match": False, "aux_loss": False}
        for k, v in unsupported.items():
            if getattr(d, k, v) != v:
                raise NotImplementedError("DECODER.%s = %r is not built" % (k, getattr(d, k)))
        if getattr(d, "loss_joint_type", "l1") != "l1" or not getattr(d, "use_loss_pose_perprojection_2d", True):
            raise NotImplementedError("built: loss_joint_type l1 with use_loss_pose_perprojection_2d")
        self.num_classes, self.matcher, self.weight_dict, self.losses = num_classes, matcher, weight_dict, losses
        self.focal_alpha, self.root_idx = focal_alpha, root_idx
        self.img_size = list(cfg.NETWORK.IMAGE_SIZE)
        self.grid_size = torch.tensor(cfg.MULTI_PERSON.SPACE_SIZE)
        self.grid_center = torch.tensor(cfg.MULTI_PERSON.SPACE_CENTER)
        self.matcher.grid_size, self.matcher.grid_center = self.grid_size, self.grid_center
        self.pred_conf_threshold = d.pred_conf_threshold

    def num_samples(self, meta):
        """None on a single process (the kernel computes clamp(sum(num_person), 1) itself); under an initialised process group the
        all-reduced device scalar of multi_view_pose_transformer.py:847-855"""
        if not (torch.distributed.is_available() and torch.distributed.is_initialized()):
            return None
        n = meta[0]["num_person"].sum().float().reshape(1)
        torch.distributed.all_reduce(n)
        return torch.clamp(n / torch.distributed.get_world_size(), min=1)

    def table(self, logits, poses, poses_2d, pairs, meta, cams=None, joint_map=None):
        """(L, 8) loss table (ops.CRITERION_COLUMNS) of L layers against one pair list; differentiable in its first three
        arguments.  cams: the packed camera records (DecoderContext.cams); packed here from meta if not given.  joint_map: the
        ground truth's joint j is joint joint_map[j] of poses / poses_2d (unconverted decoder outputs)."""
        _check_meta(meta)
        if cams is None:
            cams = ops.pack_cameras(meta, self.img_size, logits.device)
        m0 = meta[0]
        vis2d = torch.stack([m["joints_vis"] for m in meta]).float()
        pq, pg, pc = pairs[:3]
        return CriterionFunction.apply(logits.float(), poses.float(), poses_2d.float(), pq, pg, pc, m0["joints_3d"].float(),
                                       m0["joints_3d_vis"].float(), vis2d, m0["num_person"], cams,
                                       [float(v) for v in self.grid_size], [float(v) for v in self.grid_center],
                                       float(self.pred_conf_threshold), self.num_samples(meta), float(self.focal_alpha), 2.0,
                                       None if joint_map is None else [int(v) for v in joint_map])

    @staticmethod
    def row_to_dict(row):
        return {k: row[i] for i, k in enumerate(LOSS_KEYS)}

    def forward(self, outputs, meta, outputs_origin=None):
        if "aux_outputs" in outputs or "enc_outputs" in outputs:
            raise NotImplementedError("aux_outputs / enc_outputs are not built (unused by the reference)")
        src = outputs_origin if outputs_origin else outputs
        if getattr(self.matcher, "uses_logits", False):
            pairs = self.matcher.match(src["pred_poses"]["outputs_coord"].detach(), meta, logits=src["pred_logits"].detach())
        else:
            pairs = self.matcher.match(src["pred_poses"]["outputs_coord"].detach(), meta)
        table = self.table(outputs["pred_logits"][None], outputs["pred_poses"]["outputs_coord"][None],
                           outputs["pred_poses_2d"]["outputs_coord_2d"][None], pairs, meta)
        pq, pg, pc = pairs[:3]
        indices = [(pq[b, :n].long(), pg[b, :n].long()) for b, n in enumerate(pc.tolist())]
        return self.row_to_dict(table[0]), indices


def criterion_all_layers(criterion, logits, poses, poses_2d, meta, init_poses, decay_method="none", cams=None, pairs=None,
                         joint_map=None):
    """The training step's loss dict for gt_match (dq_transformer.py:653-731, loss_for_each_layers): logits (L,B,NQ,2), poses
    (L,B,NQ*J,3), poses_2d (L,B,V,NQ*J,2) of all layers against the match of the initial poses init_poses (B,NQ*J,3) (or the
    pair list `pairs` if the caller matched already).  One matcher launch and three criterion launches, nothing read back.
    joint_map: the unconverted outputs against a ground truth in another joint format (Shelf / Campus), see the module docstring.
    init_poses=None (and no pairs) with a HungarianMatcher in a Hungarian method is the reference's gt_match: False
    (dq_transformer.py:666-678): every layer is matched on its own detached outputs, all L * B problems in ONE matcher launch, and
    criterion.table runs once per layer with that layer's pairs; `pairs` then comes back with a leading layer axis.  Any other
    matcher without init_poses raises ValueError."""
    if pairs is None and init_poses is None:
        m = criterion.matcher
        if not (isinstance(m, HungarianMatcher) and m.method in ops.HUNGARIAN_METHODS):
            raise ValueError("criterion_all_layers: init_poses=None (per-layer matching) needs a HungarianMatcher in a Hungarian "
                             "method, got %s" % type(m).__name__)
        pairs = m.match(poses.detach(), meta, joint_map=joint_map,
                        num_joints=None if joint_map is None else poses.shape[2] // logits.shape[2], logits=logits.detach())
        table = torch.cat([criterion.table(logits[l:l + 1], poses[l:l + 1], poses_2d[l:l + 1], tuple(t[l] for t in pairs), meta,
                                           cams, joint_map) for l in range(logits.shape[0])])
        return _layers_dict(table, decay_method), pairs
    if pairs is None:
        pairs = criterion.matcher.match(init_poses.detach(), meta, joint_map=joint_map,
                                        num_joints=None if joint_map is None else poses.shape[2] // logits.shape[2])
    table = criterion.table(logits, poses, poses_2d, pairs, meta, cams, joint_map)
    return _layers_dict(table, decay_method), pairs


def _layers_dict(table, decay_method):
    """the step's loss dict from the (L, 8) table: weighted sums, mean metrics, the per-layer dicts, loss_init"""
    Ln = table.shape[0]
    w = layer_weights(decay_method, Ln, table.device)
    loss_dict = {}
    for i, k in enumerate(LOSS_KEYS):
        loss_dict[k] = table[:, i].mean() if k in METRIC_KEYS else (w * table[:, i]).sum()
    loss_dict["dict_losses_layers"] = [SetCriterion.row_to_dict(table[l]) for l in range(Ln)]
    loss_dict["loss_init"] = torch.zeros((1,), dtype=torch.float32, device=table.device)
    return loss_dict
