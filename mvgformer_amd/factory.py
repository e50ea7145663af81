"""Build the decoder for a synthetic case or from the reference's YAML config files."""
from __future__ import annotations

from types import SimpleNamespace

import torch
import yaml

from .decoder import DQDecoder, DQDecoderLayer
from .synthetic import decoder_cfg, to_torch_state

# defaults of lib/core/config.py for the keys the decoder reads (config.py:303-304 etc.)
_DECODER_DEFAULTS = dict(pose_embed_layer=3, d_model=256, dim_feedforward=1024, dropout=0.1, activation="relu",
                         num_feature_levels=1, nhead=8, dec_n_points=8, num_decoder_layers=4,
                         return_intermediate_dec=True, num_instance=1024, num_keypoints=15,
                         detach_refpoints_cameraprj_firstlayer=True, fuse_view_feats="cat_proj",
                         projattn_posembed_mode="ablation_not_use_rayconv", feature_update_method="MLP",
                         init_self_attention=False, open_forward_ffn=True, query_filter_method="threshold",
                         bayesian_update=False, triangulation_method="linalg", filter_query=True,
                         share_layer_weights=False, inference_conf_thr=[0.1])
# defaults of lib/core/config.py:244-257, 306-318 for the keys the training criterion reads
_CRITERION_DEFAULTS = dict(match_coord_est="abs", match_coord_gt="norm", match_method="KNN", match_method_value=5,
                           loss_weight_loss_ce=2.0, loss_pose_perjoint=5.0, loss_pose_perprojection_2d=5.0, loss_weight_init=0.0,
                           pred_conf_threshold=0.5, decay_method="none", loss_joint_type="l1", loss_pose_normalize=False,
                           use_loss_pose_perbone=False, use_loss_pose_perprojection=False, use_loss_pose_perprojection_2d=True,
                           use_ce_match=False)
# defaults of lib/core/config.py:152,169 (TRAIN.LR, TRAIN.clip_max_norm) and :245 (DECODER.lr_linear_proj_mult)
_TRAIN_DEFAULTS = dict(LR=0.001, clip_max_norm=0.1)
_LR_LINEAR_PROJ_NAMES = ("reference_points", "sampling_offsets")


def load_yaml_config(path):
    """Read the hot-path hyper-parameters from one of the reference's YAML entry points
    (e.g. configs/panoptic/knn5-lr4-q1024-g8.yaml; keys per lib/models/dq_transformer.py:129-157)."""
    with open(path) as f:
        raw = yaml.safe_load(f)
    dec = dict(_DECODER_DEFAULTS)
    dec.update(raw.get("DECODER", {}))
    train = {k: (raw.get("TRAIN") or {}).get(k, v) for k, v in _TRAIN_DEFAULTS.items()}
    return SimpleNamespace(
        DECODER=SimpleNamespace(**dec),
        NETWORK=SimpleNamespace(IMAGE_SIZE=list(raw["NETWORK"]["IMAGE_SIZE"])),
        MULTI_PERSON=SimpleNamespace(SPACE_SIZE=list(raw["MULTI_PERSON"]["SPACE_SIZE"]),
                                     SPACE_CENTER=list(raw["MULTI_PERSON"]["SPACE_CENTER"])),
        DATASET=SimpleNamespace(CAMERA_NUM=int(raw["DATASET"]["CAMERA_NUM"])),
        DEBUG=SimpleNamespace(VISUALIZATION_JUMP_NUM=-1),
        TRAIN=SimpleNamespace(LR=float(train["LR"]), clip_max_norm=float(train["clip_max_norm"])),
    )


def build_decoder_from_cfg(cfg):
    """Same construction as lib/models/dq_transformer.py:129-157."""
    d = cfg.DECODER
    layer = DQDecoderLayer(cfg.MULTI_PERSON.SPACE_SIZE, cfg.MULTI_PERSON.SPACE_CENTER, cfg.NETWORK.IMAGE_SIZE,
                           d.pose_embed_layer, d.d_model, d.dim_feedforward, d.dropout, d.activation,
                           d.num_feature_levels, d.nhead, d.dec_n_points, d.detach_refpoints_cameraprj_firstlayer,
                           d.fuse_view_feats, cfg.DATASET.CAMERA_NUM, d.projattn_posembed_mode,
                           d.feature_update_method, d.init_self_attention, d.open_forward_ffn, d.query_filter_method,
                           visualization_jump_num=-1, bayesian_update=d.bayesian_update,
                           triangulation_method=d.triangulation_method, filter_query=d.filter_query,
                           num_joints=d.num_keypoints)
    return DQDecoder(cfg, layer, d.num_decoder_layers, d.return_intermediate_dec)


def build_weight_dict(cfg):
    """multi_view_pose_transformer.py:224-230"""
    d = cfg.DECODER
    return {"loss_ce": d.loss_weight_loss_ce, "loss_pose_perjoint": d.loss_pose_perjoint,
            "loss_pose_perprojection_2d": d.loss_pose_perprojection_2d, "loss_init": d.loss_weight_init}


def build_matcher_from_cfg(cfg):
    """criterion.HungarianMatcher -- the reference's matcher class in full, on the device -- from the DECODER keys with the cost
    weights of multi_view_pose_transformer.py:217-247 (cost_class 2, cost_pose 5).  Missing keys take the reference's defaults
    (lib/core/config.py:306-318): a bare cfg gives match_method 'hungarian'.  Hand the result to build_criterion_from_cfg /
    build_training_head as `matcher`; without one they build a KNNMatcher, which refuses the Hungarian methods."""
    from .criterion import HungarianMatcher
    d = getattr(cfg, "DECODER", None)
    return HungarianMatcher(getattr(d, "match_coord_est", "abs"), getattr(d, "match_coord_gt", "norm"), cost_class=2., cost_pose=5.,
                            method=getattr(d, "match_method", "hungarian"), method_value=getattr(d, "match_method_value", 5))


def build_criterion_from_cfg(cfg, matcher=None):
    """matcher + criterion + weight_dict from the DECODER keys, as multi_view_pose_transformer.py:217-247 builds them
    (cost_class 2, cost_pose 5, focal alpha 0.25, losses joints / labels / cardinality).  Keys a hand-made cfg lacks take the
    defaults of lib/core/config.py.  matcher: the matcher to use (build_matcher_from_cfg's HungarianMatcher for the Hungarian
    methods); None builds a KNNMatcher from the cfg, which raises NotImplementedError for match_method 'hungarian' /
    'hungarian-dis'.  Returns (criterion, weight_dict, decay_method)."""
    from .criterion import KNNMatcher, SetCriterion
    d = SimpleNamespace(**{**_CRITERION_DEFAULTS, **vars(cfg.DECODER)})
    full = SimpleNamespace(DECODER=d, NETWORK=cfg.NETWORK, MULTI_PERSON=cfg.MULTI_PERSON)
    if matcher is None:
        matcher = KNNMatcher(d.match_coord_est, d.match_coord_gt, cost_class=2., cost_pose=5., method=d.match_method,
                             method_value=d.match_method_value)
    weight_dict = build_weight_dict(full)
    criterion = SetCriterion(2, matcher, weight_dict, ["joints", "labels", "cardinality"], full, focal_alpha=0.25)
    return criterion, weight_dict, d.decay_method


def build_training_head(cfg, decoder=None, t_pose=None, matcher=None):
    """caller.DecoderHead around the cfg's decoder with the cfg's criterion set: forward_train is ready.  Returns (head, weight_dict).
    matcher: handed to build_criterion_from_cfg (build_matcher_from_cfg(cfg) for the Hungarian methods).
    DECODER.convert_joint_format_indices (the shelf_campus YAMLs) becomes the head's joint map: forward_train then takes ground
    truth with that many joints."""
    from .caller import DecoderHead
    d = cfg.DECODER
    decoder = build_decoder_from_cfg(cfg) if decoder is None else decoder
    conv = getattr(d, "convert_joint_format_indices", None)
    head = DecoderHead(decoder, d.num_instance, d.num_keypoints, d.d_model, cfg.MULTI_PERSON.SPACE_SIZE, cfg.MULTI_PERSON.SPACE_CENTER,
                       convert_joint_format_indices=None if conv is None else [int(i) for i in conv], t_pose=t_pose)
    criterion, weight_dict, decay = build_criterion_from_cfg(cfg, matcher=matcher)
    head.set_criterion(criterion, decay)
    return head, weight_dict


def build_optimizer_from_cfg(head, cfg, optim_type=None, weight_decay=1e-4, lr=None):
    """optim.FusedAdam with the reference's two parameter groups (run/train_3d.py:116-146): every trainable parameter at TRAIN.LR,
    except those whose name contains 'reference_points' or 'sampling_offsets' at TRAIN.LR * DECODER.lr_linear_proj_mult.
    optim_type (default DECODER.optimizer): 'adam' -- no weight decay -- or 'adamw' -- decoupled `weight_decay` (the reference's
    1e-4).  The gradient-norm clip is TRAIN.clip_max_norm (function.py:171-176), and the step leaves the gradients zeroed in
    place.  A cfg without TRAIN / the DECODER keys takes the defaults of lib/core/config.py."""
    from .optim import FusedAdam
    train = getattr(cfg, "TRAIN", None)
    lr = float(getattr(train, "LR", _TRAIN_DEFAULTS["LR"]) if lr is None else lr)
    clip = float(getattr(train, "clip_max_norm", _TRAIN_DEFAULTS["clip_max_norm"]))
    mult = float(getattr(cfg.DECODER, "lr_linear_proj_mult", 0.1))
    optim_type = getattr(cfg.DECODER, "optimizer", "adam") if optim_type is None else optim_type
    if optim_type not in ("adam", "adamw"):
        raise ValueError("optimizer %r (adam | adamw)" % (optim_type,))
    slow = lambda n: any(k in n for k in _LR_LINEAR_PROJ_NAMES)     # noqa: E731
    named = [(n, p) for n, p in head.named_parameters() if p.requires_grad]
    groups = [{"params": [p for n, p in named if not slow(n)], "lr": lr},
              {"params": [p for n, p in named if slow(n)], "lr": lr * mult}]
    adamw = optim_type == "adamw"
    return FusedAdam(groups, lr=lr, weight_decay=float(weight_decay) if adamw else 0.0, decoupled_weight_decay=adamw,
                     clip_max_norm=clip, zero_grad=True)


def build_graphed_train_step(head, optimizer, case_or_shapes, weight_dict=None, threshold=0.1, capture=True, warmup=3):
    """training.GraphedTrainStep for `head` under `optimizer` (a FusedAdam with zero_grad=True, build_optimizer_from_cfg's): the
    whole step -- forward_train, total_loss, backward, optimizer step -- as one HIP graph.  case_or_shapes: anything with
    src_views, meta, spatial_shapes, level_start_index on the device and the ground truth in its meta (a synthetic case after
    case_to_device + add_ground_truth, or a namespace holding one real batch): it gives the shapes and the first batch.
    weight_dict: the criterion's by default.  With the decoder in bf16 training (set_training_dtype) a training.TrainOperands is
    built and attached to the optimizer unless one is attached already.  capture=True runs GraphedTrainStep.capture(warmup): its
    `warmup` warm-up steps are real optimizer steps on this first batch -- parameters, moments and step count move."""
    from .training import GraphedTrainStep, TrainOperands
    c = case_or_shapes
    weight_dict = head.criterion.weight_dict if weight_dict is None else weight_dict
    operands = optimizer.operands
    if operands is None and any(l.training_dtype == torch.bfloat16 for l in head.decoder.layers):
        operands = TrainOperands(head)
        optimizer.attach_operands(operands)
    step = GraphedTrainStep(head, optimizer, weight_dict, c.src_views, c.meta, getattr(c, "spatial_shapes", None),
                            getattr(c, "level_start_index", None), threshold=threshold, operands=operands)
    return step.capture(warmup) if capture else step


def build_decoder_for_case(case, device="cuda", dtype=torch.float32):
    """Decoder with the panoptic hyper-parameters and the case's seeded weights."""
    layer = DQDecoderLayer(list(case.space_size), list(case.space_center), list(case.img_size), 3,
                           256, 1024, 0.1, "relu", 1, 8, 8, True, "cat_proj", case.V,
                           "ablation_not_use_rayconv", "MLP", False, True, "threshold",
                           visualization_jump_num=-1, bayesian_update=False, triangulation_method="linalg",
                           filter_query=True, num_joints=15)
    dec = DQDecoder(decoder_cfg(case.space_size, case.space_center), layer, case.layers, True)
    missing, unexpected = dec.load_state_dict(to_torch_state(case.weights), strict=False)
    assert not unexpected and not missing, (missing, unexpected)
    dec = dec.to(device).eval()
    dec.set_compute_dtype(dtype)
    return dec


def case_to_device(case, device="cuda"):
    """Move a synthetic case's tensors to the GPU (meta schema preserved)."""
    mv = lambda t: t.to(device)
    case.tgt, case.query_pos, case.reference_points = mv(case.tgt), mv(case.query_pos), mv(case.reference_points)
    if case.src_views is not None:
        case.src_views = [mv(s) for s in case.src_views]
    case.spatial_shapes, case.level_start_index = mv(case.spatial_shapes), mv(case.level_start_index)
    case.meta = [{k: ({kk: mv(vv) for kk, vv in v.items()} if isinstance(v, dict) else mv(v)) for k, v in m.items()}
                 for m in case.meta]
    return case
