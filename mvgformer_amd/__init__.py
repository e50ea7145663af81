"""mvgformer_amd -- MI355X-native implementation of the MVGFormer decoder hot path.

Host-side mirror of the reference's operator interface (same names / signatures):
  Deformable op   : mvgformer_amd.deformable.deform_forward / deform_backward
  DeformFunction  : mvgformer_amd.functions.DeformFunction
  ProjAttn        : mvgformer_amd.projattn.ProjAttn            (alias MSDeformAttn)
  DQDecoderLayer  : mvgformer_amd.decoder.DQDecoderLayer       (alias MultiViewDecoderLayer)
  DQDecoder       : mvgformer_amd.decoder.DQDecoder
  Criterion       : mvgformer_amd.criterion.KNNMatcher / HungarianMatcher / SetCriterion / criterion_all_layers / total_loss,
                    factory.build_matcher_from_cfg (the reference's default match_method 'hungarian' on the device)
  Optimizer step  : mvgformer_amd.optim.FusedAdam / factory.build_optimizer_from_cfg (clip_grad_norm_ + Adam / AdamW)
All compute goes through libmvgformer_hip.so (include/mvg_decoder.h); there is no CPU path.
"""
from .decoder import MLP, DQDecoder, DQDecoderLayer, MultiViewDecoder, MultiViewDecoderLayer, offset_net  # noqa: F401
from .criterion import HungarianMatcher, KNNMatcher, SetCriterion, criterion_all_layers, total_loss  # noqa: F401
from .factory import build_matcher_from_cfg, build_optimizer_from_cfg  # noqa: F401
from .functions import CriterionFunction, DeformFunction  # noqa: F401
from .optim import FusedAdam  # noqa: F401
from .projattn import MSDeformAttn, ProjAttn  # noqa: F401

__version__ = "0.1.0"
