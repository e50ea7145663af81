"""The seeded init_self_attention case shared by tests/golden/make_golden_selfattn.py (reference side) and the tests (oracle /
HIP side): a mini5 case of the existing kind -- 5 views, two batch elements with different validity, 10 queries (Lq = 150: three
64-key tiles, the last one ragged, two 128-row workgroups per head) -- whose self_attn weights and biases are non-trivial.
Pure numpy + torch; no reference import here."""
import numpy as np

from mvgformer_amd.synthetic import build_case

SPEC = dict(config="mini5", seed=37, layers=2, B=2, NQ=10, valid_fraction=0.5, threshold=0.1)
FIXTURE = "mini5_selfattn.npz"


def selfattn_case(with_features=True):
    case = build_case(SPEC["config"], B=SPEC["B"], seed=SPEC["seed"], NQ=SPEC["NQ"], layers=SPEC["layers"],
                      valid_fraction=SPEC["valid_fraction"], with_features=with_features)
    C = 256
    for lid in range(case.layers):
        rs = np.random.RandomState(7700 + lid)
        p = "layers.%d.self_attn." % lid
        # q, k of variance ~4 per channel: scores with a standard deviation of about 2.8, a peaked but not one-hot softmax
        w = rs.standard_normal((3 * C, C)) / np.sqrt(C)
        w[:2 * C] *= 1.2
        case.weights[p + "in_proj_weight"] = w.astype(np.float32)
        case.weights[p + "in_proj_bias"] = (0.3 * rs.standard_normal(3 * C)).astype(np.float32)
        case.weights[p + "out_proj.weight"] = (rs.standard_normal((C, C)) / np.sqrt(C)).astype(np.float32)
        case.weights[p + "out_proj.bias"] = (0.1 * rs.standard_normal(C)).astype(np.float32)
    return case


def oracle_layer(prm, lid, tgt, query_pos, ref, case, thr, **kw):
    """One reference layer with init_self_attention from the unchanged oracle + tests/mha_ref.py.  In the reference the attended
    tgt is a local of generate_features (dq_decoder.py:516-540): it replaces tgt in the projective attention's query
    tgt + query_pos and nowhere else -- update_feature (dq_decoder.py:882) adds its residual to the layer's ORIGINAL tgt.  The
    oracle reads query_pos only in that sum, so handing it query_pos + (attended - tgt) states exactly that."""
    import torch
    from oracle import decoder_ref as O
    from tests import mha_ref as R
    p = "layers.%d." % lid
    att = R.block(tgt, query_pos, prm[p + "self_attn.in_proj_weight"], prm[p + "self_attn.in_proj_bias"],
                  prm[p + "self_attn.out_proj.weight"], prm[p + "self_attn.out_proj.bias"], prm[p + "norm2.weight"],
                  prm[p + "norm2.bias"])
    qp = (query_pos.double() + (att - tgt.double())).to(torch.float32)
    return O.decoder_layer_forward(prm, p, tgt, qp, ref, case.src_views, case.spatial_shapes, case.level_start_index, case.meta,
                                   case.img_size, threshold=thr, **kw), att


def build_decoder(case, device, dtype, init_self_attention=True):
    """factory.build_decoder_for_case with the switch: the panoptic hyper-parameters and the case's seeded weights"""
    import torch  # noqa: F401
    from mvgformer_amd.decoder import DQDecoder, DQDecoderLayer
    from mvgformer_amd.synthetic import decoder_cfg, to_torch_state
    layer = DQDecoderLayer(list(case.space_size), list(case.space_center), list(case.img_size), 3,
                           256, 1024, 0.1, "relu", 1, 8, 8, True, "cat_proj", case.V,
                           "ablation_not_use_rayconv", "MLP", init_self_attention, True, "threshold",
                           visualization_jump_num=-1, bayesian_update=False, triangulation_method="linalg",
                           filter_query=True, num_joints=15)
    dec = DQDecoder(decoder_cfg(case.space_size, case.space_center), layer, case.layers, True)
    missing, unexpected = dec.load_state_dict(to_torch_state(case.weights), strict=False)
    assert not unexpected and not missing, (missing, unexpected)
    dec = dec.to(device).eval()
    dec.set_compute_dtype(dtype)
    return dec
