"""Generate tests/golden/mini5_selfattn.npz by RUNNING THE REFERENCE with DECODER.init_self_attention = True.

Run in the build container only (needs the reference tree):

    python -m tests.golden.make_golden_selfattn

The reference's DQDecoderLayer / DQDecoder are built with the query self-attention switched on (dq_decoder.py:257,532-539), two
layers, on the seeded case of tests/selfattn_cases.py.  The fixture holds arrays only: the decoder's stacked outputs (layer 0's
slices are what that layer returns when called on its own)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from mvgformer_amd.synthetic import decoder_cfg, to_torch_state  # noqa: E402
from tests.golden.cases import threshold_margin  # noqa: E402
from tests.golden.ref_harness import load_reference  # noqa: E402
from tests.selfattn_cases import FIXTURE, SPEC, selfattn_case  # noqa: E402


def npy(t):
    return t.detach().cpu().numpy()


def build_reference_decoder(ref, case):
    layer = ref.DQDecoderLayer(
        list(case.space_size), list(case.space_center), list(case.img_size), 3,
        256, 1024, 0.1, "relu", 1, 8, 8, True, "cat_proj", case.V,
        "ablation_not_use_rayconv", "MLP", True, True, "threshold",          # feature_update_method, init_self_attention, open_forward_ffn
        visualization_jump_num=-1, bayesian_update=False, triangulation_method="linalg",
        filter_query=True, num_joints=15)
    assert layer.init_self_attention is True
    dec = ref.DQDecoder(decoder_cfg(case.space_size, case.space_center), layer, case.layers, True)
    missing, unexpected = dec.load_state_dict(to_torch_state(case.weights), strict=False)
    assert not unexpected, unexpected
    assert all(k.endswith(("grid_size", "grid_center")) for k in missing), missing
    return dec.eval()


def main():
    ref = load_reference()
    torch.manual_seed(0)
    case = selfattn_case()
    dec = build_reference_decoder(ref, case)
    thr = SPEC["threshold"]
    pad = [torch.zeros(1, 1, dtype=torch.bool)]
    with torch.no_grad():
        hs, refs, r2d, p2d, cls = dec(case.tgt, case.reference_points, case.src_views, case.meta, case.spatial_shapes,
                                      case.level_start_index, None, query_pos=case.query_pos, src_padding_mask=pad, threshold=thr)
    margin = threshold_margin(cls, thr)
    assert margin > 1e-3, "class prob within %.2e of the threshold" % margin
    print("valid/layer", [int((c[..., 1] > thr).sum()) for c in cls], "of", case.B * case.NQ, "margin %.3e" % margin)
    out = dict(hs=npy(hs), refs=npy(refs), refs2d=npy(r2d), projs2d=npy(p2d), cls=npy(torch.stack(cls)),
               threshold=np.float32(thr))
    path = os.path.join(HERE, FIXTURE)
    np.savez_compressed(path, **out)
    print("  ->", path, "%.0f KB" % (os.path.getsize(path) / 1024), {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
