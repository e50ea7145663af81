"""CPU side of the query self-attention (init_self_attention): tests/mha_ref.py pinned to the reference's own operator in
fp64, the oracle + mha_ref against the fixture the REFERENCE produced with the switch on (tests/golden/mini5_selfattn.npz,
tests/golden/make_golden_selfattn.py), and what the layer refuses."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mvgformer_amd.synthetic import to_torch_state
from tests import mha_ref as R
from tests.selfattn_cases import FIXTURE, oracle_layer, selfattn_case
from tests.test_oracle_golden import TOL_CLS, TOL_HS, TOL_MM, TOL_PX

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("Lq,B", [(1, 1), (45, 2), (130, 1)])
def test_mha_ref_is_the_reference_operator_in_fp64(Lq, B):
    gen = torch.Generator().manual_seed(Lq)
    C = 256
    tgt, pos = (torch.randn(B, Lq, C, generator=gen, dtype=torch.float64) for _ in range(2))
    W, b = torch.randn(3 * C, C, generator=gen, dtype=torch.float64) / 16, torch.randn(3 * C, generator=gen, dtype=torch.float64)
    Wo, bo = torch.randn(C, C, generator=gen, dtype=torch.float64) / 16, torch.randn(C, generator=gen, dtype=torch.float64)
    x = (tgt + pos).transpose(0, 1)
    want, _ = F.multi_head_attention_forward(x, x, tgt.transpose(0, 1), C, 8, W, b, None, None, False, 0.0, Wo, bo,
                                             training=False, need_weights=True)
    q, k, v = (tgt + pos) @ W[:C].T + b[:C], (tgt + pos) @ W[C:2 * C].T + b[C:2 * C], tgt @ W[2 * C:].T + b[2 * C:]
    got = R.attention(q, k, v) @ Wo.T + bo
    assert float((got - want.transpose(0, 1)).abs().max()) < 1e-12
    g, be = torch.randn(C, generator=gen, dtype=torch.float64), torch.randn(C, generator=gen, dtype=torch.float64)
    blk = R.block(tgt, pos, W, b, Wo, bo, g, be)
    assert float((blk - F.layer_norm(tgt + want.transpose(0, 1), (C,), g, be)).abs().max()) < 1e-12
    # the bf16 model is the same function up to bf16 rounding, and exact where nothing rounds (one key: O = V)
    m = R.attention_bf16_model(q, k, v)
    assert float((m - R.attention(R.bf(q), R.bf(k), R.bf(v))).abs().max()) < 2.0 ** -7 * float(v.abs().max())
    if Lq == 1:
        assert torch.equal(m, R.bf(v))


def test_oracle_with_mha_ref_reproduces_the_reference_fixture():
    g = np.load(os.path.join(GOLD, FIXTURE))
    case = selfattn_case()
    prm = to_torch_state(case.weights)
    thr = float(g["threshold"])
    tgt, ref = case.tgt, case.reference_points
    for l in range(case.layers):                  # teacher-forced, at the oracle's own tolerances (tests/test_oracle_golden.py)
        (hs, new_ref, r2d, p2d, cls), att = oracle_layer(prm, l, tgt, case.query_pos, ref, case, thr)
        assert float((att - tgt.double()).abs().max()) > 0.1          # the block does something
        assert np.array_equal((cls[..., 1] > thr).numpy(), g["cls"][l][..., 1] > thr)
        assert float((cls - torch.from_numpy(g["cls"][l])).abs().max()) < TOL_CLS
        assert float((hs - torch.from_numpy(g["hs"][l])).abs().max()) < TOL_HS
        assert float((p2d - torch.from_numpy(g["projs2d"][l])).abs().max()) < TOL_PX
        assert float((r2d - torch.from_numpy(g["refs2d"][l])).abs().max()) < TOL_PX
        assert float((new_ref - torch.from_numpy(g["refs"][l])).norm(dim=-1).max()) < TOL_MM
        tgt, ref = torch.from_numpy(g["hs"][l]), torch.from_numpy(g["refs"][l])


def _layer(**kw):
    from mvgformer_amd.decoder import DQDecoderLayer
    args = dict(projattn_posembed_mode="ablation_not_use_rayconv", n_levels=1, n_points=8, open_forward_ffn=True)
    args.update(kw)
    return DQDecoderLayer([8000.0, 8000.0, 2000.0], [0.0, 0.0, 800.0], [960, 512], 3, **args)


def test_check_supported_takes_the_switch_and_still_refuses_the_attention_updates():
    _layer(init_self_attention=True)._check_supported()
    _layer(init_self_attention=False)._check_supported()
    for method in ("attention", "attention_tgt_trans", "attention_tgt_embed_trans_direct"):
        with pytest.raises(NotImplementedError, match="attention\\* feature updates .* not built"):
            _layer(feature_update_method=method, init_self_attention=True)._check_supported()
    with pytest.raises(NotImplementedError, match="bayesian_update"):
        _layer(bayesian_update=True)._check_supported()


def test_the_previous_layer_does_not_precompute_the_query_term_of_a_layer_that_attends_first():
    """chain B of layer l can compute layer l + 1's query term from its own tgt_out + query_pos -- not when layer l + 1 puts its
    self-attention in front of that sum"""
    a, b = _layer(init_self_attention=True), _layer(init_self_attention=True)
    a.set_compute_dtype(torch.bfloat16), b.set_compute_dtype(torch.bfloat16)
    tgt = torch.zeros(1, 30, 256)
    assert a._next_query_term(b, "bf16", tgt, tgt, None) is None
    assert a._next_query_term(None, "bf16", tgt, tgt, None) is None


def test_cpu_tensors_raise_like_the_neighbours():
    from mvgformer_amd import ops
    q = torch.zeros(1, 4, 256)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.self_attention(q, q, q)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        _layer(init_self_attention=True).attend_queries(q, q)


def test_query_sharded_runners_refuse_coupled_queries_before_any_collective():
    """no process group exists here: the refusal comes first"""
    from mvgformer_amd import dist as D
    from tests.selfattn_cases import build_decoder
    case = selfattn_case(with_features=False)
    dec = build_decoder(case, "cpu", torch.float32)
    with pytest.raises(NotImplementedError, match="couples the queries"):
        D.sharded_decoder_forward(dec, case.tgt, case.reference_points, None, case.meta, case.spatial_shapes, case.level_start_index,
                                  case.query_pos, 0.1)
    for runner in (D.GraphedShardedDecoder, D.SpeculativeShardedDecoder):
        with pytest.raises(NotImplementedError, match="couples the queries"):
            runner(dec, case.tgt, case.reference_points, None, case.query_pos, None, 0.1, case.NQ)
    D.refuse_coupled_queries(build_decoder(case, "cpu", torch.float32, init_self_attention=False))
