"""CPU-only checks of the tables of mvg_refresh_operands as training.TrainOperands builds them for a decoder head: which weights get
a (W16, W16^T) pair, how the concatenated ProjAttn weight is split into records, that the tiles cover every record exactly once,
and that the builder's record layout is the header's.  No library call, no kernel."""
import os
import re

import torch

from mvgformer_amd import ops
from mvgformer_amd.caller import DecoderHead
from mvgformer_amd.factory import build_decoder_for_case
from mvgformer_amd.synthetic import build_case
from mvgformer_amd.training import RECORD_WORDS, TILE, TrainOperands, build_tables, operand_specs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _head(layers=2):
    case = build_case("mini5", seed=4, NQ=128, layers=layers, with_features=False)
    dec = build_decoder_for_case(case, "cpu", torch.float32)
    return DecoderHead(dec, case.NQ, 15, 256, case.space_size, case.space_center), dec


def _call_sites():
    """The linear_bf16 call sites, read from the SOURCE of the package: (cache key expression, weight expression) of every call of
    functions.linear_bf16 in projattn.py, and the weight expression of every call of `lin` -- which is DQDecoderLayer._lin_bf16
    under training_dtype bfloat16 -- in decoder.py's forward_autograd.  A new call site shows up here and fails the test below
    until training.operand_specs knows it.  (End to end the check is the bf16 capture on the GPU, which raises in WeightCache.get
    for a weight without an adopted pair: tests/test_train_graph_gpu.py.)"""
    import ast
    pkg = os.path.join(ROOT, "mvgformer_amd")
    name = lambda f: f.id if isinstance(f, ast.Name) else f.attr if isinstance(f, ast.Attribute) else None     # noqa: E731
    direct, callers = [], {}
    for fn in sorted(os.listdir(pkg)):
        if not fn.endswith(".py") or fn == "functions.py":
            continue
        tree = ast.parse(open(os.path.join(pkg, fn)).read())
        for func in [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)]:
            for call in [n for n in ast.walk(func) if isinstance(n, ast.Call) and name(n.func) == "linear_bf16"]:
                direct.append((fn, func.name, ast.unparse(call.args[4]), ast.unparse(call.args[1])))
                callers[(fn, func.name)] = True
    tree = ast.parse(open(os.path.join(pkg, "decoder.py")).read())
    fa = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "forward_autograd")
    via_lin = sorted({ast.unparse(c.args[1]) for c in ast.walk(fa) if isinstance(c, ast.Call) and name(c.func) == "lin"})
    users = sorted({(fn, f.name) for fn in os.listdir(pkg) if fn.endswith(".py")
                    for f in ast.walk(ast.parse(open(os.path.join(pkg, fn)).read())) if isinstance(f, ast.FunctionDef)
                    for a in ast.walk(f) if isinstance(a, ast.Attribute) and a.attr == "_lin_bf16"})
    return sorted(direct), via_lin, users


# weight expression at a call site -> the parameters its cache entry is stamped with
_PROJATTN = {"self.rayconv.weight": lambda pa: (pa.rayconv.weight,),
             "w_oa": lambda pa: (pa.sampling_offsets.weight, pa.attention_weights.weight),
             "self.output_proj.weight": lambda pa: (pa.output_proj.weight,)}
_LAYER = {"self.feature_update_mlp.weight": lambda l: [l.feature_update_mlp.weight],
          "self.linear1.weight": lambda l: [l.linear1.weight], "self.linear2.weight": lambda l: [l.linear2.weight],
          "self.class_embed.weight": lambda l: [l.class_embed.weight],
          "layer_.weight": lambda l: [m.weight for m in l.pose_embed.MLP.layers]}


def _linear_bf16_weights(dec):
    """the expectation, derived from the call sites, with the rule of functions.linear_bf16: LinearBF16 -- and so a cached pair -- only
    where both widths are multiples of 64"""
    direct, via_lin, users = _call_sites()
    # linear_bf16 is called from ProjAttn.forward (three weights) and from _lin_bf16 alone; _lin_bf16 is used by forward_autograd alone
    assert sorted({(fn, f) for fn, f, _, _ in direct}) == [("decoder.py", "_lin_bf16"), ("projattn.py", "forward")], direct
    assert users == [("decoder.py", "forward_autograd")], users
    assert [d[2:] for d in direct if d[0] == "decoder.py"] == [("'train16/%x' % id(weight)", "weight")], direct
    want = []
    for layer in dec.layers:
        pa = layer.proj_attn
        cands = [(pa._wc, eval(key), _PROJATTN[w](pa)) for fn, _, key, w in direct if fn == "projattn.py"]     # KeyError: new site
        for w_expr in via_lin:
            cands += [(layer._wc, "train16/%x" % id(w), (w,)) for w in _LAYER[w_expr](layer)]
        for cache, key, params in cands:
            N, K = sum(p.shape[0] for p in params), params[0].shape[1]
            if N % 64 == 0 and K % 64 == 0:
                want.append((id(cache), key, tuple(id(p) for p in params)))
    return want


def test_every_linear_bf16_weight_has_exactly_one_destination_pair():
    head, dec = _head()
    got = [(id(c), k, tuple(id(p) for p in ps)) for c, k, ps in operand_specs(head)]
    want = _linear_bf16_weights(dec)
    assert sorted(got) == sorted(want) and len(set(got)) == len(got)
    # per layer: rayconv, [offsets; logits], output_proj, feature_update_mlp, linear1, linear2, the first two pose layers;
    # class_embed (2 outputs) and the last pose layer (3 outputs) stay on fp32 operands
    assert len(got) == 8 * len(dec.layers)
    layer = dec.layers[0]
    keys = {k for c, k, _ in operand_specs(head) if c is layer._wc}
    assert "train16/%x" % id(layer.class_embed.weight) not in keys
    assert "train16/%x" % id(layer.pose_embed.MLP.layers[-1].weight) not in keys
    assert "train16/%x" % id(layer.pose_embed.MLP.layers[0].weight) in keys
    # operand_specs(decoder) == operand_specs(head)
    assert [(k, ps) for _, k, ps in operand_specs(dec)] == [(k, ps) for _, k, ps in operand_specs(head)]


def test_tables_on_a_cpu_head_records_offsets_and_tiles():
    head, dec = _head()
    t = TrainOperands(head)                     # CPU parameters: buffers and host tables only, nothing uploaded or launched
    assert t.record_table is None and t.tile_table is None
    rec, tiles = t.record_table_host, t.tile_table_host
    assert rec.dtype == torch.int64 and rec.shape[1] == RECORD_WORDS == ops.OPERANDS_RECORD_WORDS
    assert tiles.dtype == torch.int32 and tiles.shape[1] == 2
    # one record per source parameter: 9 per layer (the concatenated weight gives two)
    assert rec.shape[0] == 9 * len(dec.layers)
    rows = {int(r[0]): r.tolist() for r in rec}
    for cache, key, params, w16, w16t in t.entries:
        N, K = w16.shape
        assert w16.dtype == w16t.dtype == torch.bfloat16 and tuple(w16t.shape) == (K, N)
        row = 0
        for p in params:
            src, n, k, ld, dst, dst_ld, dstT, dstT_ld = rows[p.data_ptr()]
            assert (n, k, ld) == (p.shape[0], p.shape[1], p.stride(0)) and k == K
            assert dst == w16.data_ptr() + row * K * 2 and dst_ld == K          # row offset
            assert dstT == w16t.data_ptr() + row * 2 and dstT_ld == N           # column offset, the WHOLE buffer's row length
            row += n
        assert row == N
    # the concatenated weight: two records into one (192, 256) / (256, 192) pair
    pa = dec.layers[0].proj_attn
    entry = [e for e in t.entries if e[0] is pa._wc and e[1] == "train16/Woa"]
    assert len(entry) == 1
    _, _, params, w16, w16t = entry[0]
    assert tuple(w16.shape) == (192, 256) and tuple(w16t.shape) == (256, 192) and len(params) == 2
    r_off, r_att = rows[pa.sampling_offsets.weight.data_ptr()], rows[pa.attention_weights.weight.data_ptr()]
    assert (r_off[1], r_att[1]) == (128, 64)
    assert r_off[4] == w16.data_ptr() and r_att[4] == w16.data_ptr() + 128 * 256 * 2
    assert r_off[6] == w16t.data_ptr() and r_att[6] == w16t.data_ptr() + 128 * 2 and r_off[7] == r_att[7] == 192
    # destinations of different entries do not overlap
    spans = sorted((x.data_ptr(), x.data_ptr() + x.numel() * 2) for e in t.entries for x in e[3:5])
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))


def _covered_once(rec, tiles):
    per = {}
    for r, ti in tiles.tolist():
        per.setdefault(r, []).append(ti)
    assert sorted(per) == list(range(rec.shape[0]))
    for r, got in per.items():
        n, k = int(rec[r, 1]), int(rec[r, 2])
        want = -(-n // TILE) * -(-k // TILE)
        assert sorted(got) == list(range(want)), (r, n, k)
        # every element lies in exactly one tile
        cover = torch.zeros((n, k), dtype=torch.int32)
        tk = -(-k // TILE)
        for ti in got:
            n0, k0 = (ti // tk) * TILE, (ti % tk) * TILE
            cover[n0:n0 + TILE, k0:k0 + TILE] += 1
        assert bool((cover == 1).all())


def test_tiles_cover_every_record_exactly_once():
    head, _ = _head(layers=1)
    t = TrainOperands(head)
    _covered_once(t.record_table_host, t.tile_table_host)
    # shapes that are no multiple of the tile, through the builder alone
    srcs = [torch.zeros((70, 128)), torch.zeros((1, 64)), torch.zeros((130, 192))]
    entries = [((s,), torch.zeros(s.shape, dtype=torch.bfloat16), torch.zeros(s.shape[::-1], dtype=torch.bfloat16)) for s in srcs]
    rec, tiles = build_tables(entries)
    assert [int(x) for x in rec[:, 1]] == [70, 1, 130]
    _covered_once(rec, tiles)
    assert tiles.shape[0] == 2 * 2 + 1 * 1 + 3 * 3


def test_record_layout_is_the_headers():
    src = open(os.path.join(ROOT, "include", "mvg_decoder.h")).read()
    assert int(re.search(r"#define MVG_OPERANDS_RECORD_WORDS (\d+)", src).group(1)) == RECORD_WORDS
    assert int(re.search(r"#define MVG_OPERANDS_TILE (\d+)", src).group(1)) == TILE
    hip = open(os.path.join(ROOT, "mvgformer_amd", "csrc", "operands.hip")).read()
    body = re.search(r"struct OpdRecord \{(.*?)\};", hip, flags=re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    fields = [f for decl in body.split(";") if decl.strip()
              for f in re.findall(r"[A-Za-z_]\w*", re.sub(r"^\s*(const\s+)?\w+\s*\*?", "", decl, count=1))]
    assert fields == ["src", "N", "K", "src_ld", "dst", "dst_ld", "dstT", "dstT_ld"] and len(fields) == RECORD_WORDS


def test_weight_cache_adoption_is_additive():
    """a cache with nothing adopted behaves as before; an adopted entry is returned while its stamp holds, restamp() follows a
    version bump, and a stale adopted entry is rebuilt INTO the adopted tensor (its address stays)"""
    from mvgformer_amd.projattn import WeightCache
    w = torch.nn.Parameter(torch.randn(4, 4))
    plain = WeightCache()
    a = plain.get("k", (w,), torch.bfloat16)
    assert plain.get("k", (w,), torch.bfloat16) is a
    with torch.no_grad():
        w.add_(1.0)
    b = plain.get("k", (w,), torch.bfloat16)
    assert b is not a and torch.equal(b, w.detach().to(torch.bfloat16))
    wc = WeightCache()
    mine = torch.zeros((4, 4), dtype=torch.bfloat16)
    wc.adopt("k", (w,), torch.bfloat16, mine)
    assert wc.get("k", (w,), torch.bfloat16) is mine
    torch.autograd.graph.increment_version([w])         # an update through raw pointers, as FusedAdam bumps it
    wc.restamp()
    assert wc.get("k", (w,), torch.bfloat16) is mine and not bool(mine.any())      # stamped current, not rebuilt
    with torch.no_grad():
        w.mul_(2.0)                                      # somebody else's write: stale
    got = wc.get("k", (w,), torch.bfloat16)
    assert got is mine and torch.equal(mine, w.detach().to(torch.bfloat16))
    assert wc.get("other", (w,), torch.float32) is not mine
    import copy
    cp = copy.deepcopy(wc)                               # adopted entries stay with the original, the others are copied
    assert set(cp._store) == {"other"} and cp._adopted == {} and set(copy.deepcopy(plain)._store) == {"k"}
