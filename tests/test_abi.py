"""CPU-only checks of the C-ABI boundary: the shared library loads, exports every symbol
include/mvg_decoder.h declares, the ctypes table covers them all, and the host-side mirror
has the reference's class surface.  No kernels are launched."""
import ctypes
import os
import re

import pytest
import torch

import mvgformer_amd
from mvgformer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    src = open(os.path.join(ROOT, "include", "mvg_decoder.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mvg_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    syms = _header_symbols()
    assert len(syms) >= 15
    for s in syms:
        assert hasattr(lib, s), "missing export %s" % s


def test_ctypes_table_matches_header():
    """the parser that builds the ctypes table finds exactly the names this file's own regex finds (mvg_version included), and
    each resolves in the built library with the parsed types set on it"""
    assert sorted(_lib.PROTOTYPES) == sorted(_lib.SIGNATURES) == _header_symbols()
    lib = _lib.load()
    for name, argtypes in _lib.SIGNATURES.items():
        if name != "mvg_set_tuning":                 # load() wraps this one in a Python function
            fn = getattr(lib, name)
            assert list(fn.argtypes) == argtypes and fn.restype is _lib.PROTOTYPES[name][0], name
    assert lib.mvg_version().startswith(b"mvgformer_amd")


def test_parsed_signatures_equal_the_ones_written_out_here():
    """one entry point per scalar kind, two long ones and the return types, as the hand-kept table had them before the header
    became the declaration"""
    i, f, d, z, P = ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_size_t, _lib.TensorPtr
    pinned = {
        "mvg_device_info": [ctypes.c_char_p, i, P],
        "mvg_set_tuning": [ctypes.c_char_p, i],
        "mvg_tuning_knob": [i, P, P],
        "mvg_class_head": [P, P, P, f, P, P, P, P, i, i, i, i, P],
        "mvg_pose_nms": [P, i, i, i, d, i, i, P, z, P, P, P, i, P],
        "mvg_pyramid_f32h": [P, P, i, P, P, i, P, P, ctypes.c_int64, i, P],
        "mvg_sym4_eigh": [P, P, P, ctypes.c_long, P],
        "mvg_optim_step": [P, i, P, i, P, i, P, z, P, z, P, f, i, P, P],
        "mvg_track_update": [P, P, i, i, i, i, P, P, P, P, P, P, P, P, d, i, i, P, P, P],
        "mvg_version": [],
    }
    for name, argtypes in pinned.items():
        assert _lib.SIGNATURES[name] == argtypes, name
    restypes = {name: restype for name, (restype, _) in _lib.PROTOTYPES.items()}
    assert restypes.pop("mvg_version") is ctypes.c_char_p
    assert {name for name, r in restypes.items() if r is z} == {
        "mvg_bin_pairs_workspace", "mvg_msda_backward_det_workspace", "mvg_msda_backward_bal_workspace", "mvg_knn_match_workspace",
        "mvg_hungarian_match_workspace", "mvg_criterion_workspace", "mvg_optim_workspace", "mvg_pose_nms_workspace",
        "mvg_self_attention_backward_workspace"}
    assert all(r is z or r is i for r in restypes.values())
    assert issubclass(P, ctypes.c_void_p) and ctypes.sizeof(P) == ctypes.sizeof(ctypes.c_void_p)


def test_parser_reads_a_header_text_and_refuses_what_it_does_not_know():
    protos, defines = _lib.parse_header("""
        /* int mvg_in_a_comment(int x); */
        #define MVG_N 7   /* a limit */
        #define MVG_BIG 1e15
        #define MVG_GUARD
        extern "C" {
        int mvg_a(const float* const* x, int64_t n,
                  const char* key, void* stream);
        size_t mvg_b(void);
        }""")
    assert defines == {"MVG_N": 7, "MVG_BIG": 1e15} and isinstance(defines["MVG_N"], int) and isinstance(defines["MVG_BIG"], float)
    assert protos == {"mvg_a": (ctypes.c_int, [(_lib.TensorPtr, "x"), (ctypes.c_int64, "n"), (ctypes.c_char_p, "key"),
                                                 (_lib.TensorPtr, "stream")]), "mvg_b": (ctypes.c_size_t, [])}
    for bad in ("int mvg_a(unsigned n);", "int mvg_a(struct dims d);", "int mvg_a(int);", "short mvg_a(int n);", "float* mvg_a(int n);",
                "int mvg_a(int n", "int mvg_a(int n[3]);", "typedef int mvg_t;", "#define MVG_N (3 + 4)\nint mvg_a(int n);"):
        with pytest.raises(_lib.MvgError, match="mvg_decoder.h"):
            _lib.parse_header(bad)


def test_header_defines_are_numbers():
    D = _lib.DEFINES
    assert isinstance(D["MVG_LAP_BIG"], float) and D["MVG_LAP_BIG"] == 1e15
    assert isinstance(D["MVG_NMS_MAX_N"], int) and D["MVG_NMS_MAX_N"] == 2048
    assert D["MVG_E_BADARG"] == 10001 and (D["MVG_F32"], D["MVG_BF16"]) == (0, 1) == (_lib.MVG_F32, _lib.MVG_BF16)
    assert all(k.startswith("MVG_") and type(v) in (int, float) for k, v in D.items()) and "MVG_DECODER_H" not in D
    from mvgformer_amd import ops
    assert ops.MATCH_METHODS == {"KNN": 0, "multiple": 1} and ops.HUNGARIAN_METHODS == {"hungarian": 2, "hungarian-dis": 3}
    assert ops.ST_METHODS == {"LS": 0, "ST": 1} and (ops.HUNGARIAN_MAX_G, ops.HUNGARIAN_MAX_NQ) == (64, 4096)
    assert (ops.OPTIM_CHUNK, ops.OPTIM_TENSOR_WORDS, ops.OPTIM_GROUP_WORDS, ops.OPTIM_STATE_HEADER, ops.OPTIM_STATE_PER_GROUP) \
        == (4096, 6, 6, 64, 16)


def test_tensor_pointer_argtype():
    """_lib.TensorPtr through libc's memcmp: a tensor passes its data pointer, everything c_void_p takes still passes, a zero-element
    tensor is NULL, a Python float is refused"""
    libc = ctypes.CDLL(None)
    memcmp = libc.memcmp
    memcmp.argtypes, memcmp.restype = [_lib.TensorPtr, _lib.TensorPtr, ctypes.c_size_t], ctypes.c_int
    data = [3, 1, 4, 1, 5, 9, 2, 6]
    t = torch.tensor(data, dtype=torch.uint8)
    arr = (ctypes.c_uint8 * 8)(*data)
    for other in (arr, ctypes.c_void_p(ctypes.addressof(arr)), ctypes.addressof(arr), ctypes.byref(arr), t.clone(), _lib.ptr(t)):
        assert memcmp(t, other, 8) == 0 and memcmp(other, t, 8) == 0
    assert memcmp(t, torch.tensor(data[:7] + [7], dtype=torch.uint8), 8) != 0
    assert memcmp(t[2:], (ctypes.c_uint8 * 2)(4, 1), 2) == 0                    # a view passes where it starts
    empty = torch.empty((0,), dtype=torch.uint8)
    assert memcmp(empty, None, 0) == 0 and memcmp(None, t, 0) == 0
    assert _lib.TensorPtr.from_param(empty) is None and _lib.TensorPtr.from_param(None) is None      # NULL, as ctypes passes it
    with pytest.raises(ctypes.ArgumentError):
        memcmp(t, 1.5, 8)


def test_camera_stride_matches_header():
    src = open(os.path.join(ROOT, "include", "mvg_decoder.h")).read()
    assert int(re.search(r"#define MVG_CAM_STRIDE (\d+)", src).group(1)) == _lib.CAM_STRIDE


def test_state_dict_surface_matches_reference():
    """32 entries / 1 169 861 parameters per layer, names per SURVEY.md section 8(b)."""
    from mvgformer_amd.factory import build_decoder_for_case
    from mvgformer_amd.synthetic import build_case
    case = build_case("mini5", with_features=False)
    dec = build_decoder_for_case(case, device="cpu")
    sd = dec.state_dict()
    per_layer = [k for k in sd if k.startswith("layers.0.")]
    assert len(per_layer) == 32
    assert sum(p.numel() for p in dec.layers[0].parameters()) == 1169861
    assert sd["layers.0.proj_attn.sampling_offsets.weight"].shape == (128, 256)
    assert sd["layers.0.proj_attn.attention_weights.weight"].shape == (64, 256)
    assert sd["layers.0.pose_embed.MLP.layers.2.weight"].shape == (3, 256)
    assert sd["layers.0.self_attn.in_proj_weight"].shape == (768, 256)
    assert sd["layers.0.class_embed.weight"].shape == (2, 256)
    assert mvgformer_amd.MSDeformAttn is mvgformer_amd.ProjAttn
    assert mvgformer_amd.MultiViewDecoderLayer is mvgformer_amd.DQDecoderLayer


def test_cpu_tensors_raise_like_the_reference_stub():
    # lib/models/ops/src/deform.h:49 -> "Not implemented on the CPU"
    from mvgformer_amd import deformable
    from tests.golden.cases import msda_case
    c = msda_case("edge_f32")
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        deformable.deform_forward(c["value"], c["shapes"], c["starts"], c["loc"], c["weight"], 64)


def test_reference_yaml_entry_point_is_readable(tmp_path):
    """the panoptic YAML keys the decoder needs (configs/panoptic/knn5-lr4-q1024-g8.yaml)."""
    from mvgformer_amd.factory import build_decoder_from_cfg, load_yaml_config
    y = tmp_path / "cfg.yaml"
    y.write_text("""
DATASET: {CAMERA_NUM: 5}
NETWORK: {IMAGE_SIZE: [960, 512]}
MULTI_PERSON: {SPACE_SIZE: [8000.0, 8000.0, 2000.0], SPACE_CENTER: [0.0, -500.0, 800.0]}
DECODER: {d_model: 256, nhead: 8, dim_feedforward: 1024, num_feature_levels: 1, dec_n_points: 8,
          num_decoder_layers: 4, num_instance: 1024, num_keypoints: 15, feature_update_method: MLP,
          init_self_attention: false, open_forward_ffn: true, projattn_posembed_mode: ablation_not_use_rayconv}
""")
    cfg = load_yaml_config(str(y))
    dec = build_decoder_from_cfg(cfg)
    assert len(dec.layers) == 4 and dec.layers[0].proj_attn.n_points == 8


def test_every_reference_yaml_entry_point_builds_a_decoder():
    """The reference's REAL YAML entry points (configs/panoptic/knn5-lr4-q1024-g8.yaml and the 11 others).  In the build
    container they are opened where they lie under /root/reference and must (a) load through factory.load_yaml_config, (b)
    build a decoder on the supported hot path and (c) equal the committed extract of their values
    (mvgformer_amd/data/yaml_extract.json, made by tests/golden/make_yaml_extract.py); on the GPU box, where the reference does
    not exist, the decoders are built from the extract alone."""
    import json
    import os
    from types import SimpleNamespace
    from mvgformer_amd.factory import build_decoder_from_cfg, load_yaml_config
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(os.path.dirname(here), "mvgformer_amd", "data", "yaml_extract.json")) as f:
        extract = json.load(f)
    assert "configs/panoptic/knn5-lr4-q1024-g8.yaml" in extract and len(extract) == 12
    ref = os.environ.get("MVG_REFERENCE", "/root/reference")
    for rel, val in extract.items():
        if os.path.isdir(ref):
            from tests.golden.make_yaml_extract import flatten
            assert flatten(load_yaml_config(os.path.join(ref, rel))) == val, rel
        cfg = SimpleNamespace(DECODER=SimpleNamespace(**val["DECODER"]), NETWORK=SimpleNamespace(IMAGE_SIZE=val["IMAGE_SIZE"]),
                              MULTI_PERSON=SimpleNamespace(SPACE_SIZE=val["SPACE_SIZE"], SPACE_CENTER=val["SPACE_CENTER"]),
                              DATASET=SimpleNamespace(CAMERA_NUM=val["CAMERA_NUM"]))
        dec = build_decoder_from_cfg(cfg)
        assert len(dec.layers) == val["DECODER"]["num_decoder_layers"] == 4
        layer = dec.layers[0]
        layer._check_supported()                                  # every shipped YAML is on the built hot path
        assert layer.proj_attn.n_points == 8 and layer.proj_attn.n_heads == 8 and layer.num_joints == 15
        assert len(layer.state_dict()) == 32


def test_host_level_tables_are_cached_per_tensor_and_follow_in_place_updates():
    """ops.host_levels keeps the host copy of (spatial_shapes, level_start_index) on the tensor object (so the deterministic
    backward sizes its workspace without a D2H sync per call) and drops it when the tensor is modified in place."""
    import torch
    from mvgformer_amd import ops
    shapes = torch.tensor([[8, 12], [4, 6]], dtype=torch.long)
    starts = torch.tensor([0, 96], dtype=torch.long)
    a = ops.host_levels(shapes, starts)
    b = ops.host_levels(shapes, starts)
    assert a[0] is b[0] and a[1] is b[1]                       # second lookup: the cached ctypes arrays
    assert list(a[0]) == [8, 12, 4, 6] and list(a[1]) == [0, 96]
    shapes[1, 0] = 5                                           # bumps the version counter
    c = ops.host_levels(shapes, starts)
    assert c[0] is not a[0] and list(c[0]) == [8, 12, 5, 6] and c[1] is a[1]
    other = ops.host_levels(shapes.clone(), starts)            # a different tensor object never sees somebody else's copy
    assert other[0] is not c[0] and list(other[0]) == [8, 12, 5, 6]


def test_only_the_product_and_checker_libraries_ship():
    """The tree that travels to the GPU box holds exactly two kinds of shared objects: the product (libmvgformer_hip.so) and the
    oracle's C checker (libmsda_ref.so, oracle/_ref/*).  Experiment builds left in the package directory would ship with every
    push and could be loaded by accident."""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    allowed = {os.path.join("mvgformer_amd", "libmvgformer_hip.so"), os.path.join("oracle", "libmsda_ref.so")}
    found = set()
    for base, dirs, files in os.walk(root):
        dirs[:] = [d for d in dirs if d not in (".git", "gpurun_out", "__pycache__", ".pytest_cache", "_ref", "build")]
        for name in files:
            if name.endswith(".so") or ".so." in name:
                found.add(os.path.relpath(os.path.join(base, name), root))
    assert found <= allowed, sorted(found - allowed)


def test_deepcopy_of_a_decoder_does_not_copy_run_time_buffers():
    """copy.deepcopy(decoder) (EMA / checkpoint copies): parameters are copied, the product buffers (ahead and inline pairs), their
    ready state, weight caches and side-stream hand-offs are not; the copy's layers share ONE fresh, empty owner again --
    by PyramidProducts.__deepcopy__ alone, without a __deepcopy__ on the modules."""
    import copy
    from mvgformer_amd.decoder import DQDecoder
    from mvgformer_amd.factory import build_decoder_for_case
    from mvgformer_amd.projattn import ProjAttn
    from mvgformer_amd.synthetic import build_case
    dec = build_decoder_for_case(build_case("cfg1", seed=0, layers=2), "cpu", torch.float32)
    pa0, cpu = dec.layers[0].proj_attn, torch.device("cpu")
    assert all(l.proj_attn.products is dec.products for l in dec.layers)
    inline = dec.products.buffers(pa0, torch.float32, 1, 4, 256, cpu, ahead=False, stream=0)
    ahead = dec.products.buffers(pa0, torch.float32, 1, 4, 256, cpu, ahead=True)
    dec.products.produced([pa0], event=object())
    assert len(dec.products.tensors()) == 4 and dec.products.pending() and inline[0] is not ahead[0]
    dec.layers[0]._run = None
    cp = copy.deepcopy(dec)
    assert all(l._run is None for l in cp.layers)
    assert cp.products.tensors() == [] and cp.products.signature() == () and not cp.products.pending()
    assert all(l.proj_attn.products is cp.products for l in cp.layers) and cp.products is not dec.products
    assert len(dec.products.tensors()) == 4 and dec.products.pending()         # the original keeps its own
    a, b = dec.state_dict(), cp.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) and a[k].data_ptr() != b[k].data_ptr() for k in a)
    single = copy.deepcopy(pa0)
    assert single.products.tensors() == [] and not single.products.pending()
    assert single.products is not dec.products and single.products is not cp.products
    assert "__deepcopy__" not in vars(ProjAttn) and "__deepcopy__" not in vars(DQDecoder)


def test_a_forward_that_raises_leaves_no_run_attached():
    """DecoderRun is the one place per-forward state lives: DQDecoder.forward attaches it to the layers and detaches it however the
    forward ends.  On the CPU the first layer refuses to run; afterwards no layer holds a run.  A layer on its own never has one."""
    import pytest
    from mvgformer_amd.decoder import DQDecoderLayer
    from mvgformer_amd.factory import build_decoder_for_case, case_to_device
    from mvgformer_amd.synthetic import build_case
    case = build_case("cfg1", seed=0, layers=2)
    dec = build_decoder_for_case(case, "cpu", torch.float32)
    assert all(l._run is None for l in dec.layers)
    c = case_to_device(case, "cpu")
    with torch.no_grad(), pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        dec(c.tgt, c.reference_points, c.src_views, c.meta, c.spatial_shapes, c.level_start_index, None, query_pos=c.query_pos,
            threshold=0.1)
    assert all(l._run is None for l in dec.layers)
    layer = DQDecoderLayer([8000.0, 8000.0, 2000.0], [0.0, 0.0, 800.0], [960, 512], 3)
    assert layer._run is None
