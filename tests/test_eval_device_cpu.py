"""Device-side validation scoring (csrc/evalacc.hip, ops.eval_*, evaluate.DeviceEvaluator, validate --device-eval): what can be
checked without a GPU -- the C-ABI surface, the refusals, the argument parser.  The numerics are in tests/test_eval_device_gpu.py."""
import ctypes
import os
import re

import pytest
import torch

from mvgformer_amd import _lib
from mvgformer_amd import evaluate as E
from mvgformer_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mvg_eval_match", "mvg_eval_pcp")


def test_symbols_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvg_decoder.h")).read(), flags=re.S)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in _lib.SIGNATURES and hasattr(lib, s), s
    # one ctypes entry per declared parameter
    for s in SYMBOLS:
        params = re.search(r"\b%s\s*\((.*?)\)\s*;" % s, header, flags=re.S).group(1).split(",")
        assert len(params) == len(_lib.SIGNATURES[s]), s
    assert int(re.search(r"#define MVG_EVAL_STATE_WORDS (\d+)", header).group(1)) == len(ops.EVAL_STATE)
    for name, value in (("R", ops.EVAL_MAX_R), ("J", ops.EVAL_MAX_J), ("G", ops.EVAL_MAX_G), ("B", ops.EVAL_MAX_B)):
        assert int(re.search(r"#define MVG_EVAL_MAX_%s (\d+)" % name, header).group(1)) == value


def _cpu_inputs(B=1, R=4, J=15, G=2):
    dets = torch.zeros((B, R, J, 5))
    count = torch.zeros((B, 2), dtype=torch.int32)
    return dets, count, torch.zeros((B, G, J, 3)), torch.zeros((B, G, J)), torch.zeros((B,), dtype=torch.int32)


def test_cpu_tensors_raise_like_every_other_operator():
    buffers = ops.eval_buffers(8, 4, "cpu")
    assert set(buffers) == {"mpjpe", "score", "gt_id", "correct", "total", "bone_correct", "state"}
    assert buffers["state"].dtype == torch.int64 and buffers["state"].numel() == len(ops.EVAL_STATE)
    assert all(int(t.abs().sum()) == 0 for t in buffers.values()) and tuple(buffers["bone_correct"].shape) == (4, 10)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.eval_match(*_cpu_inputs(), buffers)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.eval_pcp(*_cpu_inputs(J=14), buffers)
    for kind, J in (("panoptic", 15), ("pcp", 14)):
        ev = E.DeviceEvaluator(kind=kind, capacity=8, device="cpu")
        with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
            ev.update(*_cpu_inputs(J=J))


def test_evaluator_refuses_what_stays_on_the_host():
    assert "DeviceEvaluator" in E.__all__
    with pytest.raises(ValueError, match="kind"):
        E.DeviceEvaluator(kind="coco", device="cpu")
    ev = E.DeviceEvaluator(kind="panoptic", capacity=8, device="cpu")
    with pytest.raises(ValueError, match="mpjpe_sort"):
        ev.panoptic(method="mpjpe_sort")
    with pytest.raises(ValueError, match="max_persons"):
        ev.update(*_cpu_inputs(G=11))
    with pytest.raises(ValueError):
        ev.pcp()
    with pytest.raises(ValueError):
        E.DeviceEvaluator(kind="pcp", capacity=8, device="cpu").eval_list()
    # an empty evaluator reads back as the host's empty list
    lst, total_gt = ev.eval_list()
    assert total_gt == 0 and all(len(v) == 0 for v in lst.values()) and lst["gt_id"].dtype.kind == "i"


def test_validate_parser_knows_device_eval(capsys):
    from mvgformer_amd import validate
    with pytest.raises(SystemExit) as e:
        validate.main(["--cfg", "extract:configs/panoptic/knn5-lr4-q1024-g8.yaml", "--device-eval", "1", "--device-nms", "0"])
    assert e.value.code == 2 and "--device-nms 1" in capsys.readouterr().err
    # accepted together with --device-nms 1: the run then stops where every CPU run of validate stops
    with pytest.raises(SystemExit) as e:
        validate.main(["--cfg", "extract:configs/panoptic/knn5-lr4-q1024-g8.yaml", "--device", "cpu", "--device-eval", "1",
                       "--device-nms", "1"])
    assert e.value.code == "Not implemented on the CPU"
