"""CPU checks of the balanced mode of the sampling backward (csrc/msda_bwd.hip): its three C symbols, the host-side workspace function
and the chunk rule.  Nothing here touches a device: the workspace function is host arithmetic, and an illegal chunk is refused before
the entry point looks at its device."""
import ctypes as C
import os
import re

import pytest

from mvgformer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MVG_E_BADARG = 10001
NAMES = ("mvg_msda_backward_bal_workspace", "mvg_msda_backward_bal_f32", "mvg_msda_backward_bal_bf16")
CFG2 = dict(N=5, S=40320, M=8, D=32, L=3, Lq=15360, P=8, shapes=[(128, 240), (64, 120), (32, 60)])
SMALL = dict(N=2, S=657, M=2, D=32, L=2, Lq=160, P=4, shapes=[(20, 27), (9, 13)])


def _i64(shapes):
    flat = [int(x) for hw in shapes for x in hw]
    return (C.c_int64 * len(flat))(*flat)


def _dims(s, **over):
    s = dict(s, **over)
    return (s["N"], s["S"], s["M"], s["D"], s["L"], s["Lq"], s["P"]), _i64(s["shapes"])


def test_symbols_are_in_the_header_the_signatures_and_the_library():
    header = open(os.path.join(ROOT, "include", "mvg_decoder.h")).read()
    assert re.search(r"\bsize_t\s+mvg_msda_backward_bal_workspace\s*\(", header)
    for name in NAMES[1:]:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    # the det signatures plus `int chunk`
    assert _lib.SIGNATURES["mvg_msda_backward_bal_workspace"] == _lib.SIGNATURES["mvg_msda_backward_det_workspace"] + [C.c_int]
    assert _lib.SIGNATURES["mvg_msda_backward_bal_f32"] == _lib.SIGNATURES["mvg_msda_backward_det_f32"] + [C.c_int]
    assert _lib.SIGNATURES["mvg_msda_backward_bal_bf16"] == _lib.SIGNATURES["mvg_msda_backward_bal_f32"]
    assert lib.mvg_msda_backward_bal_workspace.restype is C.c_size_t


UNSUPPORTED = [dict(D=16), dict(D=64), dict(L=3, P=86, shapes=[(8, 8)] * 3),                     # D != 32; L * P = 258 > 256
               dict(M=8, shapes=[(400, 400), (9, 13)]), dict(Lq=1 << 24), dict(N=0)]              # 20 032 bins per image > 12 288


@pytest.mark.parametrize("chunk", [0, 256, 1024, 4096])
def test_workspace_is_zero_exactly_where_dets_is_and_at_least_dets_otherwise(chunk):
    lib = _lib.load()
    for s in (CFG2, SMALL):
        dims, shapes_c = _dims(s)
        det = lib.mvg_msda_backward_det_workspace(*dims, shapes_c)
        bal = lib.mvg_msda_backward_bal_workspace(*dims, shapes_c, chunk)
        assert det > 0 and bal >= det and bal % 256 == 0
        # room for the item table: one (bin, chunk) pair of 8 bytes per possible work item
        N, S, M, D, L, Lq, P = dims
        tiles = sum(((h + 7) // 8) * ((w + 7) // 8) for h, w in s["shapes"])
        if chunk:
            assert bal - det >= 8 * M * (N * tiles + (N * Lq * L * P) // chunk)
    for over in UNSUPPORTED:
        dims, shapes_c = _dims(SMALL, **over)
        assert lib.mvg_msda_backward_det_workspace(*dims, shapes_c) == 0, over
        assert lib.mvg_msda_backward_bal_workspace(*dims, shapes_c, chunk) == 0, over


def test_a_smaller_chunk_needs_no_less_workspace():
    lib = _lib.load()
    dims, shapes_c = _dims(CFG2)
    sizes = [lib.mvg_msda_backward_bal_workspace(*dims, shapes_c, c) for c in (4096, 2048, 1024, 512, 256)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
    assert lib.mvg_msda_backward_bal_workspace(*dims, shapes_c, 0) in sizes            # the default is one of the measured chunks


def test_chunk_zero_is_the_recorded_default():
    """chunk 0 = 2048, the chunk that DESIGN.md section 9h and profiles/r12_bwd_balanced.txt choose: the workspace of chunk 0 is that of
    chunk 2048 and of no other measured chunk (the item table's size is strictly monotonic in the chunk at the cfg-2 shape), and the source's
    constant, its comment's reference and the record say the same number"""
    lib = _lib.load()
    dims, shapes_c = _dims(CFG2)
    size = {c: lib.mvg_msda_backward_bal_workspace(*dims, shapes_c, c) for c in (0, 256, 512, 1024, 2048, 4096)}
    assert size[0] == size[2048]
    assert all(size[c] != size[0] for c in (256, 512, 1024, 4096)), size
    src = open(os.path.join(ROOT, "mvgformer_amd", "csrc", "msda_bwd.hip")).read()
    assert re.search(r"constexpr int BW_CHUNK_DEFAULT = 2048;", src)
    record = open(os.path.join(ROOT, "profiles", "r12_bwd_balanced.txt")).read()
    assert re.search(r"Library default: chunk 2048\b", record)


@pytest.mark.parametrize("chunk", [100, -256, -1, 255, 257, 1000])
def test_illegal_chunks_are_rejected(chunk):
    """no workspace size for them, and MVG_E_BADARG from both entry points before anything is looked at (the pointers here are never
    dereferenced: they are host addresses of a dummy buffer)"""
    lib = _lib.load()
    dims, shapes_c = _dims(SMALL)
    assert lib.mvg_msda_backward_bal_workspace(*dims, shapes_c, chunk) == 0
    dummy = C.create_string_buffer(64)
    p = C.cast(dummy, C.c_void_p)
    starts_c = (C.c_int64 * 2)(0, 540)
    for fn in (lib.mvg_msda_backward_bal_f32, lib.mvg_msda_backward_bal_bf16):
        assert fn(p, shapes_c, starts_c, p, p, p, p, p, p, *dims, p, 1 << 30, None, chunk) == MVG_E_BADARG


def test_ops_knows_the_mode_and_keeps_det_as_the_default():
    from mvgformer_amd import ops
    assert ops.BACKWARD_CHUNK is None
    assert os.environ.get("MVG_BACKWARD") is not None or ops.BACKWARD_MODE == "det"
