"""ctypes binding of libmvgformer_hip.so (the C ABI declared in include/mvg_decoder.h).

There is NO CPU fallback: if the shared library is missing or a call fails, the product
path raises.  torch is used only to own device memory and the current HIP stream.

The header is the one declaration: the argument and return types of every entry point
(SIGNATURES, PROTOTYPES) and the numeric limits and codes (DEFINES) are read from it at
import, so a new entry point is bound by declaring it there.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# MVG_LIB: another build of the same library (measurement variants of tools/ab_*.sh); the product never sets it
LIB_PATH = os.environ.get("MVG_LIB") or os.path.join(_HERE, "libmvgformer_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mvg_decoder.h")


class MvgError(RuntimeError):
    pass


class TensorPtr(C.c_void_p):
    """argtype of every pointer parameter but char*: a torch.Tensor passes its data_ptr() (0 = NULL); None, an int, a c_void_p, a
    ctypes array or byref() go through as for c_void_p"""

    @classmethod
    def from_param(cls, value):
        if isinstance(value, torch.Tensor):
            value = value.data_ptr() or None
        return C.c_void_p.from_param(value)


_SCALARS = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t, "int64_t": C.c_int64, "long": C.c_long,
            "char*": C.c_char_p}


def _ctype(text, decl, pointers=True):
    t = re.sub(r"\bconst\b|\s+", "", text)
    if t in _SCALARS:
        return _SCALARS[t]
    if pointers and re.fullmatch(r"\w+\*+", t):
        return TensorPtr
    raise MvgError("mvg_decoder.h: unknown type %r in %r" % (text.strip(), decl))


def parse_header(text):
    """-> (prototypes: name -> (restype, [(argtype, parameter name), ...]), defines: MVG_* name -> int | float) of the C ABI's
    header.  A statement that is not a prototype of known types, or an MVG_* define that is not a number, raises MvgError."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    defines = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(MVG_\w+)[ \t]+(\S.*?)[ \t]*$", text, flags=re.M):
        try:
            defines[name] = int(value, 0)
        except ValueError:
            try:
                defines[name] = float(value)
            except ValueError:
                raise MvgError("mvg_decoder.h: #define %s %s is not a number" % (name, value)) from None
    text = re.sub(r'^[ \t]*#.*$|extern\s+"C"\s*\{|^[ \t]*\}[ \t]*$', "", text, flags=re.M)
    protos = {}
    for decl in filter(None, (" ".join(d.split()) for d in text.split(";"))):
        m = re.fullmatch(r"(.+?)\b(mvg_\w+) ?\((.*)\)", decl)
        if not m:
            raise MvgError("mvg_decoder.h: cannot read %r" % decl)
        params = []
        for p in ([] if m.group(3).strip() == "void" else m.group(3).split(",")):
            pm = re.fullmatch(r"(.+?)(\w+)", p.strip())
            if not pm:
                raise MvgError("mvg_decoder.h: cannot read parameter %r of %r" % (p.strip(), decl))
            params.append((_ctype(pm.group(1), decl), pm.group(2)))
        protos[m.group(2)] = (_ctype(m.group(1), decl, pointers=False), params)
    return protos, defines


with open(HEADER_PATH) as _f:
    PROTOTYPES, DEFINES = parse_header(_f.read())
# name -> argtypes of EVERY symbol of the header (the restype is PROTOTYPES[name][0])
SIGNATURES = {name: [t for t, _ in params] for name, (_, params) in PROTOTYPES.items()}
# the entry points whose last parameter is the stream (ops._launch appends it)
STREAM_LAST = frozenset(name for name, (_, params) in PROTOTYPES.items() if params and params[-1][1] == "stream")
MVG_F32, MVG_BF16 = DEFINES["MVG_F32"], DEFINES["MVG_BF16"]
CAM_STRIDE = DEFINES["MVG_CAM_STRIDE"]

_lib = None
TUNING = {}     # every knob of the library with its current value, from load() on (mvg_tuning_knob, kept current by mvg_set_tuning)


def load():
    """Load the HIP library (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MvgError(
            "libmvgformer_hip.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C mvgformer_amd/csrc` (there is no CPU fallback for the decoder hot path)" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)   # AttributeError if the symbol is missing
        fn.argtypes = argtypes
        fn.restype = PROTOTYPES[name][0]
    # every knob change goes through this wrapper, so that host-side caches that depend on a knob (DQDecoderLayer's rows of
    # all-masked tiles: computed by the GEMM form that is active) can key on its value: TUNING[key] = the knob's current value
    raw_set = lib.mvg_set_tuning

    def set_tuning(key, value):
        rc = raw_set(key, value)
        if rc == 0:
            TUNING[key.decode() if isinstance(key, bytes) else str(key)] = int(value)
        return rc
    lib.mvg_set_tuning = set_tuning
    key, value, index = C.c_char_p(), C.c_int(), 0
    while lib.mvg_tuning_knob(index, C.byref(key), C.byref(value)) == 0:
        TUNING[key.value.decode()] = value.value
        index += 1
    _lib = lib
    # A/B knobs for measurements: MVG_TUNE="chain_rm=128,gsamp_threads=256"
    for item in filter(None, os.environ.get("MVG_TUNE", "").split(",")):
        k, v = item.split("=")
        check(lib.mvg_set_tuning(k.strip().encode(), int(v)), "mvg_set_tuning(%s)" % item)
    return lib


@contextlib.contextmanager
def tuning(**knobs):
    """Set the given knobs for the body of a `with`; on exit, also when the body raises, every one of them is back at the
    value TUNING held on entry.  A rejected key or value raises MvgError and leaves every knob as it was."""
    lib = load()
    before = {k: TUNING[k] for k in knobs if k in TUNING}
    try:
        for k, v in knobs.items():
            check(lib.mvg_set_tuning(k.encode(), int(v)), "mvg_set_tuning(%s=%s)" % (k, v))
        yield
    finally:
        for k, v in before.items():
            check(lib.mvg_set_tuning(k.encode(), v), "mvg_set_tuning(%s=%s)" % (k, v))


def check(code, what):
    if code != 0:
        raise MvgError("%s failed with code %d" % (what, code))


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def dtype_code(dt):
    if dt == torch.float32:
        return MVG_F32
    if dt == torch.bfloat16:
        return MVG_BF16
    raise MvgError("unsupported dtype %s (float32 / bfloat16 only)" % dt)


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            # same message as the reference's CPU stub (lib/models/ops/src/deform.h:49)
            raise RuntimeError("Not implemented on the CPU")
        if t is not None and t.device.index != torch.cuda.current_device():
            # stream_ptr() hands the kernels the CURRENT device's stream: launching on another device's tensors
            # would run on the wrong GPU.  The module entry points (DQDecoder / DQDecoderLayer / ProjAttn / deformable)
            # switch to their tensors' device themselves; a direct ops.* caller has to.
            raise MvgError("tensor on %s but the current device is cuda:%d -- wrap the call in "
                           "torch.cuda.device(tensor.device)" % (t.device, torch.cuda.current_device()))


def device_info():
    lib = load()
    buf = C.create_string_buffer(64)
    cus = C.c_int(0)
    rc = lib.mvg_device_info(buf, 64, C.byref(cus))
    if rc != 0:
        raise MvgError("no usable AMD GPU (mvg_device_info -> %d)" % rc)
    return buf.value.decode(), cus.value
