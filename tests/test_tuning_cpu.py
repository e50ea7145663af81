"""The tuning knobs of the library (csrc/tuning.h, the table in csrc/api.hip) through mvg_set_tuning / mvg_tuning_knob, and their
Python side, _lib.TUNING and _lib.tuning().  Host-only entry points: no GPU.  Every test leaves the knobs as it found them (the
suite runs without MVG_TUNE: the values found are the defaults)."""
import ctypes

import pytest

from mvgformer_amd import _lib

BADARG = _lib.DEFINES["MVG_E_BADARG"]
# key -> (default, accepted values other than the default, rejected values next to the rule); in the order of the table
KNOBS = {
    "linear_tiles": (1, [0, 2], [-1, 3]),
    "f32_split": (1, [0], [-1, 2]),
    "f32h_rows": (0, [32, 64], [-1, 1, 31, 33, 63, 65, 128]),
    "chain_rm": (128, [64, 256], [0, 32, 63, 96, 129, 192, 512]),
    "wreg_grid": (512, [1, 64, 2 ** 31 - 1], [0, -1]),
    "bin_multi": (1, [0], [-1, 2]),
    "auto_small": (1, [0], [-1, 2]),
    "gsamp_map": (4, [0, 4096], [-1, 4097]),
    "fwd_map": (1, [0, 2], [-1, 3]),
    "gfused_chunk": (4, [0, 4096], [-1, 4097]),
    "gsamp_pipe": (0, [1, 2], [-1, 3]),
    "chain_a_lds_pad": (0, [1, 120 * 1024], [-1, 120 * 1024 + 1]),
    "gsamp_lds_pad": (0, [1, 120 * 1024], [-1, 120 * 1024 + 1]),
    "gsamp_threads": (256, [128, 512, 1024], [0, 64, 127, 192, 257, 2048]),
}


def _enumerate(lib):
    """[(key, value)] of mvg_tuning_knob, index 0 up to the first refusal"""
    out, key, value = [], ctypes.c_char_p(), ctypes.c_int()
    while lib.mvg_tuning_knob(len(out), ctypes.byref(key), ctypes.byref(value)) == 0:
        out.append((key.value.decode(), value.value))
        assert len(out) < 1000
    return out


def _get(lib, name):
    return dict(_enumerate(lib))[name]


def test_the_knobs_enumerate_with_their_defaults():
    lib = _lib.load()
    assert _enumerate(lib) == [(k, d) for k, (d, _, _) in KNOBS.items()] and len(KNOBS) == 14
    key, value = ctypes.c_char_p(b"untouched"), ctypes.c_int(-5)
    for index in (14, -1, 2 ** 31 - 1, -2 ** 31):
        assert lib.mvg_tuning_knob(index, ctypes.byref(key), ctypes.byref(value)) == BADARG
    assert (key.value, value.value) == (b"untouched", -5)
    assert lib.mvg_tuning_knob(0, None, ctypes.byref(value)) == BADARG and lib.mvg_tuning_knob(0, ctypes.byref(key), None) == BADARG


def test_tuning_dict_equals_the_enumeration():
    lib = _lib.load()
    assert _lib.TUNING == dict(_enumerate(lib)) and list(_lib.TUNING) == list(KNOBS)
    assert all(type(v) is int for v in _lib.TUNING.values())


@pytest.mark.parametrize("name", list(KNOBS))
def test_accepted_values_round_trip_and_rejected_ones_change_nothing(name):
    lib = _lib.load()
    default, accepted, rejected = KNOBS[name]
    before = _enumerate(lib)
    try:
        for v in accepted + [default]:
            assert lib.mvg_set_tuning(name.encode(), v) == 0, v
            assert _get(lib, name) == v == _lib.TUNING[name]
            for bad in rejected:
                assert lib.mvg_set_tuning(name.encode(), bad) == BADARG, bad
                assert _get(lib, name) == v == _lib.TUNING[name], bad
            # only this knob moved
            assert [(k, x) for k, x in _enumerate(lib) if k != name] == [(k, x) for k, x in before if k != name]
    finally:
        assert lib.mvg_set_tuning(name.encode(), dict(before)[name]) == 0
    assert _enumerate(lib) == before


def test_unknown_and_null_keys_change_nothing():
    lib = _lib.load()
    before = _enumerate(lib)
    for key in (b"no_such_knob", b"", b"chain_rm ", b"CHAIN_RM", b"chain", None):
        assert lib.mvg_set_tuning(key, 1) == BADARG, key
    assert _enumerate(lib) == before == list(_lib.TUNING.items())


def test_tuning_context_restores_on_exit_and_when_the_body_raises():
    lib = _lib.load()
    before = _enumerate(lib)
    with _lib.tuning(chain_rm=64):
        assert _get(lib, "chain_rm") == 64 == _lib.TUNING["chain_rm"]
    assert _enumerate(lib) == before == list(_lib.TUNING.items())
    with pytest.raises(ZeroDivisionError):
        with _lib.tuning(chain_rm=64, gsamp_threads=512):
            assert (_get(lib, "chain_rm"), _get(lib, "gsamp_threads")) == (64, 512)
            1 / 0
    assert _enumerate(lib) == before == list(_lib.TUNING.items())
    with _lib.tuning():                                  # no knob: nothing to do
        assert _enumerate(lib) == before


def test_nested_tuning_contexts_restore_in_order():
    lib = _lib.load()
    before = _enumerate(lib)
    with _lib.tuning(chain_rm=64):
        with _lib.tuning(f32_split=0):
            assert (_get(lib, "chain_rm"), _get(lib, "f32_split")) == (64, 0)
            with _lib.tuning(chain_rm=256):
                assert _get(lib, "chain_rm") == 256
            assert (_get(lib, "chain_rm"), _get(lib, "f32_split")) == (64, 0)
        assert (_get(lib, "chain_rm"), _get(lib, "f32_split")) == (64, dict(before)["f32_split"])
        assert _lib.TUNING == dict(_enumerate(lib))
    assert _enumerate(lib) == before == list(_lib.TUNING.items())


def test_tuning_context_refuses_an_unknown_knob_or_value_and_changes_nothing():
    lib = _lib.load()
    before = _enumerate(lib)
    for knobs in (dict(no_such_knob=1), dict(chain_rm=64, no_such_knob=1), dict(gsamp_threads=512, chain_rm=96)):
        with pytest.raises(_lib.MvgError, match="mvg_set_tuning"):
            with _lib.tuning(**knobs):
                raise AssertionError("the body must not run")
        assert _enumerate(lib) == before == list(_lib.TUNING.items()), knobs
