"""The emulation unit of the matching EQ's tone stage (tests/emu/emu_eq_tone.cpp), registered with tests/emu/build.py at
run time under the flags and sources of the "policy" unit -- its stand-alone program calls mgx_eq_tone_check,
mgx_eq_tone_curve and mgx_tone_fir, which live in csrc/mgx_policy.cpp -- and its calls.  Also what the tone tests share:
the structs of a shape and of an oracle tone (tests/eq_tone_oracle.py).  Test infrastructure."""
import ctypes

import numpy as np

import emu_build

NAME = "eq_tone"
if NAME not in emu_build.UNITS:
    _policy = emu_build.UNITS["policy"]
    emu_build.UNITS[NAME] = type(_policy)(
        ("emu_eq_tone.cpp",) + tuple(s for s in _policy.sources if not s.startswith("emu")), _policy.headers, _policy.flags,
        "EMU_EQ_TONE_MAIN")

NAN = float("nan")
_lib = None


def shape_struct(amount=1.0, max_boost_db=None, max_cut_db=None, phase="linear", reserved=0):
    from matchering_amd._native import MgxEqShape

    return MgxEqShape(amount, NAN if max_boost_db is None else max_boost_db, NAN if max_cut_db is None else max_cut_db,
                      {"linear": 0, "minimum": 1}.get(phase, phase), reserved)


def tone_struct(tone, band_count=None, reserved=0):
    """The mgx_eq_tone of an oracle tone (a dict of tests/eq_tone_oracle.py)."""
    from matchering_amd._native import MgxEqBand, MgxEqTone

    def value(v):
        return NAN if v is None else v

    out = MgxEqTone(value(tone["low_hz"]), value(tone["high_hz"]), tone["range_octaves"], value(tone["side_amount"]),
                    value(tone["mono_below_hz"]), tone["mono_octaves"], tone["tilt_db_per_octave"], tone["tilt_pivot_hz"],
                    len(tone["bands"]) if band_count is None else band_count, reserved)
    for i, band in enumerate(tone["bands"]):
        out.bands[i] = MgxEqBand(*band)
    return out


def library():
    global _lib
    if _lib is None:
        lib = emu_build.load(NAME)
        lib.emu_eq_tone.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_void_p,
                                    ctypes.c_void_p]
        lib.emu_eq_tone.restype = None
        lib.emu_eq_tone_sizeof.restype = ctypes.c_int
        _lib = lib
    return _lib


def tone_planes(planes, fs, min_value, tone, shape=None):
    """k_eq_tone on the two smooth planes [2][F/2 + 1], run on the CPU.  ``shape``: an MgxEqShape or None."""
    out = np.array(planes, dtype=np.float64)
    assert out.ndim == 2 and out.shape[0] == 2
    struct = tone_struct(tone)
    library().emu_eq_tone(out.ctypes.data, 2 * (out.shape[1] - 1), float(fs), float(min_value),
                          None if shape is None else ctypes.addressof(shape), ctypes.addressof(struct))
    return out
