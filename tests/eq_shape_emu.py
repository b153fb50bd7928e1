"""The emulation unit of the matching EQ's device stages (tests/emu/emu_eq_shape.cpp), registered with tests/emu/build.py
at run time under the flags and sources of the "policy" unit -- its stand-alone program calls mgx_shape_fir, which lives
in csrc/mgx_policy.cpp -- and its calls.  Test infrastructure."""
import ctypes

import numpy as np

import emu_build

NAME = "eq_shape"
if NAME not in emu_build.UNITS:
    _policy = emu_build.UNITS["policy"]
    emu_build.UNITS[NAME] = type(_policy)(
        ("emu_eq_shape.cpp",) + tuple(s for s in _policy.sources if not s.startswith("emu")), _policy.headers, _policy.flags,
        "EMU_EQ_SHAPE_MAIN")

_lib = None


def library():
    global _lib
    if _lib is None:
        lib = emu_build.load(NAME)
        lib.emu_eq_shape.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                     ctypes.c_double]
        lib.emu_eq_shape.restype = None
        lib.emu_eq_geometry.argtypes = [ctypes.c_int, ctypes.c_void_p]
        lib.emu_eq_geometry.restype = None
        lib.emu_eq_minphase.argtypes = [ctypes.c_void_p, ctypes.c_int]
        lib.emu_eq_minphase.restype = ctypes.c_int
        _lib = lib
    return _lib


def geometry(fft):
    """{log2m, r, threads, lds_bytes, work_bytes} of the minimum-phase chain at ``fft`` taps, as the kernels' header has them."""
    out = (ctypes.c_longlong * 5)()
    library().emu_eq_geometry(int(fft), out)
    return dict(zip(("log2m", "r", "threads", "lds_bytes", "work_bytes"), out))


def shape_curve(smooth, min_value, amount=1.0, max_boost_db=None, max_cut_db=None):
    """k_eq_shape on one smooth plane, run on the CPU."""
    nan = float("nan")
    out = np.array(smooth, dtype=np.float64)
    library().emu_eq_shape(out.ctypes.data, out.shape[0], float(amount), nan if max_boost_db is None else float(max_boost_db),
                           nan if max_cut_db is None else float(max_cut_db), float(min_value))
    return out


def minimum_phase(taps):
    """The eight launches of the minimum-phase chain on [2][F] float32 taps, run on the CPU: (taps, R)."""
    out = np.array(taps, dtype=np.float32).reshape(2, -1)
    r = library().emu_eq_minphase(out.ctypes.data, out.shape[1])
    assert r >= 1, "size refused"
    return out, r
