"""The emulation unit of the noise-shaped delivery kernel (tests/emu/emu_deliver_shaped.cpp), registered with
tests/emu/build.py at run time under the flags of the "deliver" unit, and its calls.  Test infrastructure."""
import ctypes

import numpy as np

import emu_build

NAME = "deliver_shaped"
if NAME not in emu_build.UNITS:
    _deliver = emu_build.UNITS["deliver"]
    emu_build.UNITS[NAME] = type(_deliver)(
        ("emu_deliver_shaped.cpp",), ("deliver_shaped_kernel.h", "deliver_kernel.h", "mgx_hd.h", "../../include/mgx.h"),
        _deliver.flags, "EMU_DELIVER_SHAPED_MAIN")

_lib = None


def library():
    global _lib
    if _lib is None:
        lib = emu_build.load(NAME)
        lib.emu_deliver_shaped.restype = ctypes.c_longlong
        lib.emu_deliver_shaped.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_double, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_void_p, ctypes.c_ulonglong, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
        lib.emu_deliver_shaped_constants.argtypes = [ctypes.c_void_p]
        _lib = lib
    return _lib


def constants():
    """{B, W, tile (segments of a workgroup), step, threads, lds_bytes, chains} as the kernel's header and include/mgx.h have them."""
    out = (ctypes.c_longlong * 7)()
    library().emu_deliver_shaped_constants(out)
    return dict(zip(("B", "W", "tile", "step", "threads", "lds_bytes", "chains"), out))


def deliver_shaped(x, gain, bits, coefficients, seed, segment=0, warmup=0):
    """The bytes mgx_deliver_shaped's launch writes for (n, 2) float32 frames, run on the CPU."""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, 2)
    c = np.zeros(16)
    c[:len(coefficients)] = coefficients
    out = np.full(x.shape[0] * 2 * (bits // 8), 0xA5, dtype=np.uint8)
    grid = library().emu_deliver_shaped(x.ctypes.data, x.shape[0], float(gain), int(bits), len(coefficients), c.ctypes.data,
                                        int(seed), out.ctypes.data, int(segment), int(warmup))
    assert grid >= 0, "geometry refused"
    return out.tobytes()
