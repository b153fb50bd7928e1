"""The emulation unit of the visuals (tests/emu/emu_visuals.cpp over csrc/visuals_kernel.h), registered with
tests/emu/build.py at run time under the flags of the "deliver" unit, and its calls.  Test infrastructure."""
import ctypes

import numpy as np

import emu_build

NAME = "visuals"
if NAME not in emu_build.UNITS:
    _deliver = emu_build.UNITS["deliver"]
    emu_build.UNITS[NAME] = type(_deliver)(("emu_visuals.cpp",),
                                           ("visuals_kernel.h", "visuals_plan.h", "analysis2_kernel.h", "fft2.h", "mgx_hd.h"),
                                           _deliver.flags, "EMU_VISUALS_MAIN")

_lib = None


def library():
    global _lib
    if _lib is None:
        lib = emu_build.load(NAME)
        lib.emu_spectrogram.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        lib.emu_overview.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        lib.emu_visuals_constants.argtypes = [ctypes.c_void_p]
        _lib = lib
    return _lib


def constants():
    out = (ctypes.c_longlong * 6)()
    library().emu_visuals_constants(out)
    return dict(zip(("run_cap", "share", "threads", "columns_max", "frames_max", "bytes_max"), out))


def spectrogram(x, fft_size, hop, columns, edges, mode=0):
    """(W, 2, B) float32 as the kernels' phase functions compute it on the host."""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, 2)
    edges = np.ascontiguousarray(edges, dtype=np.int32)
    hops = (x.shape[0] - 1) // hop + 1
    width = hops if columns == 0 else columns
    out = np.full((width, 2, edges.size - 1), np.nan, dtype=np.float32)
    rc = library().emu_spectrogram(x.ctypes.data, x.shape[0], int(fft_size).bit_length() - 1, int(hop), int(columns),
                                   int(mode), edges.size - 1, edges.ctypes.data, out.ctypes.data)
    assert rc == 0, rc
    return out


def overview(x, columns):
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, 2)
    minmax = np.zeros((columns, 2, 2), dtype=np.float32)
    sumsq = np.zeros((columns, 2))
    library().emu_overview(x.ctypes.data, x.shape[0], int(columns), minmax.ctypes.data, sumsq.ctypes.data)
    return minmax[:, :, 0], minmax[:, :, 1], sumsq
