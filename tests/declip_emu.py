"""The emulation unit of the clip repair (tests/emu/emu_declip.cpp over csrc/declip_kernel.h), registered with
tests/emu/build.py at run time under the flags of the "deliver" unit, and its call.  Test infrastructure."""
import ctypes

import numpy as np

import emu_build

NAME = "declip"
if NAME not in emu_build.UNITS:
    _deliver = emu_build.UNITS["deliver"]
    emu_build.UNITS[NAME] = type(_deliver)(("emu_declip.cpp",), ("declip_kernel.h", "mgx_hd.h"), _deliver.flags, "EMU_DECLIP_MAIN")

# the order of a channel's words in what k_declip_fold leaves (declip_kernel.h)
SLOTS = ("runs_repaired", "samples_repaired", "samples_raised", "runs_short", "runs_long", "runs_edge", "longest_repaired",
         "peak_before", "peak_after", "first_repaired")
_lib = None


def library():
    global _lib
    if _lib is None:
        lib = emu_build.load(NAME)
        lib.emu_declip_constants.argtypes = [ctypes.c_void_p]
        lib.emu_declip.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_double, ctypes.c_double, ctypes.c_int,
                                   ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        _lib = lib
    return _lib


def constants():
    out = (ctypes.c_longlong * 7)()
    library().emu_declip_constants(out)
    return dict(zip(("segment", "halo", "stretch", "threads", "max_run", "slots", "window"), out))


def declip(frames, level, min_run=2, max_run=32, max_rise=2.0, segment=None, halo=None, stretch=None):
    """(n, 2) float32 through the kernel's phase functions, segment by segment: (out, report) in the oracle's form.  The
    geometry defaults to the kernel's."""
    k = constants()
    assert k["slots"] == len(SLOTS)
    x = np.ascontiguousarray(frames, dtype=np.float32).reshape(-1, 2)
    out = np.full_like(x, -3.0)
    totals = np.zeros((2, len(SLOTS)), dtype=np.int64)
    rc = library().emu_declip(x.ctypes.data, x.shape[0], float(level), float(max_rise), int(min_run), int(max_run),
                              int(segment or k["segment"]), int(halo or k["halo"]), int(stretch or k["stretch"]),
                              out.ctypes.data, totals.ctypes.data)
    assert rc == 0, "the emulation refuses this geometry"
    report = {}
    for j, name in enumerate(SLOTS):
        if name.startswith("peak"):
            report[name] = tuple(float(np.array([v], dtype=np.uint32).view(np.float32)[0]) for v in totals[:, j])
        else:
            report[name] = tuple(int(v) for v in totals[:, j])
    return out, report
