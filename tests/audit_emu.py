"""The emulation unit of the audit's run monoid (tests/emu/emu_audit.cpp over csrc/audit_kernel.h), registered with
tests/emu/build.py at run time under the flags of the "deliver" unit, and its calls.  Test infrastructure."""
import ctypes

import numpy as np

import emu_build

NAME = "audit"
if NAME not in emu_build.UNITS:
    _deliver = emu_build.UNITS["deliver"]
    emu_build.UNITS[NAME] = type(_deliver)(("emu_audit.cpp",), ("audit_kernel.h", "mgx_hd.h"), _deliver.flags, "EMU_AUDIT_MAIN")

FIELDS = ("start", "len", "prefix", "suffix", "best", "best_at", "events", "samples", "first")
_lib = None


def library():
    global _lib
    if _lib is None:
        lib = emu_build.load(NAME)
        int_p = ctypes.POINTER(ctypes.c_int)
        lib.emu_audit_leaf.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, int_p]
        lib.emu_audit_combine.argtypes = [int_p, int_p, ctypes.c_int, int_p]
        lib.emu_audit_finish.argtypes = [int_p, ctypes.c_int, int_p]
        lib.emu_audit_constants.argtypes = [ctypes.c_void_p]
        assert lib.emu_audit_run_ints() == len(FIELDS)
        _lib = lib
    return _lib


def constants():
    out = (ctypes.c_longlong * 5)()
    library().emu_audit_constants(out)
    return dict(zip(("segment", "threads", "run", "subs_max", "merge_threads"), out))


def _record():
    return (ctypes.c_int * len(FIELDS))()


def leaf(predicate, start, min_run):
    """The record of a stretch of the predicate that begins at frame ``start``."""
    p = np.ascontiguousarray(predicate, dtype=np.uint8)
    out = _record()
    library().emu_audit_leaf(p.ctypes.data, int(start), int(p.size), int(min_run), out)
    return out


def combine(a, b, min_run):
    out = _record()
    library().emu_audit_combine(a, b, int(min_run), out)
    return out


def finish(total, min_run):
    out = _record()
    library().emu_audit_finish(total, int(min_run), out)
    return dict(zip(FIELDS, out))


def fields(record):
    return dict(zip(FIELDS, record))
