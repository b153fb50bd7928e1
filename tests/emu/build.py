"""Build the host emulations of tests/emu (host compiler only; test infrastructure), one shared library per unit so that
none rebuilds for another, and the stand-alone programs of the units that have one."""
import ctypes
import os
import subprocess
import sys
from collections import namedtuple

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "matchering_amd", "csrc")
ALL_HEADERS = sorted(f for f in os.listdir(CSRC) if f.endswith(".h")) + ["../../include/mgx.h"]
# -ffp-contract=off as in the library: a product and a sum are rounded each on its own unless the code says fma
EMU = ("-ffp-contract=off", "-DMGX_HOST_EMU")

# sources and headers by file name: emu*.cpp lie here, everything else in matchering_amd/csrc.  `main`: the macro that
# turns the unit's stand-alone program on, None where it has none, "" where the unit is nothing but a program.
Unit = namedtuple("Unit", "sources headers flags main")
UNITS = {
    # the kernels' phase functions of the master path and the host FIR design -> libmgx_emu.so
    "kernels": Unit(("emu.cpp", "fir_design.cpp", "fir_plan.cpp"), ALL_HEADERS, EMU, None),
    # the sample-rate converter's host plan and the emulation of its kernel
    "resample": Unit(("emu_resample.cpp", "resample_plan.cpp"), ("resample_plan.h", "resample_kernel.h", "mgx_hd.h"), EMU, None),
    # ... and of the deliveries' kernel (csrc/convert_rate_kernel.h)
    "convert_rate": Unit(("emu_convert_rate.cpp", "resample_plan.cpp"),
                         ("resample_plan.h", "resample_kernel.h", "convert_rate_kernel.h", "mgx_hd.h"), EMU, None),
    "loudness": Unit(("emu_loudness.cpp", "loudness_plan.cpp"), ("loudness_plan.h", "loudness_kernel.h", "mgx_hd.h"), EMU, None),
    "deliver": Unit(("emu_deliver.cpp",), ("deliver_kernel.h", "mgx_hd.h"), EMU, "EMU_DELIVER_MAIN"),
    "tp_limit": Unit(("emu_tp_limit.cpp", "loudness_plan.cpp"), ("tp_limit_kernel.h", "loudness_plan.h", "mgx_hd.h"), EMU,
                     "EMU_TP_LIMIT_MAIN"),
    # the call pipeline's planner, csrc/call_pipeline.cpp, behind a C interface
    "call_pipeline": Unit(("emu_call_pipeline.cpp", "call_pipeline.cpp"), ("call_pipeline.h",), ("-Wall",), "EMU_CALL_PIPELINE_MAIN"),
    # the library's device-free unit (csrc/mgx_policy.cpp) with its driver: mgx_design_fir brings in the host FIR design,
    # the loudness gate and the delivery head-room loudness_plan.cpp, the converters' request resample_plan.cpp
    "policy": Unit(("emu_policy_driver.cpp", "mgx_policy.cpp", "loudness_plan.cpp", "fir_design.cpp", "fir_plan.cpp",
                    "resample_plan.cpp"), ALL_HEADERS, EMU, ""),
}


LIBRARIES = [name for name, unit in UNITS.items() if unit.main != ""]


def _paths(names):
    return [os.path.join(HERE if os.path.basename(f).startswith("emu") else CSRC, f) for f in names]


def library_path(name="kernels"):
    return os.path.join(HERE, "libmgx_emu.so" if name == "kernels" else f"libmgx_emu_{name}.so")


def build(name="kernels", force=False):
    """The unit's shared library, compiled when a source or header is newer than it.  Returns its path."""
    unit, out = UNITS[name], library_path(name)
    assert unit.main != "", f"{name} is a program: build_driver"
    sources = _paths(unit.sources)
    newest = max(os.path.getmtime(f) for f in sources + _paths(unit.headers))
    if not force and os.path.exists(out) and os.path.getmtime(out) >= newest:
        return out
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-shared", "-fPIC", *unit.flags, "-o", out] + sources)
    return out


def build_driver(name, out, extra_flags=()):
    """The unit's stand-alone program at `out`, with whatever extra flags (a sanitizer's) the caller gives."""
    unit = UNITS[name]
    assert unit.main is not None, f"{name} has no stand-alone program"
    cxx = os.environ.get("CXX", "g++")
    main = [f"-D{unit.main}"] if unit.main else []
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", *unit.flags, *main, *extra_flags, "-o", out]
                          + _paths(unit.sources))
    return out


def load(name="kernels"):
    """The ``ctypes.CDLL`` of a unit's library, built first where it is out of date."""
    return ctypes.CDLL(build(name))


if __name__ == "__main__":
    for unit in sys.argv[1:] or LIBRARIES:
        print(build(unit, force=True))
