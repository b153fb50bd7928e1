"""Build tests/emu/libmgx_emu_convert_rate.so (host compiler only; test infrastructure): the sample-rate converter's host
plan and the emulation of the deliveries' kernel (csrc/convert_rate_kernel.h), apart from the other emulations so that
none rebuilds for another."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(os.path.dirname(HERE)), "matchering_amd", "csrc")
OUT = os.path.join(HERE, "libmgx_emu_convert_rate.so")
SOURCES = [os.path.join(HERE, "emu_convert_rate.cpp"), os.path.join(CSRC, "resample_plan.cpp")]
DEPS = SOURCES + [os.path.join(CSRC, f) for f in ("resample_plan.h", "resample_kernel.h", "convert_rate_kernel.h", "mgx_hd.h")]


def build(force=False):
    newest = max(os.path.getmtime(f) for f in DEPS)
    if not force and os.path.exists(OUT) and os.path.getmtime(OUT) >= newest:
        return OUT
    cxx = os.environ.get("CXX", "g++")
    # -ffp-contract=off as in the library: the plan's arithmetic is resample.py's, operation by operation
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-DMGX_HOST_EMU",
                           "-o", OUT] + SOURCES)
    return OUT


if __name__ == "__main__":
    print(build(force=True))
