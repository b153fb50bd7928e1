"""Build tests/emu/libmgx_emu_tp_limit.so (host compiler only; test infrastructure): the emulation of the deliveries'
true-peak limiter, apart from the other emulation libraries so that none rebuilds for another."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(os.path.dirname(HERE)), "matchering_amd", "csrc")
OUT = os.path.join(HERE, "libmgx_emu_tp_limit.so")
SOURCES = [os.path.join(HERE, "emu_tp_limit.cpp"), os.path.join(CSRC, "loudness_plan.cpp")]
DEPS = SOURCES + [os.path.join(CSRC, f) for f in ("tp_limit_kernel.h", "loudness_plan.h", "mgx_hd.h")]


def build(force=False):
    newest = max(os.path.getmtime(f) for f in DEPS)
    if not force and os.path.exists(OUT) and os.path.getmtime(OUT) >= newest:
        return OUT
    cxx = os.environ.get("CXX", "g++")
    # -ffp-contract=off as in the library: a product and a sum are rounded each on its own unless the code says fma
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-DMGX_HOST_EMU",
                           "-o", OUT] + SOURCES)
    return OUT


if __name__ == "__main__":
    print(build(force=True))
