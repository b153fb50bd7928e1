"""Build tests/emu/libmgx_emu_deliver.so (host compiler only; test infrastructure): the emulation of the delivery kernel,
apart from the other emulation libraries so that none rebuilds for another."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(os.path.dirname(HERE)), "matchering_amd", "csrc")
OUT = os.path.join(HERE, "libmgx_emu_deliver.so")
SOURCES = [os.path.join(HERE, "emu_deliver.cpp")]
DEPS = SOURCES + [os.path.join(CSRC, f) for f in ("deliver_kernel.h", "mgx_hd.h")]


def build(force=False):
    newest = max(os.path.getmtime(f) for f in DEPS)
    if not force and os.path.exists(OUT) and os.path.getmtime(OUT) >= newest:
        return OUT
    cxx = os.environ.get("CXX", "g++")
    # -ffp-contract=off as in the library: two products and one sum, each rounded on its own
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-DMGX_HOST_EMU",
                           "-o", OUT] + SOURCES)
    return OUT


if __name__ == "__main__":
    print(build(force=True))
