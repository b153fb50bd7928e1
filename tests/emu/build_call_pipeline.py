"""Build tests/emu/libmgx_emu_call_pipeline.so (host compiler only; test infrastructure): the call pipeline's planner,
csrc/call_pipeline.cpp, behind a C interface.  ``build_driver`` makes the stand-alone program of the same unit, with
whatever extra flags (a sanitizer's) the caller gives."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(os.path.dirname(HERE)), "matchering_amd", "csrc")
OUT = os.path.join(HERE, "libmgx_emu_call_pipeline.so")
DRIVER = os.path.join(HERE, "emu_call_pipeline_driver")
SOURCES = [os.path.join(HERE, "emu_call_pipeline.cpp"), os.path.join(CSRC, "call_pipeline.cpp")]
DEPS = SOURCES + [os.path.join(CSRC, "call_pipeline.h")]


def build(force=False):
    newest = max(os.path.getmtime(f) for f in DEPS)
    if not force and os.path.exists(OUT) and os.path.getmtime(OUT) >= newest:
        return OUT
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-o", OUT] + SOURCES)
    return OUT


def build_driver(out=DRIVER, extra_flags=()):
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-DEMU_CALL_PIPELINE_MAIN", *extra_flags, "-o", out]
                          + SOURCES)
    return out


if __name__ == "__main__":
    print(build(force=True))
