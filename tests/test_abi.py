"""The drop-in boundary without a GPU: libmgx.so loads, exports every function include/mgx.h
declares, its structs have the layout the ctypes mirror assumes (checked against the C compiler's
view of the header), and the entry points that need no device behave.  No compute is called here.
"""

import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT
from matchering_amd import _native

HEADER = os.path.join(ROOT, "include", "mgx.h")


def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return sorted(set(re.findall(r"\b(mgx_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_what_the_binding_binds():
    names = declared_functions()
    assert len(names) >= 25
    assert sorted(_native.SYMBOLS) == names


def test_library_exports_every_declared_symbol():
    lib = ctypes.CDLL(_native.LIB_PATH) if os.path.exists(_native.LIB_PATH) else _native.library()
    for name in declared_functions():
        assert hasattr(lib, name), f"{name} is declared in include/mgx.h but not exported by libmgx.so"


def test_library_exports_nothing_but_the_header(tmp_path):
    """include/mgx.h IS the boundary: libmgx.so exports the declared functions and no other `mgx_*` symbol --
    probes and phase traces are measurement code and live elsewhere (tools/probe/libmgx_probe.so; development
    builds made with -DMGX_TAIL_TRACE / -DMGX_DEV_LIMITER_PHASES beside the product, never as libmgx.so)."""
    _native.library()                                   # (builds the library if it is not there yet)
    listing = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted({ln.split()[-1] for ln in listing.splitlines() if re.match(r".* [TW] mgx_", ln)})
    assert exported == declared_functions()
    assert not [ln for ln in listing.splitlines() if "probe" in ln.lower()]


def test_struct_layouts_match_the_c_compiler(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mgx.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(mgx_config), sizeof(mgx_report),\n'
                   '  offsetof(mgx_config, lowess_delta), offsetof(mgx_config, release_filter_coefficient),\n'
                   '  offsetof(mgx_report, limiter_active)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    c = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert c[0] == ctypes.sizeof(_native.MgxConfig)
    assert c[1] == ctypes.sizeof(_native.MgxReport)
    assert c[2] == _native.MgxConfig.lowess_delta.offset
    assert c[3] == _native.MgxConfig.release_filter_coefficient.offset
    assert c[4] == _native.MgxReport.limiter_active.offset


def test_entry_points_that_need_no_device():
    lib = _native.library()
    assert lib.mgx_version() > 0
    cfg = _native.MgxConfig()
    assert lib.mgx_config_default(ctypes.byref(cfg)) == 0
    assert cfg.internal_sample_rate == 44100 and cfg.fft_size == 4096 and cfg.rms_correction_steps == 4
    assert abs(cfg.threshold - (2 ** 15 - 61) / 2 ** 15) < 1e-15          # defaults.py:64
    n = ctypes.c_int(-1)
    rc = lib.mgx_device_count(ctypes.byref(n))
    if rc == 0 and n.value > 0:
        pytest.skip("a GPU is visible: the no-device behaviour cannot be observed here")
    h = ctypes.c_void_p()
    rc = lib.mgx_create(0, ctypes.byref(h))
    assert rc < 0 and not h.value                      # no CPU path: creation fails, loudly
    assert lib.mgx_last_error()                        # ... with a message


def test_code_sizes_are_read_from_the_librarys_own_code_object():
    """mgx_code_bytes (no GPU needed): the windows the kernels' first workgroups read as data to put their own code
    into the L2 (wave_util.h, warm_code) come from the device ELF inside libmgx.so.  They must be there for the
    instantiations the benchmarks run, and no larger than the symbols llvm-readelf reports: a window that
    reaches past its kernel could reach past the end of the code object."""
    import ctypes
    import re
    import shutil
    import subprocess
    import tempfile

    from matchering_amd import _native

    lib = _native.library()
    sizes = (ctypes.c_int32 * 112)()
    assert lib.mgx_code_bytes(sizes, 112) == 7
    table = [[sizes[c * 16 + v] for v in range(16)] for c in range(7)]
    analyze, match_curve, conv_prep, conv, rnd, tail, limit = table
    assert analyze[12] > 4000 and conv[13] > 20000 and conv[14] > 20000 and conv_prep[13] > 2000
    assert match_curve[0] > 4000 and rnd[0] > 4000 and tail[0] > 4000 and limit[0] > 40000 and limit[1] > 40000
    assert lib.mgx_code_bytes(sizes, 8) < 0                                   # too little room: refused
    objcopy, bundler, readelf = ("/opt/rocm/lib/llvm/bin/" + t for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"))
    if not all(os.path.exists(t) for t in (objcopy, bundler, readelf)):
        pytest.skip("LLVM binary tools not installed")
    folder = tempfile.mkdtemp()
    try:
        fat, dev = os.path.join(folder, "fat.bin"), os.path.join(folder, "dev.co")
        subprocess.check_call([objcopy, "--dump-section", f".hip_fatbin={fat}", _native.LIB_PATH, os.path.join(folder, "x.so")])
        subprocess.check_call([bundler, "--unbundle", "--type=o", f"--input={fat}",
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={dev}"])
        listing = subprocess.run([readelf, "-s", "--wide", dev], capture_output=True, text=True, check=True).stdout
    finally:
        shutil.rmtree(folder, ignore_errors=True)
    seen = {}
    for line in listing.splitlines():
        m = re.match(r"\s*\d+:\s+[0-9a-f]+\s+(\d+)\s+FUNC\s+\S+\s+\S+\s+\S+\s+(\S+)", line)
        if m:
            seen[m.group(2)] = int(m.group(1))
    assert seen["_ZN3mgx6k_convILi13ELb0EEEvNS_9Conv2ArgsE"] == conv[13]
    # the 256-block limiter has four instantiations (the general one and three for fixed window geometries): the table
    # holds the smallest, so that no instantiation's window reaches past its own code
    limiters = [size for name, size in seen.items() if name.startswith("_ZN3mgx7k_limitILi256ELi4E")]
    assert len(limiters) == 4 and min(limiters) == limit[0]
    assert seen["_ZN3mgx9k_analyzeILi12EEEvNS_12AnalysisArgsES1_i"] == analyze[12]
    assert min(seen["_ZN3mgx6k_convILi14ELb0EEEvNS_9Conv2ArgsE"], seen["_ZN3mgx6k_convILi14ELb1EEEvNS_9Conv2ArgsE"]) == conv[14]
    assert seen["_ZN3mgx12k_conv_delayILi14EEEvNS_9Conv2ArgsE"] == conv[15]        # the delay-line kernel's own slot
    assert seen["_ZN3mgx11k_conv_wideILi14EEEvNS_9Conv2ArgsE"] == conv[6]          # N = 4F: the slot no k_conv<L> uses
    assert conv_prep[6] > 2000                                                     # ... and its filter preparation


def test_the_hot_kernels_do_not_spill():
    """(no GPU, no compiler) private_segment_fixed_size of the kernel descriptors inside libmgx.so: the kernels the
    BASELINE workloads spend their time in hold their working set in registers.  VERDICT round 3 asked for this as a
    test after config #5's partitioned convolution was found writing 388 B per lane of spills to memory; the
    delay-line kernel that replaced it (conv_delay_kernel.h) is written around having none."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("code_object", os.path.join(ROOT, "tools", "code_object.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    table = mod.kernels(_native.LIB_PATH)

    def scratch(fragment):
        hits = [v["scratch"] for k, v in table.items() if fragment in k]
        assert len(hits) == 1, (fragment, len(hits))
        return hits[0]

    assert scratch("k_conv_delayILi14E") <= 64                  # config #5: 16384 taps (a dozen dwords around the store phase)
    assert scratch("11k_conv_wideILi14E") == 0                  # the headline workload: 4096 taps on 16384-point blocks
    assert scratch("6k_convILi13ELb0E") == 0                    # ... and on 8192-point blocks (MGX_NO_CONV_WIDE=1)
    assert scratch("k_analyzeILi12E") == 0
    assert scratch("k_analyzeILi14E") <= 16                     # config #5: four dwords around the frames asked for a segment ahead
    assert scratch("k_limitILi256ELi4ELin1E") <= 16             # the general instantiation (two spilled scalars of the look-back)
    assert scratch("k_limitILi256ELi4ELi44ELi43E") == 0         # the headline workload's: 44.1 kHz, 1 ms attack and hold
    assert scratch("k_limitILi256ELi4ELi48ELi47E") == 0         # 48 kHz
    assert scratch("k_limitILi256ELi4ELi96ELi95E") <= 16        # 96 kHz (config #5)
    assert scratch("k_correction_tail") == 0
    # The kernels OFF the BASELINE workloads that do spill, each with the ceiling it has today (VERDICT round 5, next #8:
    # they must not grow silently).  k_conv<14,*>: 8192 taps on 16384-point blocks / the partitioned 32 k and 64 k tap
    # paths (an accumulator row beside the transform); k_analyze_double / _quad: fft_size 32768 / 65536 (two and four
    # transforms' accumulators per thread); k_analyze<10>: the 1024-point radix-32 x 32 plan on 64 threads (a row of 32
    # points, its mirror and 34 accumulators per thread exceed 256 registers); k_limit<1024,1>: attack / hold times whose
    # halos need 1024-block chunks (sixteen waves' scan totals).  Everything else holds its working set in registers.
    ceilings = {"6k_convILi14ELb0E": 72, "6k_convILi14ELb1E": 240, "16k_analyze_doubleILi14E": 340, "14k_analyze_quadILi14E": 128,
                "9k_analyzeILi10E": 64, "7k_limitILi1024ELi1E": 468, "12k_conv_delayILi14E": 64, "9k_analyzeILi14E": 16}
    for name, entry in table.items():
        if entry["scratch"] == 0:
            continue
        hit = [limit for fragment, limit in ceilings.items() if fragment in name]
        assert hit, f"{name} spills {entry['scratch']} B per lane and has no ceiling in this test"
        assert entry["scratch"] <= hit[0], (name, entry["scratch"], hit[0])


def test_the_library_source_holds_no_retired_switches():
    """(no GPU, no compiler) The library's source is the product: an environment switch selects a path a test compares
    the product against (read at mgx_create) or is MGX_LIMIT_TICKETS, and a preprocessor switch builds the CPU emulation,
    a ROCm without the profiler SDK, a fault-injection test build or an instrumentation build for tools/.  A variant that
    was measured and lost lives in git history (docs/HISTORY.md), not behind a switch."""
    csrc = os.path.join(ROOT, "matchering_amd", "csrc")
    code = ""
    for name in sorted(os.listdir(csrc)):
        with open(os.path.join(csrc, name)) as fh:
            code += re.sub(r"//[^\n]*", "", fh.read()) + "\n"
    read = set(re.findall(r'\b(?:getenv|env_flag)\("(MGX_\w+)"\)', code))
    assert read == {"MGX_NO_CONV_DELAY", "MGX_NO_CONV_WIDE", "MGX_FIR_ROUND4", "MGX_NO_TAIL", "MGX_LIMIT_TICKETS"}
    assert len(re.findall(r'\bgetenv\((?!")', code)) == 1          # env_flag's own read; it is called with names only
    assert re.findall(r'\benv_flag\((?!")', code) == ["env_flag("]
    keep = {"MGX_HOST_EMU", "MGX_NO_ROCTX", "MGX_DEV_CONV_PHASES", "MGX_DEV_LIMITER_PHASES", "MGX_TAIL_TRACE"}
    conditions = re.findall(r"^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif)\b([^\n]*)", code, flags=re.M)
    switches = {m for c in conditions for m in re.findall(r"\bMGX_\w+", c)}
    assert switches, "no preprocessor conditions found"
    assert {m for m in switches if m not in keep and not m.startswith("MGX_TEST_")} == set()
