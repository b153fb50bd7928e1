"""The stand-alone programs of the delivery and true-peak limiter emulations (tests/emu/emu_deliver.cpp, emu_tp_limit.cpp)
under the sanitizers, without a GPU: the kernels' own phase functions over exactly sized buffers, at ragged sizes and the
extreme look-aheads, where an index off by one is AddressSanitizer's to find.
"""

import subprocess

import pytest

import emu_build


@pytest.mark.parametrize("unit", ["deliver", "tp_limit"])
def test_standalone_emulation_under_sanitizers(tmp_path, unit):
    """Built with AddressSanitizer and UBSan, run once (nothing loaded into Python runs under a sanitizer): ``ok`` and
    exit status 0."""
    out = str(tmp_path / f"emu_{unit}_driver")
    emu_build.build_driver(unit, out, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    done = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout + done.stderr
    assert done.stdout.strip() == "ok", done.stdout + done.stderr
