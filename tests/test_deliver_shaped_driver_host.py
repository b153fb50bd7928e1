"""The stand-alone program of the noise-shaped delivery's emulation (tests/emu/emu_deliver_shaped.cpp) under the
sanitizers, without a GPU: the kernel's own phase functions over exactly sized buffers at the sizes around a warm-up, a
segment and a workgroup's tile, where an index off by one is AddressSanitizer's to find.
"""

import subprocess

import deliver_shaped_emu
import emu_build


def test_standalone_emulation_under_sanitizers(tmp_path):
    """Built with AddressSanitizer and UBSan, run once (nothing loaded into Python runs under a sanitizer): ``ok`` and
    exit status 0."""
    out = str(tmp_path / "emu_deliver_shaped_driver")
    emu_build.build_driver(deliver_shaped_emu.NAME, out, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    done = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout + done.stderr
    assert done.stdout.strip() == "ok", done.stdout + done.stderr
