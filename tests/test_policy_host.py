"""The library's device-free unit (csrc/mgx_policy.cpp) in a program of its own, without a GPU.

Config validation, the delivery gain rule, the limiter's pass planner, loudness gating, the host FIR design's entry
point and what the device entry points settle from their numbers alone are arithmetic on the structs of include/mgx.h;
tests/test_delivery_host.py, test_tp_limiter_host.py, test_loudness_host.py, test_resample_plan.py and
test_convert_rate_host.py check their values through libmgx.so.  Here the same unit is linked into a stand-alone driver
(tests/emu/emu_policy_driver.cpp) that walks the edges those tests name, so that it can run under the sanitizers.
"""

import re
import subprocess

import emu_build

GROUPS = ["check_config", "mgx_delivery_gain", "mgx_delivery_limit_step", "mgx_loudness_gate", "mgx_design_fir",
          "resample_request", "stage_checks"]


def test_standalone_driver_under_sanitizers(tmp_path):
    """Built with AddressSanitizer and UBSan, run once (nothing loaded into Python runs under a sanitizer): one line per
    group, every stated value met, exit status 0."""
    out = str(tmp_path / "driver")
    emu_build.build_driver("policy", out, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    done = subprocess.run([out], capture_output=True, text=True, timeout=60)
    assert done.returncode == 0, done.stdout + done.stderr
    lines = done.stdout.splitlines()
    assert len(lines) == len(GROUPS), done.stdout
    for line, group in zip(lines, GROUPS):
        m = re.fullmatch(r"(\w+): (\d+) checks, 0 wrong", line)
        assert m and m.group(1) == group and int(m.group(2)) >= 10, line
