#!/usr/bin/env python
"""What a noise-shaped delivery of a resident track costs, beside the TPDF delivery of the same width.

    python tools/bench_deliver_shaped.py [--minutes 8] [--rate 44100] [--passes 7] [--out profiles/deliver_shaped_8min.json]
                                         [--other-lib PATH --other-label 512/64]

The track (tools' usual synthetic programme material) is uploaded once.  Each pass then times, one after the other --
alternating, so that whatever the box does to one it does to the others -- ``mgx_deliver_shaped`` with both presets at 16
and 24 bits and the yardstick, ``mgx_deliver`` at dither 1 and the same width, by HIP events on the handle's stream.
Nothing is downloaded.  ``--other-lib``: a second build of the library (another MGX_SHAPER_SEGMENT / MGX_SHAPER_WARMUP in
include/mgx.h) whose ``mgx_deliver_shaped`` is timed in the same passes on a handle of its own, for the choice of the
segment length.  Prints one JSON line with the medians, the ratios to the yardstick and every
time; ``--out`` also writes it to a file.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PRESETS = {"lipshitz5": 1, "wannamaker9": 2}
WIDTHS = (16, 24)


def median(values):
    return sorted(values)[len(values) // 2]


class OtherBuild:
    """A second libmgx.so in this process: a handle of its own on the same device, timed by its own events."""

    def __init__(self, path, symbols):
        self.lib = ctypes.CDLL(path)
        for name in ("mgx_create", "mgx_destroy", "mgx_deliver_shaped", "mgx_timer_start", "mgx_timer_stop", "mgx_synchronize",
                     "mgx_last_error"):
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = symbols[name]
        self.handle = ctypes.c_void_p()
        self.check(self.lib.mgx_create(0, ctypes.byref(self.handle)))

    def check(self, code):
        if code != 0:
            raise RuntimeError(f"{code}: {self.lib.mgx_last_error().decode()}")

    def timed(self, x, frames, gain, bits, shaper, out):
        self.check(self.lib.mgx_timer_start(self.handle))
        self.check(self.lib.mgx_deliver_shaped(self.handle, x, frames, gain, bits, ctypes.byref(shaper), 1, out))
        ms = ctypes.c_float()
        self.check(self.lib.mgx_timer_stop(self.handle, ctypes.byref(ms)))
        return ms.value

    def close(self):
        self.check(self.lib.mgx_destroy(self.handle))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=8.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--other-lib")
    ap.add_argument("--other-label", default="other")
    ap.add_argument("--out")
    args = ap.parse_args()

    from matchering_amd import _native
    from matchering_amd._native import check, library
    from matchering_amd.device import default_device
    from matchering_amd.synth import make_pair

    frames = int(args.minutes * 60 * args.rate)
    target, _ = make_pair(30.0, args.rate)
    track = np.ascontiguousarray(np.tile(target, (frames // target.shape[0] + 1, 1))[:frames])
    dev, lib = default_device(), library()
    gain = 0.4567
    shapers = {}
    for name, identifier in PRESETS.items():
        shapers[name] = _native.MgxNoiseShaper()
        check(lib.mgx_noise_shaper_preset(identifier, 44100, ctypes.byref(shapers[name])))
    label = f"{_native.SHAPER_SEGMENT}/{_native.SHAPER_WARMUP}"
    rows = {}

    with dev.lock:
        buf, out = dev.upload(track), dev.alloc(frames * 8)
        dev.synchronize()
        x, o = ctypes.c_void_p(buf.ptr), ctypes.c_void_p(out.ptr)
        other = OtherBuild(args.other_lib, _native.SYMBOLS) if args.other_lib else None

        def shaped(bits, name):
            check(lib.mgx_deliver_shaped(dev.handle, x, frames, gain, bits, ctypes.byref(shapers[name]), 1, o))

        def plain(bits):
            check(lib.mgx_deliver(dev.handle, x, 2 * frames, gain, bits, 1, 1, o))

        def timed(call, *a):
            dev.timer_start()
            call(*a)
            return dev.timer_stop()

        for bits in WIDTHS:                                 # first launches: code and TLB warm
            plain(bits)
            for name in PRESETS:
                shaped(bits, name)
                if other:
                    other.timed(x, frames, gain, bits, shapers[name], o)
        dev.synchronize()
        for _ in range(args.passes):
            for bits in WIDTHS:
                rows.setdefault(f"deliver_{bits}_tpdf", []).append(timed(plain, bits))
                for name in PRESETS:
                    rows.setdefault(f"shaped_{bits}_{name}", []).append(timed(shaped, bits, name))
                    if other:
                        rows.setdefault(f"shaped_{bits}_{name}@{args.other_label}", []).append(
                            other.timed(x, frames, gain, bits, shapers[name], o))
        if other:
            other.close()
        for b in (buf, out):
            b.release()

    table = {}
    for bits in WIDTHS:
        yard = median(rows[f"deliver_{bits}_tpdf"])
        table[f"{bits}_tpdf"] = {"device_us_median": round(yard * 1e3, 1)}
        for name in PRESETS:
            ms = median(rows[f"shaped_{bits}_{name}"])
            entry = {"device_us_median": round(ms * 1e3, 1), "over_tpdf": round(ms / yard, 3),
                     "spread_us": round((max(rows[f"shaped_{bits}_{name}"]) - min(rows[f"shaped_{bits}_{name}"])) * 1e3, 1)}
            if args.other_lib:
                theirs = rows[f"shaped_{bits}_{name}@{args.other_label}"]
                entry[f"device_us_median@{args.other_label}"] = round(median(theirs) * 1e3, 1)
                entry[f"spread_us@{args.other_label}"] = round((max(theirs) - min(theirs)) * 1e3, 1)
            table[f"{bits}_{name}"] = entry
    report = {"track": f"{args.minutes:g} minutes of {args.rate} Hz stereo float32, resident", "frames": frames, "gain": gain,
              "passes": args.passes, "segment/warmup": label, "variants": table,
              "device_ms": {k: [round(v, 4) for v in vs] for k, vs in rows.items()}}
    line = json.dumps(report)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
