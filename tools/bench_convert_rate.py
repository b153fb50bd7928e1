#!/usr/bin/env python
"""The deliveries' converter against the loader's on the same resident frames.

    python tools/bench_convert_rate.py [--minutes 8] [--repeats 5] [--pairs 192000:44100,...] [--out profiles/convert_rate_8min.json]

For 44.1 -> 48, 44.1 -> 96 and 96 -> 44.1 kHz one stereo track of noise of ``--minutes`` is uploaded once; each repeat
then times ``mgx_resample`` (channels = 2, ``k_resample<2>``) and ``mgx_convert_rate`` (``k_convert_rate<P>``) one after
the other into buffers allocated beforehand, HIP events on the handle's stream around the one call.  The two alternate
within the job, so a drift of the machine's clocks meets both; min / median / max over the repeats are reported, and the
new kernel counts as faster for a pair only where its max lies under the old kernel's min by more than either's own
min-max spread.  The outputs are compared byte for byte once per pair.  Prints one JSON line; ``--out`` also writes it.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAIRS = [(44100, 48000), (44100, 96000), (96000, 44100)]


def summary(values):
    ordered = sorted(values)
    return {"min": round(ordered[0], 4), "median": round(ordered[len(ordered) // 2], 4), "max": round(ordered[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=8.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pairs", help="rate_in:rate_out,... in place of the three pairs above")
    ap.add_argument("--out")
    args = ap.parse_args()
    pairs = PAIRS if not args.pairs else [tuple(int(v) for v in item.split(":")) for item in args.pairs.split(",")]
    if args.repeats < 3:
        ap.error("at least three repeats")

    from matchering_amd import _native
    from matchering_amd.device import default_device
    from matchering_amd.resample import _Plan

    lib = _native.library()
    dev = default_device()
    report = {"track": f"{args.minutes:g} minutes of stereo float32 noise", "repeats": args.repeats,
              "library": os.path.basename(_native.LIB_PATH), "pairs": {}}
    for rate_in, rate_out in pairs:
        frames = int(args.minutes * 60 * rate_in)
        noise = (0.3 * np.random.default_rng(5).standard_normal((frames, 2), dtype=np.float32))
        n_out = ctypes.c_int64()
        _native.check(lib.mgx_convert_rate(None, None, frames, rate_in, rate_out, None, 0, ctypes.byref(n_out)))
        count = n_out.value
        with dev.lock:
            x = dev.upload(noise)
            old_out, new_out = dev.alloc(count * 8), dev.alloc(count * 8)
            dev.synchronize()
            del noise

            def old():
                _native.check(lib.mgx_resample(dev.handle, ctypes.c_void_p(x.ptr), frames, 2, rate_in, rate_out,
                                               ctypes.c_void_p(old_out.ptr), count, ctypes.byref(n_out)))

            def new():
                _native.check(lib.mgx_convert_rate(dev.handle, ctypes.c_void_p(x.ptr), frames, rate_in, rate_out,
                                                   ctypes.c_void_p(new_out.ptr), count, ctypes.byref(n_out)))

            def timed(call):
                dev.timer_start()
                call()
                return dev.timer_stop()

            for _ in range(2):                                     # the plan's design and upload, the first launches
                old()
                new()
            dev.synchronize()
            same = bool(np.array_equal(dev.download(old_out, (count, 2)), dev.download(new_out, (count, 2))))
            rows = {"mgx_resample_ms": [], "mgx_convert_rate_ms": []}
            for _ in range(args.repeats):
                rows["mgx_resample_ms"].append(timed(old))
                rows["mgx_convert_rate_ms"].append(timed(new))
            for b in (x, old_out, new_out):
                b.release()
        dev.trim()
        a, b = summary(rows["mgx_resample_ms"]), summary(rows["mgx_convert_rate_ms"])
        spread = max(a["max"] - a["min"], b["max"] - b["min"])
        width = 2 * _Plan(rate_in, rate_out).taps
        report["pairs"][f"{rate_in}->{rate_out}"] = {
            "frames_in": frames, "frames_out": count, "row_entries": width, "bit_identical": same,
            "mgx_resample_ms": a, "mgx_convert_rate_ms": b,
            "all_ms": {k: [round(v, 4) for v in vs] for k, vs in rows.items()},
            "spread_ms": round(spread, 4), "gain_ms": round(a["min"] - b["max"], 4),
            "faster_beyond_the_spread": bool(a["min"] - b["max"] > spread),
            "ratio_of_medians": round(a["median"] / b["median"], 2),
            "f64_fma": 2 * width * count,
            "convert_rate_f64_fma_per_s": round(2 * width * count / (b["median"] * 1e-3), 0),
        }
    line = json.dumps(report)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
