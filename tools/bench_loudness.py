#!/usr/bin/env python
"""What a loudness measurement of a resident track costs, beside the one call that already streams the same frames.

    python tools/bench_loudness.py [--minutes 8] [--rate 44100] [--passes 7] [--out profiles/loudness_8min.json]
    python tools/bench_loudness.py --kernel-only            (under rocprofv3 --kernel-trace --stats: k_loudness alone)

The track (tools' usual synthetic programme material) is uploaded once.  Each pass then times ``mgx_loudness`` and
``mgx_peak_count`` on the same frames, one after the other -- alternating, so that whatever the box does to one it does
to the other -- by HIP events on the handle's stream (``device_ms``: the launches and the few KB of results coming back)
and by the host's clock around the blocking call (``call_ms``).  ``mgx_peak_count`` is the existing streaming call over
these frames (two reads: the maximum, then the samples on it) and the only yardstick there is for a new capability.
Prints one JSON line with the medians; ``--out`` also writes it to a file.  ``hbm_fraction`` is 8 B/frame over the
median device time against 8 TB/s.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=8.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()

    from matchering_amd.device import default_device
    from matchering_amd.synth import make_pair

    frames = int(args.minutes * 60 * args.rate)
    target, _ = make_pair(30.0, args.rate)
    track = np.ascontiguousarray(np.tile(target, (frames // target.shape[0] + 1, 1))[:frames])
    dev = default_device()
    rows = {"loudness_device_ms": [], "loudness_call_ms": [], "peak_count_device_ms": [], "peak_count_call_ms": []}

    def timed(call):
        dev.timer_start()
        t0 = time.perf_counter()
        out = call()
        wall = (time.perf_counter() - t0) * 1e3
        return out, dev.timer_stop(), wall

    with dev.lock:
        buf = dev.upload(track)
        dev.synchronize()
        value = dev.loudness(buf, frames, args.rate)            # the plan's design and upload, the first launch
        dev.peak_count(buf, 2 * frames)
        if args.kernel_only:
            for _ in range(args.passes):
                dev.loudness(buf, frames, args.rate)
            buf.release()
            print(json.dumps({"loudness": str(value)}))
            return
        for _ in range(args.passes):
            _, device_ms, wall = timed(lambda: dev.loudness(buf, frames, args.rate))
            rows["loudness_device_ms"].append(device_ms)
            rows["loudness_call_ms"].append(wall)
            _, device_ms, wall = timed(lambda: dev.peak_count(buf, 2 * frames))
            rows["peak_count_device_ms"].append(device_ms)
            rows["peak_count_call_ms"].append(wall)
        buf.release()

    def median(values):
        return sorted(values)[len(values) // 2]

    loud, peak = median(rows["loudness_device_ms"]), median(rows["peak_count_device_ms"])
    report = {
        "track": f"{args.minutes:g} minutes of {args.rate} Hz stereo float32, resident", "frames": frames,
        "bytes": 8 * frames, "loudness": str(value),
        **{k: [round(v, 4) for v in vs] for k, vs in rows.items()},
        "loudness_device_us_median": round(loud * 1e3, 1), "peak_count_device_us_median": round(peak * 1e3, 1),
        "loudness_call_us_median": round(median(rows["loudness_call_ms"]) * 1e3, 1),
        "peak_count_call_us_median": round(median(rows["peak_count_call_ms"]) * 1e3, 1),
        "loudness_over_peak_count": round(loud / peak, 2),
        "hbm_fraction": round(8 * frames / (loud * 1e-3) / HBM_BYTES_PER_S, 4),
    }
    line = json.dumps(report)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
