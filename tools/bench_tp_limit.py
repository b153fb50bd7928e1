#!/usr/bin/env python
"""What the deliveries' true-peak limiter costs on a resident track, beside the meter that reads the same frames.

    python tools/bench_tp_limit.py [--minutes 8] [--rate 44100] [--passes 7] [--out profiles/tp_limit_8min.json]

The track (tools' usual synthetic programme material, scaled so that a -1 dBTP ceiling binds) is uploaded once.  Each pass
then times, one after the other -- alternating, so that whatever the box does to one it does to the others --
``mgx_tp_limit`` at the default look-ahead and release (1.5 ms, 50 ms), at the largest look-ahead (2048 frames) and the
yardstick, ``mgx_loudness`` on the same frames, by HIP events on the handle's stream.  ``mgx_tp_limit`` is timed as a
delivery's pass calls it, max_reduction asked for, so both include one wait and one small copy.  Nothing else is
downloaded.  Prints one JSON line with the medians and the limiter's traffic (36 B/frame over its three launches) as a
fraction of 8 TB/s; ``--out`` also writes it to a file.  ``--once``: one call of each variant and no timing -- what a
``rocprofv3 --kernel-trace --stats`` run of its own wraps to split the call by launch.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12
BYTES_PER_FRAME = 36                # envelope 8 + 4, aggregate 4, apply 4 + 8 + 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=8.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()

    from matchering_amd import _native
    from matchering_amd._native import check, library
    from matchering_amd.delivery import LOOKAHEAD_MAX, TruePeakLimiter
    from matchering_amd.device import default_device
    from matchering_amd.synth import make_pair

    frames = int(args.minutes * 60 * args.rate)
    target, _ = make_pair(30.0, args.rate)
    track = np.ascontiguousarray(np.tile(target, (frames // target.shape[0] + 1, 1))[:frames])
    dev, lib = default_device(), library()
    lookahead, release = TruePeakLimiter().frames(args.rate)
    ceiling = 10.0 ** (-1.0 / 20.0)
    variants = {"default": (lookahead, release), "largest_lookahead": (LOOKAHEAD_MAX, release)}
    rows, reductions = {}, {}

    with dev.lock:
        buf = dev.upload(track)
        out = dev.alloc(frames * 8)
        dev.synchronize()
        x, o = ctypes.c_void_p(buf.ptr), ctypes.c_void_p(out.ptr)
        first = dev.loudness(buf, frames, args.rate)
        pre_gain = 2.0 * ceiling / first.true_peak          # 6 dB over the ceiling at the track's highest peak
        worst = ctypes.c_double()

        def limit(name):
            check(lib.mgx_tp_limit(dev.handle, x, frames, pre_gain, ceiling, variants[name][0], variants[name][1], o,
                                   ctypes.byref(worst)))
            reductions[name] = worst.value

        def meter(_):
            report = _native.MgxLoudnessReport()
            check(lib.mgx_loudness(dev.handle, x, frames, args.rate, ctypes.byref(report), None, 0, None))

        def timed(call, name):
            dev.timer_start()
            call(name)
            return dev.timer_stop()

        calls = [("tp_limit_" + name, limit, name) for name in variants] + [("loudness", meter, None)]
        for _, call, name in calls:                          # first launches: code and TLB warm
            call(name)
        dev.synchronize()
        if not args.once:
            for _ in range(args.passes):
                for key, call, name in calls:
                    rows.setdefault(key, []).append(timed(call, name))
        for b in (buf, out):
            b.release()
    if args.once:
        print(json.dumps({"once": True, "frames": frames, "max_reduction": reductions}))
        return

    def median(values):
        return sorted(values)[len(values) // 2]

    yard = median(rows["loudness"])
    table = {"loudness": {"device_us_median": round(yard * 1e3, 1)}}
    for name, (frames_ahead, frames_release) in variants.items():
        ms = median(rows["tp_limit_" + name])
        table["tp_limit_" + name] = {"lookahead": frames_ahead, "release": frames_release, "device_us_median": round(ms * 1e3, 1),
                                     "over_loudness": round(ms / yard, 3), "bytes_per_frame": BYTES_PER_FRAME,
                                     "hbm_fraction": round(BYTES_PER_FRAME * frames / (ms * 1e-3) / HBM_BYTES_PER_S, 4),
                                     "max_reduction": round(reductions[name], 6)}
    report = {"track": f"{args.minutes:g} minutes of {args.rate} Hz stereo float32, resident", "frames": frames,
              "pre_gain": pre_gain, "ceiling": ceiling, "passes": args.passes, "variants": table,
              "device_ms": {k: [round(v, 4) for v in vs] for k, vs in rows.items()}}
    line = json.dumps(report)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
