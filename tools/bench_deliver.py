#!/usr/bin/env python
"""What a delivery rendition of a resident track costs, beside the two calls it replaces.

    python tools/bench_deliver.py [--minutes 8] [--rate 44100] [--passes 7] [--out profiles/deliver_8min.json]

The track (tools' usual synthetic programme material) is uploaded once.  Each pass then times, one after the other --
alternating, so that whatever the box does to one it does to the others -- ``mgx_deliver`` at every width and dither and
the yardstick, ``mgx_scale`` followed by ``mgx_pcm_encode`` at the same width (what a caller had to queue for a scaled
integer rendition before: 16 + 12 B/frame at 16 bits against 12), by HIP events on the handle's stream.  Nothing is
downloaded.  Prints one JSON line with the medians and, per variant, the bytes it moves per frame and their fraction of
8 TB/s; ``--out`` also writes it to a file.
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
VARIANTS = [(0, 0), (16, 0), (16, 1), (16, 2), (24, 0), (24, 1), (24, 2), (32, 0)]
DITHER = ("none", "tpdf", "tpdf_hp")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=8.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--out")
    args = ap.parse_args()

    from matchering_amd._native import check, library
    from matchering_amd.device import default_device
    from matchering_amd.synth import make_pair

    frames = int(args.minutes * 60 * args.rate)
    target, _ = make_pair(30.0, args.rate)
    track = np.ascontiguousarray(np.tile(target, (frames // target.shape[0] + 1, 1))[:frames])
    dev, lib = default_device(), library()
    gain = 0.4567
    rows = {}

    with dev.lock:
        buf = dev.upload(track)
        scaled, out = dev.alloc(frames * 8), dev.alloc(frames * 8)
        dev.synchronize()
        x, s, o = (ctypes.c_void_p(b.ptr) for b in (buf, scaled, out))

        def fused(bits, dither):
            check(lib.mgx_deliver(dev.handle, x, 2 * frames, gain, bits, dither, 1, o))

        def pair(bits):
            check(lib.mgx_scale(dev.handle, x, frames, gain, s))
            if bits:
                check(lib.mgx_pcm_encode(dev.handle, s, 2 * frames, bits, o))

        def timed(call, *a):
            dev.timer_start()
            call(*a)
            return dev.timer_stop()

        for bits, dither in VARIANTS:                       # first launches: code and TLB warm
            fused(bits, dither)
        for bits in (0, 16, 24, 32):
            pair(bits)
        dev.synchronize()
        for _ in range(args.passes):
            for bits, dither in VARIANTS:
                rows.setdefault(f"deliver_{bits}_{DITHER[dither]}", []).append(timed(fused, bits, dither))
                if dither == 0:
                    rows.setdefault(f"scale_then_encode_{bits}", []).append(timed(pair, bits))
        for b in (buf, scaled, out):
            b.release()

    def median(values):
        return sorted(values)[len(values) // 2]

    table = {}
    for bits, dither in VARIANTS:
        ms = median(rows[f"deliver_{bits}_{DITHER[dither]}"])
        moved = 8 + (bits // 4 if bits else 8)              # bytes per frame: 8 read, 2 * bits / 8 written
        entry = {"device_us_median": round(ms * 1e3, 1), "bytes_per_frame": moved,
                 "hbm_fraction": round(moved * frames / (ms * 1e-3) / HBM_BYTES_PER_S, 4)}
        if dither == 0:
            yard = median(rows[f"scale_then_encode_{bits}"])
            entry["scale_then_encode_us_median"] = round(yard * 1e3, 1)
            entry["fused_over_pair"] = round(ms / yard, 3)
        table[f"{bits or 'float32'}_{DITHER[dither]}"] = entry
    report = {"track": f"{args.minutes:g} minutes of {args.rate} Hz stereo float32, resident", "frames": frames, "gain": gain,
              "passes": args.passes, "variants": table, "device_ms": {k: [round(v, 4) for v in vs] for k, vs in rows.items()}}
    line = json.dumps(report)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
