#!/usr/bin/env python
"""The audit against the meter on the same resident frames.

    python tools/bench_audit.py [--minutes 8] [--rate 44100] [--repeats 5] [--out profiles/audit_8min.json]

One stereo track of noise of ``--minutes`` is uploaded once as float32 frames and once as the int16 samples of a PCM_16
file; each repeat then times ``mgx_loudness`` on the frames, ``mgx_audit`` on the frames (bits 0) and ``mgx_audit`` on
the int16 samples (bits 16) one after the other, HIP events on the handle's stream around the one call -- launches,
the copy of the result and the wait for it included, as a caller pays them.  The three alternate within the job, so a
drift of the machine's clocks meets all of them; min / median / max over the repeats are reported.  The audit does
less arithmetic per frame than the meter; whether it is faster is recorded here, not asserted: it counts as faster only
where its max lies under the meter's min by more than either's own min-max spread.  Prints one JSON line; ``--out``
also writes it.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(values):
    ordered = sorted(values)
    return {"min": round(ordered[0], 4), "median": round(ordered[len(ordered) // 2], 4), "max": round(ordered[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=8.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.repeats < 3:
        ap.error("at least three repeats")

    from matchering_amd import _native
    from matchering_amd.device import default_device

    dev = default_device()
    frames = int(args.minutes * 60 * args.rate)
    noise = 0.1 * np.random.default_rng(5).standard_normal((frames, 2), dtype=np.float32)
    with dev.lock:
        x = dev.upload(noise)
        pcm = dev.upload(np.round(np.clip(noise, -1.0, 1.0) * 32767.0).astype(np.int16), dtype=None)
        dev.synchronize()
        del noise

        def timed(call):
            dev.timer_start()
            call()
            return dev.timer_stop()

        calls = {"mgx_loudness_ms": lambda: dev.loudness(x, frames, args.rate),
                 "mgx_audit_float32_ms": lambda: dev.audit(x, frames, args.rate, 0),
                 "mgx_audit_int16_ms": lambda: dev.audit(pcm, frames, args.rate, 16)}
        for _ in range(2):                                          # the meter's plan, the scratch, the first launches
            for call in calls.values():
                call()
        rows = {name: [] for name in calls}
        for _ in range(args.repeats):
            for name, call in calls.items():
                rows[name].append(timed(call))
        audited = calls["mgx_audit_float32_ms"]()
        x.release()
        pcm.release()
    dev.trim()
    stats = {name: summary(values) for name, values in rows.items()}
    meter = stats["mgx_loudness_ms"]
    report = {"track": f"{args.minutes:g} minutes of stereo noise at {args.rate} Hz", "frames": frames, "repeats": args.repeats,
              "library": os.path.basename(_native.LIB_PATH), "segments": -(-frames // 4096), "sub_blocks": audited.sub_blocks,
              **stats, "all_ms": {k: [round(v, 4) for v in vs] for k, vs in rows.items()}}
    for name in ("mgx_audit_float32_ms", "mgx_audit_int16_ms"):
        mine = stats[name]
        spread = max(mine["max"] - mine["min"], meter["max"] - meter["min"])
        bytes_read = frames * (8 if "float32" in name else 4)
        report[name.replace("_ms", "")] = {
            "ratio_of_medians_meter_over_audit": round(meter["median"] / mine["median"], 2),
            "spread_ms": round(spread, 4),
            "faster_than_the_meter_beyond_the_spread": bool(meter["min"] - mine["max"] > spread),
            "slower_than_the_meter_beyond_the_spread": bool(mine["min"] - meter["max"] > spread),
            "input_GB_per_s_at_the_median": round(bytes_read / (mine["median"] * 1e-3) / 1e9, 1)}
    line = json.dumps(report)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
