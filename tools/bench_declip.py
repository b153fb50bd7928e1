#!/usr/bin/env python
"""The clip repair against a plain stream of the same traffic, and against the audit, on the same resident frames.

    python tools/bench_declip.py [--minutes 8] [--rate 44100] [--repeats 5] [--out profiles/declip_8min.json]

One stereo track of ``--minutes`` -- five tones under a little noise, peak 1 -- is uploaded three times: at half its
level (peak under the repair's level of 0.7: every segment is a copy), hard-clipped at 0.7 (runs to rebuild in every
segment) and with every sample at the rail (two runs as long as the track, `long`).  Each repeat times, one after the other, a blocking ``mgx_declip`` on each of the three, ``mgx_scale`` on the clean
buffer followed by a wait -- 8 bytes read and 8 written per frame, the plain-stream yardstick for the repair's traffic --
and ``mgx_audit`` on the clean buffer; HIP events on the handle's stream around the one call, launches, the copy of the
report and the wait for it included, as a caller pays them.  The five alternate within the job, so a drift of the
machine's clocks meets all of them; min / median / max over the repeats are reported.  Nothing is asserted.  Prints one
JSON line; ``--out`` also writes it.
"""
import argparse
import ctypes
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
    from matchering_amd.device import check, default_device, library
    from matchering_amd.repair import ClipRepair, from_report

    dev = default_device()
    frames = int(args.minutes * 60 * args.rate)
    # five tones (as tests/test_declip_host.py's) under a little noise, peak 1: clipped at 0.7 it holds runs to rebuild
    t = np.arange(frames, dtype=np.float64) / args.rate
    rng = np.random.default_rng(5)
    tones = sum(a * np.sin(2 * np.pi * f * t + p) for f, a, p in zip((110, 331, 523, 1480, 3100), (1, .6, .4, .3, .2), rng.uniform(0, 6, 5)))
    noise = np.stack([tones, tones[::-1]], axis=1) + 0.01 * rng.standard_normal((frames, 2))
    noise = (noise / np.max(np.abs(noise))).astype(np.float32)
    del t, tones
    level = float(np.float32(0.7))                              # (a float32: the clipped samples sit ON the level)
    rail = np.empty_like(noise)
    rail[:, 0], rail[:, 1] = level, -level
    with dev.lock:
        tracks = {"clean": dev.upload(0.5 * noise), "clipped": dev.upload(np.clip(noise, -level, level)), "rail": dev.upload(rail)}
        del rail
        out = dev.alloc(frames * 8)
        dev.synchronize()
        del noise
        repair = ClipRepair(level=level)
        params, found = repair.native(), {}

        def declip(name):
            report = _native.MgxDeclipReport()
            check(library().mgx_declip(dev.handle, ctypes.c_void_p(tracks[name].ptr), frames, ctypes.byref(params),
                                       ctypes.c_void_p(out.ptr), ctypes.byref(report)))
            found[name] = report

        def scale():
            check(library().mgx_scale(dev.handle, ctypes.c_void_p(tracks["clean"].ptr), frames, 0.5, ctypes.c_void_p(out.ptr)))
            dev.synchronize()

        def timed(call):
            dev.timer_start()
            call()
            return dev.timer_stop()

        calls = {"mgx_declip_clean_ms": lambda: declip("clean"), "mgx_declip_clipped_ms": lambda: declip("clipped"),
                 "mgx_declip_rail_ms": lambda: declip("rail"), "mgx_scale_ms": scale,
                 "mgx_audit_ms": lambda: dev.audit(tracks["clean"], frames, args.rate, 0)}
        for _ in range(2):                                          # the scratch, the first launches
            for call in calls.values():
                call()
        rows = {name: [] for name in calls}
        for _ in range(args.repeats):
            for name, call in calls.items():
                rows[name].append(timed(call))
        for buf in (*tracks.values(), out):
            buf.release()
    dev.trim()
    stats = {name: summary(values) for name, values in rows.items()}
    plain = stats["mgx_scale_ms"]
    report = {"track": f"{args.minutes:g} minutes of five tones under noise at {args.rate} Hz", "frames": frames, "repeats": args.repeats,
              "library": os.path.basename(_native.LIB_PATH), "segments": -(-frames // 4096), "level_of_peak": 0.7,
              **stats, "all_ms": {k: [round(v, 4) for v in vs] for k, vs in rows.items()}}
    for name in ("clean", "clipped", "rail"):
        mine = stats[f"mgx_declip_{name}_ms"]
        did = from_report(found[name], level, frames)
        report["mgx_declip_" + name] = {
            "ratio_of_medians_over_mgx_scale": round(mine["median"] / plain["median"], 2),
            "ratio_of_medians_over_mgx_audit": round(mine["median"] / stats["mgx_audit_ms"]["median"], 2),
            "ranges_overlap_mgx_scale": bool(mine["min"] <= plain["max"] and plain["min"] <= mine["max"]),
            "GB_per_s_read_and_written_at_the_median": round(frames * 16 / (mine["median"] * 1e-3) / 1e9, 1),
            "runs_repaired": sum(did.runs_repaired), "samples_raised": sum(did.samples_raised), "runs_long": sum(did.runs_long)}
    line = json.dumps(report)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
