#!/usr/bin/env python
"""What it costs to bring an off-rate file to the internal rate: the host route against the device route.

    python tools/bench_resample.py [--minutes 8] [--rate 48000] [--repeats 3] [--out profiles/resample_DATE.json]
    python tools/bench_resample.py --kernel-only          (under rocprofv3 --kernel-trace --stats)

One 16-bit stereo WAVE file of noise at ``--rate`` is written to a temporary folder.  Each repeat then times, one
after the other,
  (i)   the host route:   audio_io.load + checker.check (float64 resampler, one host thread) + upload, to synchronisation;
  (ii)  the device route: audio_io.load + Device.track_frames (upload as the file holds it, mgx_pcm_decode,
        mgx_resample) + mgx_peak_count + checker.check(on_device=True), to synchronisation;
  (iii) the kernel alone: mgx_resample on the decoded frames, HIP events on the handle's stream (best of 5).
Prints one JSON line; ``--out`` also writes it to a file.  The kernel's bytes/s and float64 FMA/s are given against
what the conversion must move and compute at least: 8 n bytes in, 8 n_out bytes out, 2 W n_out FMAs.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=8.0)
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()

    import matchering_amd as mg
    from matchering_amd import audio_io, checker
    from matchering_amd.device import default_device, takes_resident
    from matchering_amd.resample import _Plan

    config = mg.Config()
    internal = config.internal_sample_rate
    frames = int(args.minutes * 60 * args.rate)
    dev = default_device()
    rows = {"host_route_s": [], "device_route_s": [], "kernel_ms": []}
    with tempfile.TemporaryDirectory() as folder:
        path = os.path.join(folder, "off_rate.wav")
        noise = np.random.default_rng(5).integers(-12000, 12000, size=(frames, 2), dtype=np.int16)
        audio_io.write_wav(path, noise, args.rate, "PCM_16")
        del noise

        def host_route():
            t0 = time.perf_counter()
            audio, rate = audio_io.load(path, "target", folder, pcm=True)
            array, _ = checker.check(audio, rate, config, "target")
            with dev.lock:
                buf = dev.upload_frames(array)
                dev.synchronize()
            took = time.perf_counter() - t0
            buf.release()
            return took

        def device_route():
            t0 = time.perf_counter()
            audio, rate = audio_io.load(path, "target", folder, pcm=True)
            assert takes_resident(audio, rate, internal)
            with dev.lock:
                track = dev.track_frames(audio, rate, internal)
                peaks = dev.peak_count(track, 2 * track.frames)
            checker.check(audio, rate, config, "target", peaks=peaks, on_device=True)
            with dev.lock:
                dev.synchronize()
            took = time.perf_counter() - t0
            track.release()
            return took

        def kernel(repeats=5):
            audio, rate = audio_io.load(path, "target", folder, pcm=True)
            best = None
            with dev.lock:
                decoded = dev.upload_frames(audio)
                dev.synchronize()
                for _ in range(repeats):
                    dev.timer_start()
                    track = dev.resample_frames(decoded, frames, 2, rate, internal)
                    ms = dev.timer_stop()
                    track.release()
                    best = ms if best is None else min(best, ms)
                decoded.release()
            return best

        kernel(2)                                                  # the plan's design and upload, the first launch
        if args.kernel_only:
            print(json.dumps({"kernel_ms": kernel()}))
            return
        device_route()
        for _ in range(args.repeats):
            rows["host_route_s"].append(host_route())
            rows["device_route_s"].append(device_route())
            rows["kernel_ms"].append(kernel())

    n_out = int(frames * (float(internal) / args.rate))
    width = 2 * _Plan(args.rate, internal).taps
    best = min(rows["kernel_ms"]) * 1e-3
    host = rows["host_route_s"]
    report = {
        "file": f"{args.minutes:g} minutes of {args.rate} Hz PCM_16 stereo -> {internal} Hz",
        "frames_in": frames, "frames_out": n_out, "row_entries": width,
        **{k: [round(v, 6) for v in vs] for k, vs in rows.items()},
        "host_route_spread_s": round(max(host) - min(host), 6),
        "device_route_gain_s": round(min(host) - max(rows["device_route_s"]), 6),
        "speedup_median": round(sorted(host)[len(host) // 2] / sorted(rows["device_route_s"])[len(host) // 2], 1),
        "kernel_bytes": 8 * (frames + n_out), "kernel_fma": 2 * width * n_out,
        "kernel_bytes_per_s": round(8 * (frames + n_out) / best, 0),
        "kernel_f64_fma_per_s": round(2 * width * n_out / best, 0),
    }
    line = json.dumps(report)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
