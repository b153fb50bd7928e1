#!/usr/bin/env python
"""The pair route against the reference-profile route inside ONE process (one box, one clock state).

    python tools/bench_profile.py [--seconds 480] [--sample-rate 44100] [--fft-size 4096] [--passes 3] [--blocks 6]
                                  [--steps 10] [--json FILE] [--batch]

The workload is bench.py's: the synthetic pair of matchering_amd/synth.py, resident in HBM, all three outputs of
stages.main left aside but the limited one.  Both routes are warmed, then timed in alternation: a BLOCK is `steps`
calls of one route between two events, ending in a synchronise (the step time is the block's time over `steps`), and
a PASS is `blocks` blocks, routes alternating.  Per route: min / median / max of the block step times, the medians of
mgx_stage_times for `analyze` and `design_fir` (taken in blocks of their own, since stage events add to the stream),
and the bytes per frame the model of DESIGN.md section 3 books.  The verdicts printed at the end are the two the
route must meet: its step and its curve stage no slower than the pair route's by more than the pair route's own
min-to-max spread.

--batch adds the PCIe-inclusive figure: process_batch on three jobs sharing one reference file, with and without
share_references -- wall time to the last file and the megabytes of input uploaded.
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# bytes per frame of the whole step at equal lengths (the analysis reads 8 B of each track)
MODEL_BYTES_PER_FRAME = {"pair": 72, "profile": 64}


def spread(values):
    return {"min": min(values), "median": statistics.median(values), "max": max(values)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=480.0)
    ap.add_argument("--sample-rate", type=int, default=44100)
    ap.add_argument("--fft-size", type=int, default=4096)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--json", default=None)
    ap.add_argument("--batch", action="store_true")
    args = ap.parse_args()

    import matchering_amd as mg
    from matchering_amd import ReferenceProfile
    from matchering_amd.device import Device, DeviceFrames
    from matchering_amd.synth import make_pair

    dev = Device(0)
    cfg = mg.Config(internal_sample_rate=args.sample_rate, fft_size=args.fft_size)
    native = cfg.to_native()
    target, reference = make_pair(args.seconds, args.sample_rate, pair=0)
    n, nr = target.shape[0], reference.shape[0]
    t_dev, r_dev = dev.upload(target), dev.upload(reference)
    out = dev.alloc(n * 8)
    profile = ReferenceProfile.analyze(DeviceFrames(r_dev, nr), cfg, device=dev)
    p_dev = profile.resident(dev)

    def step(route):
        if route == "pair":
            dev.master(t_dev, n, r_dev, nr, native, result=out, want_report=False)
        else:
            dev.master(t_dev, n, None, 0, native, result=out, want_report=False, profile=p_dev)

    routes = ("pair", "profile")
    got = {}
    for route in routes:                     # warm-up (code objects, FIR operator, workspaces) + what the routes compute
        for _ in range(3):
            step(route)
        dev.synchronize()
        got[route] = np.array(dev.download(out, (n, 2)))
    diff = got["profile"].astype(np.float64) - got["pair"]
    agreement = {"rms": float(np.sqrt(np.mean(diff * diff))), "max": float(np.abs(diff).max())}
    print(f"profile route vs pair route on this workload: rms {agreement['rms']:.3e}, max {agreement['max']:.3e}")

    steps_ms = {route: [] for route in routes}
    for _ in range(args.passes):
        for block in range(args.blocks):
            route = routes[block % 2]
            dev.synchronize()
            dev.timer_start()
            for _ in range(args.steps):
                step(route)
            steps_ms[route].append(dev.timer_stop() / args.steps)
    stage_ms = {route: {"analyze": [], "design_fir": []} for route in routes}
    dev.stage_timing(True)
    for _ in range(args.passes * args.blocks // 2):
        for route in routes:
            step(route)
            times = dev.stage_times()
            for name in stage_ms[route]:
                stage_ms[route][name].append(times[name])
    dev.stage_timing(False)

    report = {"workload": {"seconds": args.seconds, "sample_rate": args.sample_rate, "fft_size": args.fft_size,
                           "frames": [n, nr]},
              "passes": args.passes, "blocks_per_pass": args.blocks, "steps_per_block": args.steps,
              "agreement": agreement, "routes": {}}
    for route in routes:
        report["routes"][route] = {
            "step_ms": spread(steps_ms[route]), "blocks": len(steps_ms[route]),
            "stage_ms": {name: spread(values) for name, values in stage_ms[route].items()},
            "model_bytes_per_frame": MODEL_BYTES_PER_FRAME[route]}
    pair, prof = report["routes"]["pair"], report["routes"]["profile"]
    step_spread = pair["step_ms"]["max"] - pair["step_ms"]["min"]
    report["verdicts"] = {
        "pair_step_spread_ms": step_spread,
        "step_not_slower": prof["step_ms"]["median"] <= pair["step_ms"]["median"] + step_spread,
        "curve_stage_not_slower": prof["stage_ms"]["design_fir"]["median"]
                                  <= pair["stage_ms"]["design_fir"]["median"] + step_spread}
    print(f"{'route':9s}{'step min':>10s}{'median':>10s}{'max':>10s}{'analyze':>10s}{'design_fir':>12s}{'B/frame':>9s}   (ms)")
    for route in routes:
        r = report["routes"][route]
        print(f"{route:9s}{r['step_ms']['min']:10.4f}{r['step_ms']['median']:10.4f}{r['step_ms']['max']:10.4f}"
              f"{r['stage_ms']['analyze']['median']:10.4f}{r['stage_ms']['design_fir']['median']:12.4f}"
              f"{r['model_bytes_per_frame']:9d}")
    print("verdicts:", json.dumps(report["verdicts"]))

    if args.batch:
        report["batch"] = batch_figure(mg, args)
        print("process_batch, three jobs sharing a reference (PCIe and file I/O included):", json.dumps(report["batch"]))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(report, fh, indent=1)
    print(json.dumps({"bench_profile": report["routes"], "verdicts": report["verdicts"]}))


def batch_figure(mg, args):
    """Wall time to the last file and input megabytes uploaded for three jobs that share one reference file."""
    from matchering_amd import audio_io, device
    from matchering_amd.synth import make_pair

    folder = tempfile.mkdtemp(prefix="bench_profile_")
    rate = args.sample_rate
    reference = make_pair(args.seconds, rate, pair=0)[1]
    rp = os.path.join(folder, "reference.wav")
    audio_io.write_wav(rp, reference, rate, "PCM_16")
    jobs = []
    for i in range(3):
        tp = os.path.join(folder, f"target{i}.wav")
        audio_io.write_wav(tp, make_pair(args.seconds, rate, pair=i + 1)[0], rate, "PCM_16")
        jobs.append({"target": tp, "reference": rp, "results": [mg.pcm16(os.path.join(folder, f"out{i}.wav"))]})
    cfg = mg.Config(internal_sample_rate=rate, fft_size=args.fft_size)
    uploaded = [0]
    real = device.Device.upload_frames

    def counting(self, array):
        uploaded[0] += array.nbytes
        return real(self, array)

    device.Device.upload_frames = counting
    figures = {}
    try:
        mg.process_batch(jobs, cfg, rank=0, world_size=1, lanes=2)            # warm-up: lanes, plans, page cache
        for share in (False, True, False, True):
            uploaded[0] = 0
            t0 = time.perf_counter()
            mg.process_batch(jobs, cfg, rank=0, world_size=1, lanes=2, share_references=share)
            key = "shared" if share else "per_job"
            figures.setdefault(key, []).append({"wall_ms": (time.perf_counter() - t0) * 1e3,
                                                "input_MB_uploaded": uploaded[0] / 1e6})
    finally:
        device.Device.upload_frames = real
        shutil.rmtree(folder, ignore_errors=True)
    return figures


if __name__ == "__main__":
    main()
