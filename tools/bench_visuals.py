#!/usr/bin/env python
"""The visuals against what a caller does without them: download every frame and transform on the host.

    python tools/bench_visuals.py [--minutes 8] [--rate 44100] [--repeats 5] [--out profiles/visuals_8min.json]

One stereo track of noise of ``--minutes`` is uploaded once; each repeat then times, one after the other,
``mgx_spectrogram`` at the defaults (4096 points, hop 1024) pooled to 1024 columns of 96 logarithmic bands,
``mgx_overview`` at 2048 columns, and ``Device.download`` of the frames alone -- HIP events on the handle's stream around
the one blocking call, launches, the copy of the result and the wait for it included, as a caller pays them.  The three
alternate within the job, so a drift of the machine's clocks meets all of them; min / median / max over the repeats are
reported.  The host's share of today's route -- the same picture by ``scipy.fft`` in float32 from the downloaded frames,
on at most 16 workers -- is timed by the wall clock once per repeat and reported beside them.  "Faster than the download
alone" is recorded only where the medians differ by more than either spread.  Prints one JSON line; ``--out`` also
writes it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(values):
    ordered = sorted(values)
    return {"min": round(ordered[0], 4), "median": round(ordered[len(ordered) // 2], 4), "max": round(ordered[-1], 4)}


def host_picture(x, fft_size, hop, columns, edges, workers):
    """The same picture on the host in float32: hops in blocks, scipy's real transform over ``workers`` threads."""
    import scipy.fft

    n = x.shape[0]
    hops = (n - 1) // hop + 1
    window = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(fft_size) / fft_size)).astype(np.float32)
    scale = np.float32((2.0 / float(window.astype(np.float64).sum())) ** 2)
    padded = np.zeros((n + 2 * fft_size, 2), dtype=np.float32)
    padded[fft_size // 2:fft_size // 2 + n] = x
    bounds = np.arange(columns + 1, dtype=np.int64) * hops // columns
    out = np.zeros((columns, 2, edges.size - 1), dtype=np.float32)
    block = 64
    for c0 in range(0, columns, block):
        c1 = min(columns, c0 + block)
        t0, t1 = int(bounds[c0]), int(bounds[c1])
        index = (np.arange(t0, t1) * hop)[:, None] + np.arange(fft_size)[None, :]
        seg = padded[index] * window[None, :, None]                                # (hops, N, 2)
        spec = scipy.fft.rfft(seg, axis=1, workers=workers)
        power = (spec.real ** 2 + spec.imag ** 2) * scale
        for c in range(c0, c1):
            mean = power[int(bounds[c]) - t0:int(bounds[c + 1]) - t0].mean(axis=0)  # (bins, 2)
            out[c] = np.add.reduceat(mean, edges[:-1], axis=0).T / np.diff(edges)[None, :]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=8.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.repeats < 3:
        ap.error("at least three repeats")

    from matchering_amd import _native, visuals
    from matchering_amd.device import default_device

    dev = default_device()
    frames = int(args.minutes * 60 * args.rate)
    fft_size, hop, columns, overview_columns = 4096, 1024, 1024, 2048
    edges = visuals.log_bands(fft_size, args.rate, 96)
    workers = min(16, os.cpu_count() or 1)
    noise = 0.1 * np.random.default_rng(5).standard_normal((frames, 2), dtype=np.float32)
    with dev.lock:
        x = dev.upload(noise)
        dev.synchronize()
        del noise
        kept = {}

        def timed(call):
            dev.timer_start()
            call()
            return dev.timer_stop()

        calls = {"mgx_spectrogram_ms": lambda: kept.__setitem__("picture", dev.spectrogram(x, frames, args.rate, fft_size, hop, columns, edges)),
                 "mgx_overview_ms": lambda: dev.overview(x, frames, args.rate, overview_columns),
                 "download_ms": lambda: kept.__setitem__("host", dev.download(x, (frames, 2)))}
        for _ in range(2):                                          # the window, the scratch, the first launches
            for call in calls.values():
                call()
        rows = {name: [] for name in calls}
        rows["host_scipy_float32_ms"] = []
        for _ in range(args.repeats):
            for name, call in calls.items():
                rows[name].append(timed(call))
            begin = time.perf_counter()
            on_host = host_picture(kept["host"], fft_size, hop, columns, edges, workers)
            rows["host_scipy_float32_ms"].append((time.perf_counter() - begin) * 1e3)
        picture = kept["picture"].power
        agreement = float(np.max(np.abs(picture - on_host)) / np.max(on_host))
        x.release()
    dev.trim()
    stats = {name: summary(values) for name, values in rows.items()}
    download = stats["download_ms"]
    report = {"track": f"{args.minutes:g} minutes of stereo noise at {args.rate} Hz", "frames": frames, "repeats": args.repeats,
              "library": os.path.basename(_native.LIB_PATH), "fft_size": fft_size, "hop": hop, "hops": kept["picture"].hops,
              "columns": columns, "bands": int(edges.size - 1), "overview_columns": overview_columns, "host_workers": workers,
              "picture_bytes": int(picture.nbytes), "frames_bytes": frames * 8,
              "gpu_against_host_picture_max_error_of_peak": agreement,
              **stats, "all_ms": {k: [round(v, 4) for v in vs] for k, vs in rows.items()}}
    for name in ("mgx_spectrogram_ms", "mgx_overview_ms"):
        mine = stats[name]
        spread = max(mine["max"] - mine["min"], download["max"] - download["min"])
        report[name.replace("_ms", "")] = {
            "ratio_of_medians_download_over_call": round(download["median"] / mine["median"], 2),
            "spread_ms": round(spread, 4),
            "faster_than_the_download_alone_beyond_the_spread": bool(download["median"] - mine["median"] > spread),
            "slower_than_the_download_alone_beyond_the_spread": bool(mine["median"] - download["median"] > spread),
            "frames_GB_per_s_at_the_median": round(frames * 8 / (mine["median"] * 1e-3) / 1e9, 1)}
    line = json.dumps(report)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
