#!/usr/bin/env python
"""What the matching EQ's tone controls cost: the FIR design stage without an eq, with a shape, and with a full tone, on
the same resident pair (tools/bench_eq_shape.py's method).

    python tools/bench_eq_tone.py [--minutes 8] [--repeats 7] [--label tree] [--out profiles/eq_tone.json]

One synthetic pair of ``--minutes`` is uploaded once.  Each repeat runs ``mgx_master`` with ``eq=None``, with the shape of
DESIGN 3.16 (amount 0.5, +-6 dB) and with a full tone on top of it, one after the other, with stage timing on (HIP events
around the ``design_fir`` stage): the variants alternate within the job, so a drift of the machine's clocks meets all of
them.  min / median / max over the repeats are reported.  Copied into a tree from before the tone controls the tool runs
there too and leaves the toned variant out: that is how the shaped stage of two trees is compared on one box.  Prints
one JSON line; ``--out`` also writes it.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPED = dict(amount=0.5, max_boost_db=6.0, max_cut_db=6.0)


def summary(values):
    ordered = sorted(values)
    return {"min": round(ordered[0], 4), "median": round(ordered[len(ordered) // 2], 4), "max": round(ordered[-1], 4),
            "all": [round(v, 4) for v in values]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=8.0)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--label", default="tree")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.repeats < 3:
        ap.error("at least three repeats")

    import matchering_amd as mg
    from matchering_amd import _native
    from matchering_amd.device import default_device
    from matchering_amd.synth import make_pair

    eqs = {"eq_none": None, "shaped": mg.MatchingEq(**SHAPED)}
    if hasattr(mg, "ToneBand"):
        eqs["full_tone"] = mg.MatchingEq(match_range=(60.0, 12000.0), side_amount=0.3, mono_below_hz=120.0,
                                         tilt_db_per_octave=-0.5,
                                         bands=(mg.ToneBand("high_shelf", 10000.0, 1.0), mg.ToneBand("bell", 300.0, -2.0, q=1.4)),
                                         **SHAPED)
    dev = default_device()
    target, reference = make_pair(args.minutes * 60.0, 44100, pair=0)
    n, nr = target.shape[0], reference.shape[0]
    report = {"label": args.label, "pair": f"{args.minutes:g} minutes at 44.1 kHz", "repeats": args.repeats, "fft_size": 4096,
              "library": os.path.abspath(_native.LIB_PATH), "design_fir_ms": {}}
    with dev.lock:
        td, rd, out = dev.upload(target), dev.upload(reference), dev.alloc(n * 8)
        dev.synchronize()
        cfg = mg.Config().to_native()

        def call(eq):
            dev.master(td, n, rd, nr, cfg, result=out, want_report=False, eq=eq)

        for eq in eqs.values():                                 # plans, scratch, first launches
            call(eq)
            call(eq)
        dev.synchronize()
        dev.stage_timing(True)
        rows = {name: [] for name in eqs}
        for _ in range(args.repeats):
            for name, eq in eqs.items():
                call(eq)
                rows[name].append(dev.stage_times()["design_fir"])
        dev.stage_timing(False)
        report["design_fir_ms"] = {name: summary(values) for name, values in rows.items()}
        for b in (td, rd, out):
            b.release()
    line = json.dumps(report)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
