#!/usr/bin/env python
"""What the matching EQ's controls cost: the FIR design stage with and without a shape, on the same resident pair.

    python tools/bench_eq_shape.py [--minutes 8] [--repeats 7] [--out profiles/eq_shape.json]

One synthetic pair of ``--minutes`` is uploaded once per fft_size.  Each repeat runs ``mgx_master`` with ``eq=None`` and
then with each shape of the size, one after the other, with stage timing on (HIP events on the handle's stream around
the ``design_fir`` stage): the variants alternate within the job, so a drift of the machine's clocks meets all of them.
min / median / max over the repeats are reported, and a variant counts as slower than ``eq=None`` only where its min lies
above the plain stage's max.  The whole call (events around ``mgx_master``, no stage timing) is measured the same way
for ``eq=None`` against ``MatchingEq()``, the shape that changes nothing and launches nothing.  Prints one JSON line;
``--out`` also writes it.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = {
    4096: {"linear_shaped": dict(amount=0.5, max_boost_db=6.0, max_cut_db=6.0), "minimum_phase": dict(phase="minimum")},
    16384: {"minimum_phase": dict(phase="minimum")},
}


def summary(values):
    ordered = sorted(values)
    return {"min": round(ordered[0], 4), "median": round(ordered[len(ordered) // 2], 4), "max": round(ordered[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=8.0)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.repeats < 3:
        ap.error("at least three repeats")

    import matchering_amd as mg
    from matchering_amd import _native
    from matchering_amd.device import default_device
    from matchering_amd.synth import make_pair

    dev = default_device()
    target, reference = make_pair(args.minutes * 60.0, 44100, pair=0)
    n, nr = target.shape[0], reference.shape[0]
    report = {"pair": f"{args.minutes:g} minutes at 44.1 kHz", "repeats": args.repeats,
              "library": os.path.basename(_native.LIB_PATH), "design_fir_ms": {}, "mgx_master_ms": {}}
    with dev.lock:
        td, rd, out = dev.upload(target), dev.upload(reference), dev.alloc(n * 8)
        dev.synchronize()
        for fft, variants in VARIANTS.items():
            cfg = mg.Config(fft_size=fft).to_native()
            shapes = {"eq_none": None, **{name: mg.MatchingEq(**kw) for name, kw in variants.items()}}

            def call(eq):
                dev.master(td, n, rd, nr, cfg, result=out, want_report=False, eq=eq)

            for eq in shapes.values():                              # plans, twiddles, scratch, first launches
                call(eq)
                call(eq)
            dev.synchronize()
            dev.stage_timing(True)
            rows = {name: [] for name in shapes}
            for _ in range(args.repeats):
                for name, eq in shapes.items():
                    call(eq)
                    rows[name].append(dev.stage_times()["design_fir"])
            dev.stage_timing(False)
            plain = summary(rows["eq_none"])
            entry = {}
            for name, values in rows.items():
                s = summary(values)
                entry[name] = {**s, "all": [round(v, 4) for v in values]}
                if name != "eq_none":
                    entry[name]["added_median"] = round(s["median"] - plain["median"], 4)
                    entry[name]["slower_beyond_the_spread"] = bool(s["min"] > plain["max"])
            report["design_fir_ms"][str(fft)] = entry
            if fft == 4096:                                         # the whole call, events around it, nothing else on
                whole = {"eq_none": [], "default_shape": []}
                for _ in range(args.repeats):
                    for name, eq in (("eq_none", None), ("default_shape", mg.MatchingEq())):
                        dev.timer_start()
                        call(eq)
                        whole[name].append(dev.timer_stop())
                report["mgx_master_ms"] = {name: {**summary(v), "all": [round(x, 4) for x in v]} for name, v in whole.items()}
        for b in (td, rd, out):
            b.release()
    line = json.dumps(report)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
