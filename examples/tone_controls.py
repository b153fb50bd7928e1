"""One pair, three masters under the matching EQ's tone controls.

    python examples/tone_controls.py target.wav reference.wav

``match_range=(60, 12000)`` matches the target to the reference between 60 Hz and 12 kHz only and leaves its lowest and
highest octaves alone; ``side_amount=0`` keeps the target's stereo image while the tone is matched.  ``mono_below_hz=120``
takes the side channel out below 120 Hz: a linear-phase high-pass on the side curve, time-aligned for free.  A
``ToneBand`` and a tilt trim the result on top of the match: "as the reference, but +1 dB air and a touch darker".
``curves()`` gives what a front end plots, without a GPU.  Levels are matched as always.
"""
import sys

import numpy as np

import matchering_amd as mg


def main(target, reference):
    mg.log(print)
    masters = {
        "range_image_kept.wav": mg.MatchingEq(match_range=(60.0, 12000.0), side_amount=0.0),
        "mono_bass.wav": mg.MatchingEq(mono_below_hz=120.0),
        "air_and_tilt.wav": mg.MatchingEq(tilt_db_per_octave=-0.3, bands=(mg.ToneBand("high_shelf", 10000.0, 1.0),)),
    }
    config = mg.Config()
    for name, eq in masters.items():
        mg.process(target, reference, [mg.pcm16(name)], config=config, eq=eq)
        curves = eq.curves(config)
        print(f"{name}: {eq.describe()}")
        for hz in (30.0, 60.0, 120.0, 1000.0, 10000.0, 16000.0):
            k = int(np.argmin(np.abs(curves["hz"] - hz)))
            mid, side = curves["mid"], curves["side"]
            print(f"  {curves['hz'][k]:8.1f} Hz: match weight mid {mid['weight'][k]:.3f} side {side['weight'][k]:.3f}, "
                  f"trim {mid['trim_db'][k]:+.2f} dB, side gate {side['gate'][k]:.3f}")


if __name__ == "__main__":
    main(*sys.argv[1:3])
