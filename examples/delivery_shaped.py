"""A CD-width result with noise-shaped dither: the quantiser's error is fed back through a published 9-tap filter, which
moves the noise out of the 2-5 kHz region, where the ear is most sensitive, to the top of the band.

    python examples/delivery_shaped.py target.wav reference.wav

``dither`` names one of the library's presets -- "lipshitz5" (Lipshitz, Vanderkooy, Wannamaker 1991) or "wannamaker9"
(Wannamaker 1992, F-weighted), both designed for 44.1 kHz and handed out for file rates of 44.1 to 48 kHz -- or is a
``NoiseShaper`` with coefficients of one's own.  The true-peak ceiling holds for the written file as before: the gain
leaves the larger head-room a shaped quantiser needs.
"""
import sys

import matchering_amd as mg


def main(target, reference):
    mg.log(print)
    records = {}
    mg.process(target, reference, [
        mg.pcm16("cd_shaped.wav", delivery=mg.Delivery(true_peak=-1.0, dither="wannamaker9", seed=1)),
        mg.pcm16("cd_tpdf.wav", delivery=mg.Delivery(true_peak=-1.0, dither="tpdf", seed=1)),
        # a first-order high-pass of one's own, at any rate
        mg.pcm24("own.wav", delivery=mg.Delivery(true_peak=-1.0, dither=mg.NoiseShaper((1.0,)))),
    ], loudness=lambda name, value: records.__setitem__(name, value))
    for name, value in records.items():
        if name.startswith("delivered:"):
            print(f"{name[len('delivered:'):]}: {value}")


if __name__ == "__main__":
    main(*sys.argv[1:3])
