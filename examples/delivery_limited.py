"""Write a LOUD rendition at a delivery specification: -9 LUFS under a -1 dBTP true-peak ceiling, 16 bit, dithered -- what a
club or a loud-streaming rendition asks for, and more than one linear gain can give: the ceiling stops the gain several LU
short.  A ``TruePeakLimiter`` on the ``Delivery`` makes up for it: where the ceiling binds (and only there) the rendering is
limited on the GPU by a true-peak look-ahead limiter, pass by pass until the loudness is within ``tolerance_lu`` of the
target or more pre-gain buys no more loudness, and the linear gain then trims the limited frames, so that the ceiling
holds for the written file exactly as it does without the limiter.  The ``Delivered`` record says what was done: passes,
pre-gain, the deepest gain reduction, and what is still missing, if anything.

    python examples/delivery_limited.py [target.wav reference.wav]
"""
import sys

import matchering_amd as mg

mg.log(print)
target, reference = sys.argv[1:3] if len(sys.argv) >= 3 else ("my_song.wav", "some_popular_song.wav")

loud = mg.Delivery(loudness=-9.0, true_peak=-1.0, dither="tpdf_hp", seed=2024,
                   limiter=mg.TruePeakLimiter(lookahead_ms=1.5, release_ms=50.0, max_passes=4, tolerance_lu=0.1))
results = [
    mg.pcm16("my_song_loud_16bit.wav", delivery=loud),
    mg.pcm24("my_song_master_24bit.wav"),
]


def report(name, value):
    if name.startswith("delivered:"):
        print(f"{name[len('delivered:'):]}: {value}")
        print(f"  {value!r}")


mg.process(target=target, reference=reference, results=results, loudness=report)

for item in results:
    print(f"{item.file} as written: {mg.measure(item.file)}")
