"""Write a master AT a delivery specification: one 24-bit file at -14 LUFS under a -1 dBTP true-peak ceiling (what the
streaming services ask for), one dithered 16-bit file (what a CD is cut from), and the plain result beside them.

A ``Delivery`` rides on a ``Result``.  The rendering is measured on the GPU (ITU-R BS.1770-4), ONE linear gain brings it to
the target -- never past the ceiling, which holds for the written file as a meter reads it back --, and gain, dither,
quantisation and packing are one pass over the frames.  ``loudness=`` also receives ("delivered:" + file, Delivered): the
gain, the loudness and true peak it leads to, and by how much the ceiling kept the loudness under the target, if it did.

    python examples/delivery.py [target.wav reference.wav]
"""
import sys

import matchering_amd as mg

mg.log(print)
target, reference = sys.argv[1:3] if len(sys.argv) >= 3 else ("my_song.wav", "some_popular_song.wav")

results = [
    mg.pcm24("my_song_streaming_24bit.wav", delivery=mg.Delivery(loudness=-14.0, true_peak=-1.0)),
    mg.pcm16("my_song_cd_16bit.wav", delivery=mg.Delivery(dither="tpdf_hp", seed=2024)),
    mg.pcm24("my_song_master_24bit.wav"),
]


def report(name, value):
    if name.startswith("delivered:"):
        print(f"{name[len('delivered:'):]}: {value}")


mg.process(target=target, reference=reference, results=results, loudness=report)

for item in results:
    print(f"{item.file} as written: {mg.measure(item.file)}")
