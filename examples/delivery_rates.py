"""Deliver one master at three rates: a 44.1 kHz 16-bit file with dither (CD), a 48 kHz 24-bit file at -14 LUFS under
-1 dBTP (video, streaming) and a 96 kHz float file (hi-res store).  ``Delivery(sample_rate=...)`` converts the rendering on
the GPU (``mgx_convert_rate``, the loader's kaiser_best filter) BEFORE it is measured, so the loudness and the true-peak
ceiling are those of the file as written at its own rate: a conversion made afterwards, somewhere else, would move the
inter-sample peaks and quantise a second time.  A rate the converter does not take (more than 4096 phases, such as
44100 -> 44056 Hz) is a ``ValueError`` before a file is read: there is no approximate route.

    python examples/delivery_rates.py [target.wav reference.wav]
"""
import sys

import matchering_amd as mg

mg.log(print)
target, reference = sys.argv[1:3] if len(sys.argv) >= 3 else ("my_song.wav", "some_popular_song.wav")

results = [
    mg.pcm16("my_song_cd_44k1_16bit.wav", delivery=mg.Delivery(dither="tpdf_hp", seed=2024, sample_rate=44100)),
    mg.pcm24("my_song_video_48k_24bit.wav", delivery=mg.Delivery(loudness=-14.0, true_peak=-1.0, sample_rate=48000)),
    mg.Result("my_song_hires_96k_float.wav", "FLOAT", delivery=mg.Delivery(true_peak=-1.0, sample_rate=96000)),
]


def report(name, value):
    if name.startswith("delivered:"):
        print(f"{name[len('delivered:'):]}: {value.frames} frames at {value.sample_rate} Hz: {value}")


mg.process(target=target, reference=reference, results=results, loudness=report)

for item in results:
    print(f"{item.file} as written: {mg.measure(item.file)}")
