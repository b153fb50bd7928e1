"""Master a synthetic pair and draw what a mastering front end shows beside the numbers: the spectrogram of the target
(before), of the result (after) and of the reference, as greyscale PNGs, and their long-term average spectra in
third-octave-like bands -- all computed from the frames while they are on the GPU; a few hundred kilobytes come back
instead of every frame.

``visuals=`` receives (name, Visuals) for the target, the reference and each rendering the results need;
``mg.spectrogram`` and ``mg.overview`` do the same for a file (or an array, or frames already in HBM) on their own.

    python visuals_report.py [seconds]
"""
import os
import sys

import numpy as np

import matchering_amd as mg
from matchering_amd import audio_io, visuals
from matchering_amd.synth import make_pair

seconds = float(sys.argv[1]) if len(sys.argv) >= 2 else 20.0
rate = 44100
target, reference = make_pair(seconds, rate, pair=0, reference_seconds=0.9 * seconds)
audio_io.save("visuals_target.wav", target, rate, "FLOAT")
audio_io.save("visuals_reference.wav", reference, rate, "FLOAT")

pictures = {}
sizes = visuals.VisualsRequest(overview_columns=1024, fft_size=4096, hop=1024, columns=512, bands=96)
mg.process(
    target="visuals_target.wav",
    reference="visuals_reference.wav",
    results=[mg.pcm24("visuals_master_24bit.wav")],
    visuals=(lambda name, value: pictures.__setitem__(name, value), sizes),
)
for name, file in (("target", "visuals_before.png"), ("result", "visuals_after.png"), ("reference", "visuals_reference.png")):
    pictures[name].spectrogram.save_png(file, top_db=-10.0, range_db=90.0)
    drawn = pictures[name].overview
    print(f"{file}: {pictures[name].spectrogram.columns} columns of {len(sizes.edges(rate)) - 1} bands; "
          f"waveform {drawn.columns} columns, peak {max(float(np.max(drawn.hi)), -float(np.min(drawn.lo))):.3f}")

# the long-term average spectrum: one column; about three bands to the octave from 25 Hz up
thirds = visuals.log_bands(4096, rate, 30, f_lo=25.0)
spectra = {name: mg.spectrogram(file, fft_size=4096, hop=1024, columns=1, bands=thirds, channels="ms")
           for name, file in (("before", "visuals_target.wav"), ("after", "visuals_master_24bit.wav"),
                              ("reference", "visuals_reference.wav"))}
print("long-term average spectrum of the mid channel, dB")
print("      Hz    before     after reference")
hz = spectra["before"].band_hz
for band in range(hz.shape[0]):
    row = "  ".join(f"{spectra[name].db(-150.0)[0, 0, band]:8.2f}" for name in ("before", "after", "reference"))
    print(f"{np.sqrt(max(hz[band, 0], 1.0) * hz[band, 1]):8.0f}  {row}")
print("written:", ", ".join(sorted(f for f in os.listdir(".") if f.startswith("visuals_") and f.endswith(".png"))))
