"""Master a track and read every figure a delivery specification asks for -- integrated loudness in LUFS, loudness range,
true peak in dBTP (ITU-R BS.1770-4, EBU Tech 3341 / 3342) -- from the frames while they are still on the GPU.

``loudness=`` receives (name, Loudness) for the target, the reference, and each rendering the results need, measured
before any encoding; ``mg.measure`` does the same for a file (or an array, or frames already in HBM) on its own."""
import matchering_amd as mg

mg.log(print)


def report(name, value):
    print(f"{name:>30}: {value}")
    if name == "result" and value.true_peak_db > -1.0:
        print(f"{'':>30}  (over a -1 dBTP ceiling by {value.true_peak_db + 1.0:.2f} dB between the samples; "
              f"the sample peak reads {value.sample_peak_db:.2f} dBFS)")


mg.process(
    target="my_song.wav",
    reference="some_popular_song.wav",
    results=[mg.pcm16("my_song_master_16bit.wav"), mg.pcm24("my_song_master_24bit.wav")],
    loudness=report,
)

print(mg.measure("my_song_master_24bit.wav"))
