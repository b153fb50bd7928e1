"""A 48 kHz target against a mono 22.05 kHz reference: neither file is at ``Config.internal_sample_rate`` (44.1 kHz).

Nothing changes for the caller -- the log shows the reference's codes (3003 the target was resampled, 2201 / 2202 the
reference is mono and was resampled) -- but with a GPU both files go up as they are and are converted there
(``mgx_resample``), instead of passing through the host's float64 resampler first."""
import matchering_amd as mg

mg.log(print, show_codes=True)

mg.process(
    target="my_song_48k.wav",
    reference="some_popular_song_mono_22k.wav",
    results=[mg.pcm16("my_song_master_16bit.wav"), mg.pcm24("my_song_master_24bit.wav")],
)
