"""Keep "the sound of" a reference without keeping its audio: analyse it once, save the profile (a few kilobytes:
two scalars and the two averaged spectra stages.main takes from a reference), and master any number of songs
against the saved file.  A profile belongs to the Config it was made with; `process` refuses any other by name."""
import matchering_amd as mg

config = mg.Config()

profile = mg.ReferenceProfile.analyze("some_popular_song.wav", config)
profile.save("some_popular_song.profile")
print(profile)

for song in ("my_song", "my_other_song"):
    mg.process(
        target=f"{song}.wav",
        reference="some_popular_song.profile",      # recognised by the file's first bytes, not by its name
        results=[mg.pcm16(f"{song}_master_16bit.wav")],
        config=config,
    )
