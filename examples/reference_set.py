"""Master to "the sound of" several records at once: a set of references becomes ONE profile.  Every reference is
analysed on its own (peak-normalised, cut into pieces, its loud pieces chosen against its own average), then the loud
pieces of all of them are pooled: the matching spectrum and level are their means.  The merged profile is an ordinary
one: save it, master against it, or merge it again with next year's records."""
import matchering_amd as mg

config = mg.Config()

records = ["first_record.wav", "second_record.wav", "third_record.wav"]
profile = mg.ReferenceProfile.analyze(records, config)          # a list in a reference's place: a set
profile.save("label_sound.profile")
print(profile)

for song in ("my_song", "my_other_song"):
    mg.process(
        target=f"{song}.wav",
        reference="label_sound.profile",
        results=[mg.pcm16(f"{song}_master_16bit.wav")],
        config=config,
    )

# The same in one call per song, and with a record that counts twice (weights are whole numbers):
#   mg.process("my_song.wav", records, [mg.pcm16("my_song_master_16bit.wav")], config)
#   singles = [mg.ReferenceProfile.analyze(record, config) for record in records]
#   profile = mg.ReferenceProfile.merge(singles, weights=[2, 1, 1])
