"""Master a track and have every track, rendering and written file looked at the way a distributor's intake check does:
DC offset, runs of samples at the rail, a stereo image that cancels in mono, dropouts, head and tail silence, samples
that are not finite numbers -- read from the frames while they are still on the GPU.

``audit=`` receives (name, Audit) for the target, the reference, each rendering the results need and, as
"delivered:" + file, for the integer samples a delivery writes; ``mg.audit`` does the same for a file (or an array, or
frames already in HBM) on its own.

    python audit_report.py [target.wav reference.wav]
"""
import sys

import matchering_amd as mg

mg.log(print)
target, reference = sys.argv[1:3] if len(sys.argv) >= 3 else ("my_song.wav", "some_popular_song.wav")


def report(name, value):
    print(f"{name}: {value}")
    for finding, measured, limit in value.findings(head_s=2.0, tail_s=5.0):
        print(f"    {finding}: {measured:.4g} (limit {limit:.4g})")


mg.process(
    target=target,
    reference=reference,
    results=[
        mg.pcm24("my_song_master_24bit.wav"),
        mg.Result("my_song_master_16bit.wav", "PCM_16",
                  delivery=mg.Delivery(loudness=-14.0, true_peak=-1.0, dither="tpdf")),
    ],
    audit=report,
)

# stricter limits for the file that goes out: two samples at full scale are an event, -80 dBFS counts as silence
print(mg.audit("my_song_master_16bit.wav", limits=mg.AuditLimits(clip_level=1.0, clip_run=2, silence_db=-80.0)))
