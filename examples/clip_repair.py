"""Master a target that was hard-clipped, with and without clip repair: the short flat tops are rebuilt on the GPU from
the samples around them before the matching EQ and the level correction see them.

``repair=`` takes a ``ClipRepair`` (or a pair ``(callable, ClipRepair)``: the callable receives ("target", Repaired));
``mg.repair_clipping`` does the same for a file or an array on its own and hands the frames back.  The pair is synthetic,
so the example runs anywhere:

    python clip_repair.py [folder for the files]
"""
import os
import sys
import tempfile

import numpy as np

import matchering_amd as mg
from matchering_amd import audio_io
from matchering_amd.synth import make_pair

folder = sys.argv[1] if len(sys.argv) >= 2 else tempfile.mkdtemp(prefix="clip_repair_")
rate = 44100
clean, reference = make_pair(6.0, rate)
clean = clean / np.max(np.abs(clean))
target = np.clip(clean, -0.6, 0.6).astype(np.float32)          # the top 4.4 dB of the mix are gone
paths = {name: os.path.join(folder, name + ".wav") for name in ("target", "reference", "master", "master_repaired")}
audio_io.save(paths["target"], target, rate, "FLOAT")
audio_io.save(paths["reference"], reference, rate, "PCM_24")

# on its own: the frames and what was done
frames, found = mg.repair_clipping(paths["target"])
print(found.describe())
for name, x in (("clipped", target), ("repaired", frames)):
    error = np.sqrt(np.mean((x.astype(np.float64) - clean) ** 2))
    print(f"{name}: RMS error against the unclipped mix {20 * np.log10(error):.1f} dB")

# in the master: everything downstream of the upload hears the repaired target
mg.process(paths["target"], paths["reference"], [mg.pcm24(paths["master"])])
mg.process(paths["target"], paths["reference"], [mg.pcm24(paths["master_repaired"])],
           repair=(lambda name, value: print(f"{name}: {value.describe()}"), mg.ClipRepair(max_run=48)))
print("written:", paths["master"], paths["master_repaired"])
