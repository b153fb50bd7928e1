"""One pair, three masters: the whole matching EQ, half of it under caps, and the whole of it in minimum phase.

    python examples/matching_eq.py target.wav reference.wav

``MatchingEq(amount=0.5, max_boost_db=6, max_cut_db=6)`` applies half of the matching curve, in dB, and lets no bin be
boosted or cut by more than 6 dB: for a reference whose tonal balance is far from the target's.  ``phase="minimum"``
keeps the curve and moves the FIR's energy behind its main tap: no pre-echo in front of transients, and the result stays
time-aligned with the linear-phase master.  Levels are matched as always: every result reaches the reference's RMS.
"""
import sys

import matchering_amd as mg


def main(target, reference):
    mg.log(print)
    mg.process(target, reference, [mg.pcm16("full.wav")])
    mg.process(target, reference, [mg.pcm16("half_capped.wav")],
               eq=mg.MatchingEq(amount=0.5, max_boost_db=6.0, max_cut_db=6.0))
    mg.process(target, reference, [mg.pcm16("minimum_phase.wav")], eq=mg.MatchingEq(phase="minimum"))


if __name__ == "__main__":
    main(*sys.argv[1:3])
