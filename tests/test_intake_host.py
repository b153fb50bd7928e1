"""``process`` and ``process_batch`` read their files through one intake (matchering_amd/intake.py): without a GPU, with a
stand-in behind ``stages.main``, both hand the stand-in the same arrays and emit the same warning and info codes, whatever
the files hold.
"""

import numpy as np
import pytest

import matchering_amd as mg
from matchering_amd import audio_io, batch, core
from matchering_amd.synth import make_pair
from test_profile_host import make_profile

KINDS = [("PCM_16", 44100, 2, True), ("PCM_24", 44100, 1, True), ("PCM_16", 48000, 2, True), ("FLOAT", 22050, 1, False),
         ("PCM_32", 48000, 2, True), ("PCM_24", 48000, 1, False)]       # (subtype, rate, channels, clipped)
PAIRS = [(0, 0), (0, 3), (1, 2), (1, 5), (2, 1), (2, 4), (3, 0), (3, 3), (4, 2), (4, 5), (5, 1), (5, 4)]
ONLY_PROCESS = (2003, 2008, 2010)           # loading, exporting, completed: process_batch has no such lines
NO_EQUALITY_CHECK = "cannot be checked"


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """{(role, kind): path}: 1.0 s of target and 1.1 s of reference in every kind of file."""
    folder = tmp_path_factory.mktemp("kinds")
    paths = {}
    for kind, (subtype, rate, channels, clipped) in enumerate(KINDS):
        pair = make_pair(1.0, rate, pair=kind, reference_seconds=1.1)
        for role, audio in zip(("target", "reference"), pair):
            if clipped:
                audio = np.clip(8.0 * audio, -1.0, 1.0)
            paths[role, kind] = str(folder / f"{role}{kind}.wav")
            audio_io.write_wav(paths[role, kind], audio[:, :channels], rate, subtype)
    return paths


def _logged(call):
    """(warning and info codes in order, debug lines) of one call."""
    codes, lines = [], []
    take = lambda text: codes.append(int(str(text).split(":")[0]))          # noqa: E731
    mg.log(warning_handler=take, info_handler=take, debug_handler=lines.append, show_codes=True)
    try:
        call()
    finally:
        mg.log()
    return [code for code in codes if code not in ONLY_PROCESS], [str(line) for line in lines]


def _both_ways(tmp_path, monkeypatch, config, target, reference, job_reference):
    """What ``main`` receives and what is logged, by ``process`` and by ``process_batch`` with a stand-in."""
    received = []

    def stand_in(target, reference, config, need_default=True, need_no_limiter=False, need_no_limiter_normalized=False,
                 encodings=None):
        received.append((target, reference))
        return np.zeros((target.shape[0], 2), np.float32), None, None

    monkeypatch.setattr(core, "main", stand_in)
    monkeypatch.setattr(core, "_gpu", lambda: None)
    single = _logged(lambda: mg.process(target, reference, [mg.Result(str(tmp_path / "single.wav"), "FLOAT")], config))
    job = {"target": target, "results": [mg.Result(str(tmp_path / "batch.wav"), "FLOAT")], **job_reference}
    many = _logged(lambda: batch.process_batch([job], config, lanes=1, io_threads=1, master=stand_in))
    assert len(received) == 2
    return received, single, many


@pytest.mark.parametrize("kinds", PAIRS, ids=lambda kinds: f"K{kinds[0]}-K{kinds[1]}")
def test_process_and_batch_hand_main_the_same_pair(files, tmp_path, monkeypatch, kinds):
    target, reference = files["target", kinds[0]], files["reference", kinds[1]]
    received, (codes, _), (batch_codes, _) = _both_ways(tmp_path, monkeypatch, mg.Config(max_piece_size=1.0), target, reference,
                                                        {"reference": reference})
    for single, many in zip(*received):
        assert single.dtype == many.dtype and np.array_equal(single, many)
    if kinds == (0, 3):
        # an on-rate stereo integer target: the batch takes its peak statistics on the lane, after the reference's codes
        assert codes == [3002, 2201, 2202] and batch_codes == [2201, 2202, 3002]
    else:
        assert codes == batch_codes


def test_process_and_batch_hand_main_the_same_target_and_profile(files, tmp_path, monkeypatch):
    config = mg.Config(max_piece_size=1.0)
    saved = str(tmp_path / "reference.profile")
    make_profile(config)[0].save(saved)
    received, (codes, lines), (batch_codes, batch_lines) = _both_ways(tmp_path, monkeypatch, config, files["target", 2], saved,
                                                                      {"reference_profile": saved})
    (target, profile), (batch_target, batch_profile) = received
    assert target.dtype == batch_target.dtype and np.array_equal(target, batch_target)
    assert profile == batch_profile == make_profile(config)[0]
    assert codes == batch_codes and codes
    assert any(NO_EQUALITY_CHECK in line for line in lines) and any(NO_EQUALITY_CHECK in line for line in batch_lines)
