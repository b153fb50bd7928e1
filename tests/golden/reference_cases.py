#!/usr/bin/env python
"""Frozen answers of the UNMODIFIED reference for tests/test_oracle_vs_reference.py and tests/test_host_vs_reference.py.

    python tests/golden/reference_cases.py        (needs the reference tree, oracle/reference_runner.py)

The cases below are run through the reference's own ``stages.main``, ``checker.check`` and
``preview_creator.create_preview`` (I/O imports stubbed, LOWESS served by the oracle's restatement, as
oracle/reference_runner.py does) and their results are stored in ``reference_cases/<case>.npz`` beside this file, so
that the tests need nothing outside the repository.  The inputs are regenerated from the seeded synthesiser at test time; the
SHA-256 of the inputs is stored with every case so that a drifted generator fails loudly instead of comparing apples
with pears.

What is kept of a long array (the outputs of a mastering case, its two FIRs, the two preview pieces), all in float64:
the values on ``kept_index`` (both edges and a fixed, seeded sample of the middle: every value of an array of up to
2 * EDGE + SAMPLE), the sums of every BLOCK consecutive values, its shape and its largest magnitude.  ``assert_matches``
holds an array to that: the kept values to the test's tolerance, every block sum to BLOCK times it -- so every value of
the array is covered, and no file grows with the length of a case.  The level-correction coefficients are kept whole.
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURES = os.path.join(HERE, "reference_cases")   # one .npz per case (or group of small cases)
EDGE, SAMPLE, BLOCK = 1024, 4096, 64
SAMPLE_SEED = 20241016

# ---- tests/test_oracle_vs_reference.py -------------------------------------------------------------------------------
PAIR_CASES = {
    "cd_rate": dict(pair=dict(seconds=2.4, sample_rate=44100, pair=7, reference_seconds=2.0),
                    config=dict(max_piece_size=0.5)),
    "hot_two_rounds": dict(pair=dict(seconds=3.0, sample_rate=22050, pair=8, reference_gain=6.0),
                           config=dict(internal_sample_rate=22050, fft_size=1024, max_piece_size=0.7,
                                       rms_correction_steps=2)),
    "quiet_reference_custom_limiter": dict(
        pair=dict(seconds=1.6, sample_rate=48000, pair=9, reference_gain=0.5),
        config=dict(internal_sample_rate=48000, fft_size=2048, max_piece_size=0.4,
                    limiter=dict(attack=2.0, hold=1.5, release=800.0))),
}
for _fft in (8, 16, 32):
    PAIR_CASES[f"small_fft_{_fft}"] = dict(pair=dict(seconds=3.0, sample_rate=8000, pair=1),
                                           config=dict(internal_sample_rate=8000, fft_size=_fft, max_piece_size=1.0))
for _fft in (32768, 65536):
    PAIR_CASES[f"large_fft_{_fft}"] = dict(pair=dict(seconds=2.0, sample_rate=192000, pair=14, reference_seconds=1.7),
                                           config=dict(internal_sample_rate=192000, fft_size=_fft, max_piece_size=0.6))
PAIR_CASES["twenty_correction_steps"] = dict(pair=dict(seconds=3.0, sample_rate=8000, pair=2),
                                             config=dict(internal_sample_rate=8000, fft_size=256, max_piece_size=1.0,
                                                         rms_correction_steps=20))

# values that pass defaults.py's asserts and then fail inside the reference
FAILING = {"fft_size_2": dict(fft_size=2), "fft_size_4": dict(fft_size=4), "hold_0.25": dict(limiter=dict(hold=0.25)),
           "hold_0.05": dict(limiter=dict(hold=0.05))}
FAILING_PAIR = dict(seconds=3.0, sample_rate=8000, pair=1, reference_gain=3.0)
FAILING_BASE = dict(internal_sample_rate=8000, fft_size=256, max_piece_size=1.0)

# ---- tests/test_host_vs_reference.py ---------------------------------------------------------------------------------
CHECK_CASES = ["stereo", "mono", "clipping", "limited", "three_channels", "too_short", "too_long"]
CHECK_RATE = 8000
CHECK_CONFIG = dict(internal_sample_rate=CHECK_RATE, fft_size=256, max_length=20)
PREVIEW_SECONDS = [2.0, 11.0, 23.0]
PREVIEW_RATE = 8000
PREVIEW_CONFIG = dict(internal_sample_rate=PREVIEW_RATE, fft_size=256, preview_size=6, preview_analysis_step=2)


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def pair_inputs(name):
    from matchering_amd.synth import make_pair

    return make_pair(**PAIR_CASES[name]["pair"])


def failing_inputs():
    from matchering_amd.synth import make_pair

    return make_pair(**FAILING_PAIR)


def failing_config(name):
    kw = dict(FAILING_BASE)
    kw.update(FAILING[name])
    return kw


def check_input(case):
    """(array, name) handed to checker.check for one case."""
    from matchering_amd.synth import synth

    x = 0.4 * synth(3.0, CHECK_RATE, 3)
    name = "target"
    if case == "mono":
        x = x[:, :1]
        name = "reference"
    elif case == "clipping":
        x = np.clip(4.0 * x, -1.0, 1.0)
    elif case == "limited":
        x = np.clip(4.0 * x, -0.9, 0.9)
    elif case == "three_channels":
        x = np.concatenate((x, x[:, :1]), axis=1)
    elif case == "too_short":
        x = x[:100]
    elif case == "too_long":
        x = np.tile(x, (8, 1))
    return x, name


def preview_inputs(seconds):
    from matchering_amd.synth import synth

    rng = np.random.RandomState(int(seconds))
    target = 1.3 * synth(seconds, PREVIEW_RATE, 5)
    result = synth(seconds, PREVIEW_RATE, 6) * (0.3 + rng.rand(1)[0] * np.hanning(int(seconds * PREVIEW_RATE))[:, None])
    return target, result


def load():
    """Every fixture as {"<file stem>/<key>": array}."""
    out = {}
    for name in sorted(os.listdir(FIXTURES)):
        if name.endswith(".npz"):
            z = np.load(os.path.join(FIXTURES, name), allow_pickle=False)
            out.update({name[:-4] + "/" + k: z[k] for k in z.files})
    return out


def kept_index(n):
    """Positions kept value for value: both edges (filter edge effects live there) and a fixed, seeded sample of the
    middle; all of them where the array is short."""
    edge = min(EDGE, n // 3)
    middle = np.arange(edge, n - edge)
    if middle.size > SAMPLE:
        middle = np.sort(np.random.default_rng([SAMPLE_SEED, n]).choice(middle, SAMPLE, replace=False))
    return np.unique(np.concatenate((np.arange(edge), middle, np.arange(n - edge, n))))


def block_sums(x):
    x = np.asarray(x, dtype=np.float64)
    return np.add.reduceat(x, np.arange(0, x.shape[0], BLOCK), axis=0)


def freeze(prefix, x):
    """What the fixture keeps of a long array (module docstring), as {key: array}."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    return {prefix + "_shape": np.array(x.shape), prefix + "_max_abs": np.array(np.abs(x).max()),
            prefix + "_kept": x[kept_index(x.shape[0])], prefix + "_blocks": block_sums(x)}


def assert_matches(mine, frozen, prefix, tol):
    """``max |mine - frozen array| <= tol`` on the kept positions, and every block sum within BLOCK * tol."""
    mine = np.asarray(mine, dtype=np.float64)
    assert mine.shape == tuple(frozen[prefix + "_shape"]), (prefix, mine.shape)
    assert np.abs(mine[kept_index(mine.shape[0])] - frozen[prefix + "_kept"]).max() <= tol, prefix
    assert np.abs(block_sums(mine) - frozen[prefix + "_blocks"]).max() <= BLOCK * tol, prefix


def codes(lines):
    return [line.split(":")[0].strip() for line in lines]


def run_check(module, package, array, rate, name, cfg):
    """checker.check of either package -> (result or None, log codes, error code or None)."""
    lines = []
    package.log(warning_handler=lines.append, info_handler=lines.append, show_codes=True)
    try:
        try:
            got = module.check(np.array(array), rate, package.Config(**cfg), name)
            err = None
        except Exception as exc:                 # ModuleError of either package
            got, err = None, str(exc).split(":")[0].strip()
    finally:
        package.log()
    return got, codes(lines), err


def run_preview(module, package, target, result, cfg, patch):
    """create_preview of either package -> {file name: array it would have saved}; ``patch(module, name, value)``
    replaces the module's ``save``."""
    pieces = {}
    patch(module, "save", lambda file, array, rate_, subtype, name="": pieces.__setitem__(file, np.array(array)))
    module.create_preview(np.array(target), np.array(result), package.Config(**cfg),
                          package.pcm16("target.wav"), package.pcm16("result.wav"))
    return pieces


def main():
    import importlib

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, HERE)
    import reference_runner as rr

    assert rr.reference_available(), "the reference tree is needed to freeze its answers"
    out = {}
    for name in sorted(PAIR_CASES):
        target, reference = pair_inputs(name)
        outs, inter = rr.run_reference(target, reference, PAIR_CASES[name]["config"])
        out[f"{name}/input_sha256"] = np.array(digest(target, reference))
        for k, o in enumerate(outs):
            out.update(freeze(f"{name}/out{k}", o))
        for key in ("fir_mid", "fir_side"):
            out.update(freeze(f"{name}/{key}", inter[key]))
        for key in ("rms_coefficient", "final_amplitude_coefficient", "correction_coefficients"):
            out[f"{name}/{key}"] = np.asarray(inter[key], dtype=np.float64)
    target, reference = failing_inputs()
    out["failing/input_sha256"] = np.array(digest(target, reference))
    for name in sorted(FAILING):
        try:
            rr.run_reference(target, reference, failing_config(name), capture=False)
            raised = ""
        except Exception as exc:                     # noqa: BLE001 -- what the reference raises is the answer
            raised = type(exc).__name__
        out[f"failing/{name}"] = np.array(raised)

    ref = rr.load_reference()
    ref_checker = importlib.import_module("matchering.checker")
    for case in CHECK_CASES:
        x, name = check_input(case)
        got, got_codes, err = run_check(ref_checker, ref, x, CHECK_RATE, name, CHECK_CONFIG)
        out[f"check/{case}/input_sha256"] = np.array(digest(x))
        out[f"check/{case}/codes"] = np.array(json.dumps(got_codes))
        out[f"check/{case}/error"] = np.array(json.dumps(err))
        if got is not None:
            out[f"check/{case}/rate"] = np.array(got[1])
            out[f"check/{case}/array_sha256"] = np.array(digest(np.asarray(got[0], np.float64)))
    ref_preview = importlib.import_module("matchering.preview_creator")
    for seconds in PREVIEW_SECONDS:
        target, result = preview_inputs(seconds)
        pieces = run_preview(ref_preview, ref, target, result, PREVIEW_CONFIG, setattr)
        out[f"preview/{seconds}/input_sha256"] = np.array(digest(target, result))
        for key, value in pieces.items():
            out.update(freeze(f"preview/{seconds}/{key}", value))
    files = {}
    for key, value in out.items():                   # "<file stem>/<key in the file>"
        stem, rest = key.split("/", 1)
        files.setdefault(stem, {})[rest] = value
    os.makedirs(FIXTURES, exist_ok=True)
    for stem, arrays in files.items():
        path = os.path.join(FIXTURES, stem + ".npz")
        np.savez_compressed(path, **arrays)
        print(f"{path}: {len(arrays)} arrays, {os.path.getsize(path) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
