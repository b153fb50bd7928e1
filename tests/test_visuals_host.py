"""The visuals' device-free part on a machine without a GPU: mgx_spectrogram_plan against the oracle's hops and columns
and every one of its refusals by name, log_bands' properties, and pictures through a minimal PNG reader."""
import ctypes
import struct
import zlib

import numpy as np
import pytest

import visuals_oracle as oracle
from matchering_amd import _native, visuals

INT_P = ctypes.POINTER(ctypes.c_int32)


def plan_call(n, log2_fft=12, hop=1024, columns=0, channels=0, edges=None, spec_null=False, edges_null=False):
    lib = _native.library()
    edges = np.arange((1 << log2_fft) // 2 + 2, dtype=np.int32) if edges is None else np.asarray(edges, dtype=np.int32)
    spec = _native.MgxSpectrogramSpec(log2_fft, hop, columns, channels, edges.size - 1)
    hops, width = ctypes.c_int64(-7), ctypes.c_int32(-7)
    rc = lib.mgx_spectrogram_plan(n, None if spec_null else ctypes.byref(spec), None if edges_null else edges.ctypes.data_as(INT_P),
                                  ctypes.byref(hops), ctypes.byref(width))
    return rc, hops.value, width.value, lib.mgx_last_error().decode()


@pytest.mark.parametrize("n, hop, columns", [
    (1, 1024, 0), (1, 1, 1), (1024, 1024, 0), (1025, 1024, 0), (1025, 1024, 2), (2047, 1024, 1), (2048, 1024, 2), (4097, 1024, 0),
    (300, 1, 0), (300, 1, 300), (300, 1, 299), (300, 1, 7), (10000, 1000, 10), (10001, 1000, 11), (10001, 1000, 3),
    (21168000, 1024, 1024), (21168000, 1024, 1), (21168000, 4096, 0), (500000000, 4096, 2048), (40000, 4096, 0)])
def test_plan_gives_the_oracles_hops_and_columns(n, hop, columns):
    rc, hops, width, message = plan_call(n, 12, hop, columns)
    assert rc == 0, message
    assert (hops, width) == oracle.plan(n, hop, columns)
    assert hops == len(range(0, n, hop))                          # a hop per multiple of the hop below n


def test_plan_of_an_empty_track():
    assert plan_call(0, columns=0)[:3] == (0, 0, 0)
    assert plan_call(0, columns=9)[:3] == (0, 0, 0)               # (with no frames the columns are not looked at)


def test_plan_takes_null_outputs():
    lib = _native.library()
    edges = np.arange(130, dtype=np.int32)
    spec = _native.MgxSpectrogramSpec(8, 64, 0, 0, 129)
    assert lib.mgx_spectrogram_plan(1000, ctypes.byref(spec), edges.ctypes.data_as(INT_P), None, None) == 0


@pytest.mark.parametrize("kwargs, code, word, value", [
    (dict(spec_null=True), "ERR_ARGUMENT", "spec", None),
    (dict(edges_null=True), "ERR_ARGUMENT", "edges", None),
    (dict(n=-5), "ERR_ARGUMENT", "n_frames", "-5"),
    (dict(n=500000001), "ERR_UNSUPPORTED", "n_frames", "500000001"),
    (dict(log2_fft=7, edges=[0, 1]), "ERR_ARGUMENT", "log2_fft", "7"),
    (dict(log2_fft=15, edges=[0, 1]), "ERR_ARGUMENT", "log2_fft", "15"),
    (dict(hop=0), "ERR_ARGUMENT", "hop", "0"),
    (dict(hop=4097), "ERR_ARGUMENT", "hop", "4097"),
    (dict(channels=2), "ERR_ARGUMENT", "channels", "2"),
    (dict(channels=-1), "ERR_ARGUMENT", "channels", "-1"),
    (dict(edges=[0]), "ERR_ARGUMENT", "bands", "0"),
    (dict(edges=np.arange(2051)), "ERR_ARGUMENT", "bands", "2050"),
    (dict(edges=[-1, 4]), "ERR_ARGUMENT", "edges[0]", "-1"),
    (dict(edges=[0, 4, 4, 9]), "ERR_ARGUMENT", "edges[2]", "4"),
    (dict(edges=[0, 4, 3, 9]), "ERR_ARGUMENT", "edges[2]", "3"),
    (dict(edges=[0, 4, 2050]), "ERR_ARGUMENT", "edges[2]", "2050"),
    (dict(columns=-1), "ERR_ARGUMENT", "columns", "-1"),
    (dict(n=10000, columns=11), "ERR_ARGUMENT", "columns", "11"),
    (dict(n=400000000, hop=1), "ERR_UNSUPPORTED", "columns", "400000000"),
])
def test_plan_refusals_name_the_field_and_the_value(kwargs, code, word, value):
    given = dict(n=10000)
    given.update(kwargs)
    rc, hops, width, message = plan_call(**given)
    assert rc == getattr(_native, code), message
    assert message.startswith(word + ":"), message
    if value is not None:
        assert value in message, message
    assert (hops, width) == (-7, -7)                              # (a refusal writes nothing)


def test_plan_accepts_the_extremes():
    assert plan_call(10000, 8, 256, edges=[0, 129])[0] == 0       # hop == N, one band of every bin
    assert plan_call(10000, 14, 1, columns=1, edges=np.arange(8194))[0] == 0
    assert plan_call(10000, 12, 1024, edges=[2048, 2049])[0] == 0  # the Nyquist bin alone


def test_python_plan_raises_value_errors():
    assert visuals.plan(10000, 4096, 1000, 0) == (10, 10)
    with pytest.raises(ValueError, match="hop: 5000"):
        visuals.plan(10000, 4096, 5000)
    with pytest.raises(ValueError, match="power of two"):
        visuals.plan(10000, 4000, 1000)
    with pytest.raises(ValueError, match="channels"):
        visuals.plan(10000, 4096, 1000, channels="xy")


# ---- log_bands -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fft_size, rate, bands", [(4096, 44100, 96), (256, 44100, 96), (16384, 48000, 31), (1024, 8000, 1),
                                                   (4096, 44100, 3000), (512, 96000, 12)])
def test_log_bands_properties(fft_size, rate, bands):
    edges = visuals.log_bands(fft_size, rate, bands)
    assert edges.dtype == np.int32 and edges.ndim == 1
    assert 1 <= edges.size - 1 <= bands                           # however many bands strict ascent leaves
    assert np.all(np.diff(edges) >= 1)                            # strictly ascending
    assert edges[0] >= 0 and edges[-1] == fft_size // 2 + 1       # up to and including the Nyquist bin
    assert edges[0] == max(0, int(np.floor(20.0 * fft_size / rate + 0.5)))
    widths = np.diff(edges)
    first_wide = int(np.argmax(widths > 1)) if np.any(widths > 1) else widths.size
    assert np.all(widths[:first_wide] == 1)                       # the low bands are one bin wide
    if edges.size - 1 == bands and bands > 8:                     # where nothing was dropped the top follows the ratio
        ratio = (rate / 2.0 / 20.0) ** (1.0 / bands)
        assert abs(edges[-2] / edges[-3] - ratio) < 0.05 * ratio
    rc, _, _, message = plan_call(100000, fft_size.bit_length() - 1, fft_size // 4, edges=edges)
    assert rc == 0, message                                       # the library accepts the table


def test_log_bands_limits():
    assert visuals.log_bands(4096, 44100, 10, f_lo=100.0, f_hi=10000.0)[-1] == int(np.ceil(10000.0 * 4096 / 44100))
    with pytest.raises(ValueError):
        visuals.log_bands(4096, 44100, 0)
    with pytest.raises(ValueError):
        visuals.log_bands(4096, 44100, 8, f_lo=30000.0)
    assert np.array_equal(visuals.linear_bands(256), np.arange(130))


# ---- pictures --------------------------------------------------------------------------------------------------------------
def read_png(path):
    """A minimal reader: 8-bit greyscale, filter 0 on every row."""
    with open(path, "rb") as fh:
        data = fh.read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(data):
        size, kind = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + size]
        assert struct.unpack(">I", data[at + 8 + size:at + 12 + size])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF
        chunks.append((kind, body))
        at += 12 + size
    assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    columns, rows, depth, colour, compression, filtering, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, compression, filtering, interlace) == (8, 0, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), dtype=np.uint8).reshape(rows, columns + 1)
    assert not raw[:, 0].any()
    return raw[:, 1:]


def a_spectrogram():
    power = np.zeros((5, 2, 4), dtype=np.float32)
    power[:, 0, :] = 10.0 ** (np.array([0.0, -24.0, -40.0, -200.0]) / 10.0)       # band 0 loudest
    power[:, 1, :] = 10.0 ** (np.array([-96.0, -72.0, 6.0, -48.0]) / 10.0)
    power[3, 0, 3] = 1.0
    return visuals.Spectrogram(44100, 5000, 4096, 1000, 5, "lr", np.array([0, 1, 2, 4, 8], dtype=np.int32), power)


def test_image_puts_high_frequencies_at_the_top():
    s = a_spectrogram()
    image = s.image(top_db=0.0, range_db=96.0)
    assert image.dtype == np.uint8 and image.shape == (8, 5)      # the first channel above the second
    assert image[3, 0] == 255 and image[0, 0] == 0                # channel 0: band 0 at the bottom row of its half
    assert image[2, 0] == round(255 * 72 / 96) and image[1, 0] == round(255 * 56 / 96)
    assert image[0, 3] == 255                                     # the one loud top band, in its column
    assert image[7, 0] == 0 and image[6, 0] == round(255 * 24 / 96) and image[5, 0] == 255       # clipped at top_db
    assert np.array_equal(s.image(channel=1), image[4:])
    assert np.allclose(s.db(-120.0)[0, 0], [0.0, -24.0, -40.0, -120.0], atol=1e-5)
    assert np.allclose(s.band_hz[:, 0], np.array([0, 1, 2, 4]) * 44100 / 4096) and s.band_hz[-1, 1] == 8 * 44100 / 4096
    assert np.allclose(s.times_s, np.arange(5) * 1000 / 44100)
    assert s.as_dict()["power"][3][0][3] == 1.0 and s.as_dict()["edges"] == [0, 1, 2, 4, 8]


def test_save_png_round_trips(tmp_path):
    s = a_spectrogram()
    path = str(tmp_path / "picture.png")
    s.save_png(path, top_db=0.0, range_db=96.0)
    assert np.array_equal(read_png(path), s.image(0.0, 96.0))
    rng = np.random.default_rng(3)
    noise = rng.integers(0, 256, size=(37, 301), dtype=np.uint8)
    visuals.write_png(path, noise)
    assert np.array_equal(read_png(path), noise)
    with pytest.raises(ValueError):
        visuals.write_png(path, np.zeros((0, 4), dtype=np.uint8))


def test_overview_values():
    lo = np.array([[-0.5, -0.25], [0.0, 0.0]], dtype=np.float32)
    hi = np.array([[0.5, 0.25], [0.0, 0.0]], dtype=np.float32)
    o = visuals.Overview(44100, 5, lo, hi, np.array([[0.5, 0.125], [0.0, 0.0]]))
    assert o.columns == 2 and o.frames_per_column.tolist() == [2, 3]
    assert np.allclose(o.rms, [[0.5, 0.25], [0.0, 0.0]])
    assert np.allclose(o.rms_db(-100.0), [[20 * np.log10(0.5), 20 * np.log10(0.25)], [-100.0, -100.0]])
    assert o.as_dict()["lo"] == [[-0.5, -0.25], [0.0, 0.0]] and o.as_dict()["frames_per_column"] == [2, 3]


def test_request_from_json():
    r = visuals.VisualsRequest.from_json({"columns": 64, "bands": [0, 1, 5], "channels": "ms"})
    assert r.columns == 64 and r.channels == "ms" and r.edges(44100).tolist() == [0, 1, 5]
    assert visuals.VisualsRequest.from_json(True) == visuals.VisualsRequest()
    assert visuals.VisualsRequest(bands=None, fft_size=256).edges(44100).size == 130
