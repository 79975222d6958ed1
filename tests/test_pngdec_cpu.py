"""CPU: the definition of the device PNG decoder (tests/pngdec_model.py) against Pillow, byte for byte; its emulation of the device's
scheme (window ring, literal batches, lane-wise match copies, chunked Adler-32, unfilter wavefront) against its straightforward
decode; host/pngdec.py::probe on files of and outside the supported set; the status bits of malformed streams; a seeded corpus of
mutated streams; and the ABI of the new entry points."""
import ctypes
import io
import re
from pathlib import Path

import numpy as np
import pytest
from PIL import Image

import pngdec_cases as cases
import pngdec_model as model
from diffuman4d_amd.host import pngdec

ROOT = Path(__file__).resolve().parent.parent


def pillow(data):
    return np.asarray(Image.open(io.BytesIO(data)))


def test_model_equals_pillow_on_every_supported_case():
    for name, data in cases.supported():
        want = pillow(data)
        got, status = model.decode_status(data)
        assert status == 0, name
        assert got.shape == want.shape and np.array_equal(got, want), name


def test_device_scheme_emulation_equals_the_plain_decode():
    for name, data in cases.supported():
        plain, s0 = model.decode_status(data)
        dev, s1 = model.decode_status(data, scheme="device")
        assert s0 == s1 == 0, name
        assert np.array_equal(plain, dev), name


def test_emulation_flushes_halves_of_the_ring():
    data = dict(cases.supported())["260x520-noise"]
    plan = model.probe(data)
    sink = model.DeviceSink(plan["h"] * (1 + plan["w"]))
    stream = b"".join(data[s:e] for s, e in plan["idat"])
    assert model.inflate(stream, sink.expect, sink) == 0
    assert sink.flushes == 5 and sink.pos == 260 * 521  # four whole halves (the ring wraps twice) and the tail


def test_probe_takes_exactly_the_supported_set():
    for name, data in cases.supported():
        p = pngdec.probe(data)
        want = pillow(data)
        assert p is not None, name
        assert (p.h, p.w) == want.shape[:2] and p.channels == (1 if want.ndim == 2 else want.shape[2]), name
        assert p.mode == Image.open(io.BytesIO(data)).mode, name
        m = model.probe(data)
        assert [tuple(r) for r in m["idat"]] == list(p.idat) and b"".join(data[s:e] for s, e in p.idat) == cases.idat_stream(data), name
    for name, data in cases.unsupported():
        assert pngdec.probe(data) is None, name
        assert model.probe(data) is None, name
    for name, data, _ in cases.malformed():
        assert pngdec.probe(data) is not None, name


def test_malformed_files_give_the_intended_status_bits():
    seen = 0
    for name, data, bit in cases.malformed():
        _, status = model.decode_status(data)
        assert status & bit, f"{name}: status {status}"
        assert model.decode_status(data, scheme="device")[1] == status, name
        seen |= bit
    assert seen == 127  # one file per status bit at least


def test_what_pillow_does_with_the_malformed_files():
    """Pillow raises for a bad checksum, a truncated stream and a bad filter byte; a stream that is merely too short or too long gives
    an image, which is what the caller gets through the Pillow route."""
    by_name = {name: data for name, data, _ in cases.malformed()}
    for name in ("adler", "truncated-stream", "filter-5"):
        with pytest.raises(Exception):
            pillow(by_name[name])
    for name in ("stream-too-short", "stream-too-long"):
        assert pillow(by_name[name]).shape == (40, 33)


def test_mutated_streams_never_pass_with_other_pixels():
    passed = flagged = 0
    for name, data in cases.mutations():
        assert pngdec.probe(data) is not None, name
        got, status = model.decode_status(data)
        try:
            want = pillow(data)
        except Exception:
            want = None
        if want is None:
            assert status != 0, f"{name}: Pillow raises, the model accepts"
        if status == 0:
            assert want is not None and np.array_equal(got, want), name
            passed += 1
        else:
            flagged += 1
    assert flagged > 20  # the corpus does exercise the error paths


def test_symbols_signatures_and_constants():
    from diffuman4d_amd import build
    from diffuman4d_amd.host import lib as L
    assert "pngdec.hip" in build.SOURCES
    lib = ctypes.CDLL(str(build.build(force=False, verbose=False)))
    for name in ("dm4d_png_decode_u8", "dm4d_png_decode_ws_bytes", "dm4d_vhull_pack_masks_u8"):
        assert hasattr(lib, name) and name in L.SIGNATURES, name
    header = (ROOT / "include" / "dm4d.h").read_text()
    assert len(L.SIGNATURES["dm4d_png_decode_u8"][1]) == 11 and re.search(r"int dm4d_png_decode_u8\(void\* stream, const void\* streams, "
                                                                         r"int64_t streams_bytes", header)
    found = dict(re.findall(r"^#define DM4D_(PNGDEC_\w+)[ \t]+(\S[^\n]*)$", header, flags=re.M))
    assert set(found) == {"PNGDEC_FIELDS", "PNGDEC_RING_BYTES", "PNGDEC_MAX_ROW_BYTES", "PNGDEC_MAX_STREAM_BYTES", "PNGDEC_ST_HEADER",
                          "PNGDEC_ST_BLOCK", "PNGDEC_ST_CODE", "PNGDEC_ST_DISTANCE", "PNGDEC_ST_END", "PNGDEC_ST_ADLER", "PNGDEC_ST_FILTER"}
    for name, text in found.items():
        m = re.fullmatch(r"\((\d+) << (\d+)\)|(\d+)", text.strip())
        value = int(m.group(1)) << int(m.group(2)) if m.group(1) else int(m.group(3))
        assert getattr(L, name) == value, name
    assert (pngdec.MAX_ROW_BYTES, pngdec.MAX_STREAM_BYTES) == (L.PNGDEC_MAX_ROW_BYTES, L.PNGDEC_MAX_STREAM_BYTES)
    assert (model.RING, model.MAX_ROW_BYTES, model.MAX_STREAM_BYTES) == (L.PNGDEC_RING_BYTES, L.PNGDEC_MAX_ROW_BYTES, L.PNGDEC_MAX_STREAM_BYTES)
    assert (model.ST_HEADER, model.ST_BLOCK, model.ST_CODE, model.ST_DISTANCE, model.ST_END, model.ST_ADLER, model.ST_FILTER) == (
        L.PNGDEC_ST_HEADER, L.PNGDEC_ST_BLOCK, L.PNGDEC_ST_CODE, L.PNGDEC_ST_DISTANCE, L.PNGDEC_ST_END, L.PNGDEC_ST_ADLER, L.PNGDEC_ST_FILTER)
