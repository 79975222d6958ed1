"""CPU: the definition the device JPEG decoder is held to.  tests/jpegdec_model.py equals Pillow on every file of the shared case
list; ``probe`` takes exactly the supported set; the emulated speculative entropy scheme reaches the serial decode at the device's
subsequence length, and the list holds files that need several propagation rounds and more than one tile; the IDCT's integer-width
statements hold against Python integers; malformed scans get their status."""
import functools
import io
import itertools

import numpy as np
import pytest
from PIL import Image

import jpegdec_cases as cases
import jpegdec_model as model
from diffuman4d_amd.host import jpegdec
from diffuman4d_amd.host import lib as L


def test_model_equals_pillow_on_every_case():
    assert len(cases.supported()) >= 40
    for name, data in cases.supported():
        want = np.asarray(Image.open(io.BytesIO(data)))
        got, status = model.decode_status(data)
        assert status == 0, name
        assert got.shape == want.shape and got.dtype == np.uint8, name
        assert np.array_equal(got, want), f"{name}: {int((got != want).sum())} bytes differ"


def test_case_list_covers_what_it_claims():
    names = [n for n, _ in cases.supported()]
    for h, w in cases.SIZES + [cases.BIG]:
        assert any(n.startswith(f"{h}x{w}-") for n in names)
    for token in ("-420-", "-422-", "-444-", "-gray-", "-noise-", "-smooth-", "-white-", "-q30-", "-q90-", "-q100-", "-opt", "-std", "-model-"):
        assert any(token in n for n in names), token
    plans = {n: jpegdec.probe(d) for n, d in cases.supported()}
    assert {(p.ncomp, p.hs, p.vs) for p in plans.values()} == {(1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)}
    # chroma planes of width <= 2 (replicated, not filtered) and wider ones, in both down-sampled layouts
    for hs_vs in ((2, 1), (2, 2)):
        widths = {-(-p.w // 2) <= 2 for p in plans.values() if (p.hs, p.vs) == hs_vs}
        assert widths == {True, False}


def test_probe_accepts_the_cases_and_refuses_the_rest():
    for name, data in cases.supported():
        p = jpegdec.probe(data)
        with Image.open(io.BytesIO(data)) as im:
            assert p is not None and (p.h, p.w) == (im.height, im.width) and p.mode == im.mode, name
        assert len(p.tables) == L.JPEGDEC_TABLE_BYTES
    for name, data in cases.unsupported():
        assert jpegdec.probe(data) is None, name
    good = cases.supported()[12][1]
    assert jpegdec.probe(good[:300]) is None and jpegdec.probe(b"") is None and jpegdec.probe(b"\xff\xd8\xff\xd9") is None
    # component ids 1 2 3 without a JFIF or Adobe marker are YCbCr to libjpeg; any other ids are not ours
    n = int.from_bytes(good[4:6], "big")
    bare = good[:2] + good[4 + n:]
    assert jpegdec.probe(bare) is not None
    sof = bare.index(b"\xff\xc0")
    rgb_ids = bytearray(bare)
    sos = bare.index(b"\xff\xda")
    for c, cid in enumerate(b"RGB"):
        rgb_ids[sof + 11 + 3 * c] = cid
        rgb_ids[sos + 5 + 2 * c] = cid
    assert jpegdec.probe(bytes(rgb_ids)) is None
    # a DRI of zero is no restart interval
    assert jpegdec.probe(good[:2] + b"\xff\xdd\x00\x04\x00\x00" + good[2:]) is not None
    assert jpegdec.probe(good[:2] + b"\xff\xdd\x00\x04\x00\x02" + good[2:]) is None


@functools.lru_cache(maxsize=None)
def speculative_runs():
    out = {}
    for name, data in cases.supported():
        plan = jpegdec.probe(data)
        counters = {}
        spec = model.speculative_coefficients(plan, data, L.JPEGDEC_SUB_BITS, L.JPEGDEC_TILE_LANES, counters)
        out[name] = (spec, model.serial_coefficients(plan, data), counters)
    return out


def test_speculative_scheme_reaches_the_serial_decode():
    assert (model.SUB_BITS, model.TILE_LANES) == (L.JPEGDEC_SUB_BITS, L.JPEGDEC_TILE_LANES)
    for name, ((coef, status), (want, want_status), _) in speculative_runs().items():
        assert status == want_status == 0, name
        assert np.array_equal(coef, want), name


def test_case_list_needs_propagation_rounds_and_more_than_one_tile():
    counters = [c for _, _, c in speculative_runs().values()]
    assert max(c["rounds"] for c in counters) >= 2
    assert sum(c["rounds"] >= 2 for c in counters) >= 5
    assert max(c["tiles"] for c in counters) >= 2
    assert any(c["tiles"] >= 2 and c["rounds"] >= 2 for c in counters)  # rounds in a tile that starts from a carried state


def test_speculative_scheme_at_other_subsequence_lengths():
    """The fixed point does not depend on where the cuts fall: short subsequences, tiles of few lanes."""
    for name, data in cases.supported()[12:16]:
        plan = jpegdec.probe(data)
        want = model.serial_coefficients(plan, data)
        for sub_bits, lanes in ((32, 4), (64, 256), (96, 7)):
            got = model.speculative_coefficients(plan, data, sub_bits, lanes)
            assert got[1] == want[1] and np.array_equal(got[0], want[0]), (name, sub_bits, lanes)


def test_idct_pass_one_fits_32_bits_for_coefficients_in_range():
    """Dequantised coefficients in [-8192, 8191]: every pass-1 sum plus its rounding constant stays below 2^30 in magnitude, so 32-bit
    arithmetic (wrapping or not) gives the exact value.  A sum is linear in the inputs, so its extremes over the box are at corners:
    all 2^8 patterns of the extreme values."""
    half = 1 << (model.CONST_BITS - model.PASS1_BITS - 1)
    worst = 0
    for corner in itertools.product((-8192, 8191), repeat=8):
        sums = model._idct_sums(np.array(corner, dtype=object))
        worst = max(worst, max(abs(int(v) + half) for v in sums))
    assert worst < 1 << 30


def test_idct_pass_two_may_wrap():
    """Only bits 18 .. 27 of a pass-2 sum survive `>> 18 & 1023`, so arithmetic modulo 2^32 with a logical shift gives the same sample
    whatever the int workspace holds -- extreme and random rows against Python integers."""
    rng = np.random.default_rng(0)
    rows = [list(c) for c in itertools.product((-(1 << 31), (1 << 31) - 1), repeat=8)][::5]
    rows += rng.integers(-(1 << 31), 1 << 31, (200, 8)).tolist() + rng.integers(-(1 << 19), 1 << 19, (200, 8)).tolist()
    shift = model.CONST_BITS + model.PASS1_BITS + 3
    for row in rows:
        sums = [int(v) for v in model._idct_sums(np.array(row, dtype=object))]
        exact = [((v + (1 << (shift - 1))) >> shift) & 1023 for v in sums]
        wrapped = [((((v & 0xFFFFFFFF) + (1 << (shift - 1))) & 0xFFFFFFFF) >> shift) & 1023 for v in sums]
        assert exact == wrapped
    lim = model.range_limit(np.arange(1024))
    assert lim[0] == 128 and lim[127] == 255 and lim[128] == 255 and lim[511] == 255 and lim[512] == 0 and lim[895] == 0 and lim[896] == 0
    assert lim[1023] == 127


def test_status_rules():
    (_, cut), (_, flipped), (_, rng_file) = cases.malformed()
    for data in (cut, flipped, rng_file):
        assert jpegdec.probe(data) is not None
    assert model.decode_status(cut)[1] & model.ST_END
    assert model.decode_status(flipped)[1] & model.ST_BAD_CODE
    assert model.decode_status(rng_file)[1] == model.ST_RANGE
    for data in (cut, flipped):  # the speculative scheme reports the same status
        plan = jpegdec.probe(data)
        assert model.speculative_coefficients(plan, data)[1] == model.serial_coefficients(plan, data)[1] != 0
    # data left over: a whole extra byte after the last block's padding
    good = cases.supported()[12][1]
    plan = jpegdec.probe(good)
    longer = good[:plan.scan[1]] + b"\x55" + good[plan.scan[1]:]
    assert jpegdec.probe(longer) is not None and model.decode_status(longer)[1] & model.ST_END
    assert (model.ST_BAD_CODE, model.ST_ZIGZAG, model.ST_END, model.ST_RANGE) == (
        L.JPEGDEC_ST_BAD_CODE, L.JPEGDEC_ST_ZIGZAG, L.JPEGDEC_ST_END, L.JPEGDEC_ST_RANGE)


def test_zigzag_index_past_63_is_a_status():
    """A block rebuilt so that a run carries the index to 64: DC, then ZRL x 3 (k = 49), then run 15 / size 1 (k = 64)."""
    from diffuman4d_amd.host.jpeg import AC_LUMA, DC_LUMA
    from jpeg_model import _Bits, huff_codes
    base = cases.save(cases.content("white", 8, 8, 0), "gray", 90, False)
    plan = jpegdec.probe(base)
    dc, ac = huff_codes(DC_LUMA), huff_codes(AC_LUMA)
    bw = _Bits()
    bw.put(*dc[0])
    for _ in range(3):
        bw.put(*ac[0xF0])
    bw.put(*ac[0xF1])
    bw.put(1, 1)
    bw.flush()
    data = base[:plan.scan[0]] + bytes(bw.out) + base[plan.scan[1]:]
    assert model.decode_status(data)[1] & model.ST_ZIGZAG


def test_no_cpu_path():
    with pytest.raises(L.Dm4dError, match="HIP device"):
        jpegdec.decode_jpeg_batch([cases.supported()[0][1]], "cpu")


def test_device_decode_is_passed_down_only_when_asked_for(tmp_path, monkeypatch):
    """diffuman4d_to_nerfstudio and tools/preprocess.py hand `device_decode` to remove_background; left off, the call is the one it was."""
    import sys
    from pathlib import Path
    from diffuman4d_amd.host import nerfstudio
    seen = []
    monkeypatch.setattr(nerfstudio, "remove_background", lambda **kw: seen.append(kw) or {})
    monkeypatch.setattr(nerfstudio, "write_nerfstudio_transforms", lambda *a: None)
    monkeypatch.setattr(nerfstudio.shutil, "copy", lambda *a: None)
    nerfstudio.diffuman4d_to_nerfstudio("data", "res", matting_model=lambda x: x)
    nerfstudio.diffuman4d_to_nerfstudio("data", "res", matting_model=lambda x: x, device_decode=True)
    assert "device_decode" not in seen[0] and seen[1]["device_decode"] is True
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
    try:
        import preprocess
    finally:
        sys.path.pop(0)
    calls = []
    monkeypatch.setitem(preprocess.STAGES, "remove_background", lambda *a, **kw: calls.append(kw) or {})
    preprocess.run(str(tmp_path), ["remove_background"], matting_model_dir="m")
    preprocess.run(str(tmp_path), ["remove_background"], matting_model_dir="m", device_decode=True)
    assert "device_decode" not in calls[0] and calls[1]["device_decode"] is True


def test_evaluator_refuses_device_decode_without_a_device():
    from diffuman4d_amd.host import metrics
    with pytest.raises(L.Dm4dError, match="HIP device"):
        metrics.ImageEvaluator("cpu", device_decode=True)
