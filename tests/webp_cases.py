"""The images that tests/test_webp_cpu.py (the model against Pillow's decoder) and tests/test_webp_gpu.py (the device against the model)
share: name -> uint8 [h, w, 3].  Deterministic."""
import numpy as np

import skel_model
import webp_model as M

# counts of 17 green values: the Huffman tree of a Fibonacci sequence is a chain, here of depth 16; 4180 pixels in all
FIB = (1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597)


def fibonacci_image() -> np.ndarray:
    """One row of literals only: the green values have a Fibonacci-shaped histogram, and red changes from every pixel to the next (and
    the image has one row), so no pixel equals the one before it."""
    rng = np.random.default_rng(5)
    green = rng.permutation(np.concatenate([np.full(c, 10 + 3 * k) for k, c in enumerate(FIB)]))
    img = np.zeros((1, green.size, 3), dtype=np.uint8)
    img[0, :, 1] = green
    img[0, :, 0] = np.arange(green.size) % 7
    img[0, :, 2] = 9
    return img


def deep_literals_image() -> np.ndarray:
    """Literals of the most bits: 16 colours whose counts are FIB[:16] in every row, each colour (11 + 3 s, 10 + 3 s, 12 + 3 s), so the
    red, green and blue codes are all chains of depth 15 and the rarest colours cost 45 bits, the format's maximum for a token.  The
    colours sorted by count, most frequent first, fill the even places of a row and then the odd ones, so no two neighbours are equal;
    row r is that sequence rolled by r, so no pixel equals the one above it.  2583 pixels a row, two stripes."""
    order = np.concatenate([np.full(c, s) for s, c in sorted(enumerate(FIB[:16]), key=lambda sc: -sc[1])])
    seq = np.empty(order.size, dtype=np.int64)
    seq[np.concatenate([np.arange(0, order.size, 2), np.arange(1, order.size, 2)])] = order
    assert not (seq[1:] == seq[:-1]).any()
    row = np.stack([11 + 3 * seq, 10 + 3 * seq, 12 + 3 * seq], axis=1).astype(np.uint8)
    return np.stack([np.roll(row, r, axis=0) for r in range(4)])


def long_run_image() -> np.ndarray:
    """100 pixels a row: rows 75 .. 139 are one colour, a run of kind U of 6400 pixels from pixel 7600 that crosses the stripe boundary at
    8192; noise elsewhere."""
    img = np.random.default_rng(6).integers(0, 256, (150, 100, 3), dtype=np.uint8)
    img[75:140] = (9, 200, 31)
    return img


def striped_image() -> np.ndarray:
    """Three stripes, the last one partial and the height no multiple of a stripe: noise, flat bands and columns."""
    img = np.random.default_rng(11).integers(0, 256, (211, 97, 3), dtype=np.uint8)
    img[40:90, 10:80] = (0, 0, 0)
    img[150:200, ::3] = (255, 0, 7)
    assert M.n_stripes(211, 97) == 3 and (211 * 97) % M.STRIPE_PIXELS != 0
    return img


def skeleton_map() -> np.ndarray:
    """A map as the skeleton stage draws it: coloured limbs and joints on black, reduced by Pillow to 48 x 64."""
    pts = [(60, 30), (128, 60), (128, 150), (90, 230), (170, 232), (40, 120), (215, 110)]
    links = [(0, 1), (1, 2), (2, 3), (2, 4), (1, 5), (1, 6)]
    calls = [dict(type="line", p1=pts[a], p2=pts[b], thickness=9, color=(40 * k + 15, 255 - 30 * k, 90 + 20 * k)) for k, (a, b) in enumerate(links)]
    calls += [dict(type="circle", center=p, radius=7, color=(255, 30 * k, 200 - 25 * k)) for k, p in enumerate(pts)]
    return skel_model.expected_map(calls, (256, 256), (48, 64))


def cases() -> dict:
    rng = np.random.default_rng(2025)
    out = {}
    for h, w in ((1, 1), (1, 2), (2, 1)):
        out[f"noise_{h}x{w}"] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    out["constant"] = np.full((64, 64, 3), (201, 7, 44), dtype=np.uint8)
    two = np.zeros((40, 30, 3), dtype=np.uint8)
    two[rng.random((40, 30)) < 0.5] = (255, 128, 3)
    out["two_colours"] = two
    out["column"] = np.repeat(rng.integers(0, 4, (300, 1, 1), dtype=np.uint8) * 60, 3, axis=2)  # width 1: the pixel above is the pixel before
    out["noise_17x33"] = rng.integers(0, 256, (17, 33, 3), dtype=np.uint8)
    out["long_run"] = long_run_image()
    out["striped"] = striped_image()
    # 2 x 8192 + 1 pixels of one colour: the last stripe is one reference of length 1, a few bits that share a byte with the stripe before
    out["one_pixel_stripe"] = np.full((5, 3277, 3), (0, 0, 0), dtype=np.uint8)
    out["fibonacci"] = fibonacci_image()
    out["deep_literals"] = deep_literals_image()
    widest = np.repeat((np.arange(M.MAX_SIDE) // 97).astype(np.uint8)[None, :, None], 3, axis=2)
    widest[0, 5000:7000] = rng.integers(0, 256, (2000, 3), dtype=np.uint8)
    out["widest"] = widest
    out["skeleton_map"] = skeleton_map()
    return out
