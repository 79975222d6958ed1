"""The images that tests/test_png_cpu.py (the model against independent decoders) and tests/test_png_gpu.py (the device against the
model) share: name -> uint8 [h, w] (L) or [h, w, 4] (RGBA).  Deterministic."""
import numpy as np

import png_model as M

RUNS = (2, 3, 258, 259, 260, 261, 516, 517)
# counts of 15 residual values: with the row's filter byte (1) and the end-of-block symbol (1) the stripe's histogram is the Fibonacci
# sequence over 17 symbols, whose Huffman tree is a chain of depth 16; 4178 bytes in all
FIB = (2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597)


def from_residuals(res) -> np.ndarray:
    """A one-row L image whose filtered bytes (row 0: Paeth against zeros = Sub) are `res`."""
    return (np.cumsum(np.asarray(res, dtype=np.int64)) & 255).astype(np.uint8)[None, :]


def run_image(n: int) -> np.ndarray:
    return from_residuals([9, 200] + [77] * n + [31, 5])


def fibonacci_image() -> np.ndarray:
    """Residuals with a Fibonacci-shaped histogram, shuffled; runs of four or more equal bytes (which would become matches and leave
    the histogram) are broken up by further random swaps."""
    rng = np.random.default_rng(5)
    res = rng.permutation(np.concatenate([np.full(c, 10 + 3 * k) for k, c in enumerate(FIB)]))
    while True:
        long = np.flatnonzero((res[3:] == res[2:-1]) & (res[3:] == res[1:-2]) & (res[3:] == res[:-3])) + 3
        if long.size == 0:
            return from_residuals(res)
        for i in long:
            j = int(rng.integers(res.size))
            res[i], res[j] = res[j], res[i]


def striped(kind: str) -> np.ndarray:
    """Three stripes, the last one partial, with a constant band across the first stripe boundary."""
    ch, w = (1, 300) if kind == "L" else (4, 300)
    rows = M.stripe_rows(1, w, ch)
    h = 2 * rows + rows // 2 + 1
    img = np.random.default_rng(11).integers(0, 256, (h, w) + ((4,) if ch == 4 else ()), dtype=np.uint8)
    img[rows - 5: rows + 5] = 123
    assert M.n_stripes(h, w, ch) == 3 and h % rows != 0
    return img


def cases() -> dict:
    rng = np.random.default_rng(2024)
    out = {}
    for kind, tail in (("L", ()), ("RGBA", (4,))):
        for h, w in ((1, 1), (1, 3), (300, 1), (1, 300), (17, 19), (5, 15), (5, 16), (5, 17)):
            out[f"{kind}_{h}x{w}"] = rng.integers(0, 256, (h, w) + tail, dtype=np.uint8)
        out[f"{kind}_constant"] = np.full((64, 64) + tail, 201, dtype=np.uint8)
        out[f"{kind}_noise"] = rng.integers(0, 256, (64, 64) + tail, dtype=np.uint8)
        out[f"{kind}_striped"] = striped(kind)
    for n in RUNS:
        out[f"L_run{n}"] = run_image(n)
    out["L_fibonacci"] = fibonacci_image()
    # the widest rows: one row per stripe (R >= the stripe size); an RGBA stripe is 65537 bytes, one more than 16 bits count
    for kind, tail, h in (("L", (), 3), ("RGBA", (4,), 2)):
        wide = np.broadcast_to((np.arange(M.MAX_SIDE) // 97).astype(np.uint8).reshape((1, -1) + (1,) * len(tail)), (h, M.MAX_SIDE) + tail).copy()
        wide[:, 5000:7000] = rng.integers(0, 256, (h, 2000) + tail, dtype=np.uint8)
        out[f"{kind}_widest"] = wide
    out["L_onerun"] = from_residuals([4] * 600)  # with the filter byte, the whole stripe is one run of 601 bytes
    return out


def result_like(h: int = 256, w: int = 320):
    """A result-like pair: (RGB uint8 [h, w, 3]: a smooth foreground on white through a JPEG round trip, mask uint8 [h, w]: a blurred
    ellipse)."""
    import io

    from PIL import Image, ImageFilter
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    inside = ((x - w / 2) / (0.33 * w)) ** 2 + ((y - h / 2) / (0.42 * h)) ** 2 <= 1.0
    fg = np.stack([128 + 90 * np.sin(x / 23.0 + y / 41.0), 120 + 80 * np.cos(y / 17.0), 110 + 70 * np.sin((x + y) / 29.0)], axis=-1)
    rgb = np.where(inside[..., None], fg, 255.0).clip(0, 255).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="JPEG", quality=90)
    rgb = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))
    mask = np.asarray(Image.fromarray((inside * 255).astype(np.uint8)).filter(ImageFilter.GaussianBlur(3)))
    return rgb, mask
