"""The definition of raw-capture rectification (csrc/rectify.hip, diffuman4d_amd/host/rectify.py; DESIGN.md "Raw-capture rectification"),
in numpy on the CPU.  Modelled on the reference's ``calib_undist_image`` (scripts/download/extract_dnar_images.py:89-120) with COLMAP's
``UndistortImage`` for the undistort step and OpenCV's ``INTER_AREA`` for the resize; none of COLMAP, EasyVolcap and OpenCV is at hand,
so the distance to them is not measured.

``rectify`` is the definition: fp32, every operation rounded on its own, in the order written here; the device equals it byte for byte.
``reference64`` is the same geometry written independently in fp64 with whole intermediate images; it checks the definition.

An image goes through four steps:

  A. colour: byte b of RGB channel c becomes lut[c][b] = clamp(b*b*m[c,0] + b*m[c,1] + m[c,2], 0, 255), m = ccm[[2, 1, 0]] (the files hold
     the rows in B, G, R order), computed for the 256 bytes by torch CPU with the reference's own expression;
  B. undistort to the pinhole camera K_undist of size uw x uh, bilinear over the table values, black outside, truncated to uint8;
  C. area resize uw x uh -> rw x rh, separable, horizontal first and kept in fp32, rounded half to even at the end;
  D. crop [top:bottom, left:right].
"""
from __future__ import annotations

import numpy as np
import torch

F = np.float32
MAX_SCALE = 8


def colour_table(ccm) -> np.ndarray:
    """fp32 [3, 256]: the reference's ``calib_color`` (extract_dnar_images.py:90-100) applied by torch CPU to an image that holds every
    byte once in every channel."""
    img = torch.arange(256, dtype=torch.float32)[:, None, None].expand(256, 1, 3).contiguous()[None]
    sol = torch.from_numpy(np.array(ccm, dtype=np.float64)).float()[None][:, [2, 1, 0], :]
    X = torch.stack([img ** 2, img, torch.ones_like(img)], dim=-1)
    out = (X * sol[:, None, None, :, :]).sum(dim=-1)[0].clamp(0, 255)
    return np.ascontiguousarray(out[:, 0, :].numpy().T)


def area_taps(n_in: int, n_out: int):
    """Output i of an axis n_in -> n_out covers [i s, (i + 1) s), s = n_in / n_out -> (first source cell [n_out], tap count [n_out],
    weights fp32 [n_out, k]); a weight is fp32(overlap / s) with the overlap taken in exact integers and the quotient in fp64; taps
    past the count have weight 0.  s outside [1, MAX_SCALE] is a ValueError."""
    n_in, n_out = int(n_in), int(n_out)
    if n_out < 1 or not (n_out <= n_in <= MAX_SCALE * n_out):
        raise ValueError(f"area resize {n_in} -> {n_out}: the scale is outside 1..{MAX_SCALE}")
    first = [(i * n_in) // n_out for i in range(n_out)]
    last = [-((-(i + 1) * n_in) // n_out) for i in range(n_out)]  # one past the last cell
    k = max(e - f for f, e in zip(first, last))
    wts = np.zeros((n_out, k), dtype=F)
    for i, (f, e) in enumerate(zip(first, last)):
        for t, j in enumerate(range(f, e)):
            overlap = min((i + 1) * n_in, (j + 1) * n_out) - max(i * n_in, j * n_out)  # in units of 1 / n_out
            wts[i, t] = F(np.float64(overlap) / np.float64(n_in))
    return np.array(first), np.array(last) - np.array(first), wts


def camera_constants(K, D, K_undist) -> np.ndarray:
    """fp32 [16] = {fx, fy, cx, cy | k1, k2, p1, p2, k3 | cxu, cyu | fp32(1 / fxu), fp32(1 / fyu), divided in fp64 | 0, 0, 0}."""
    K, Ku = np.asarray(K, dtype=np.float64), np.asarray(K_undist, dtype=np.float64)
    cam = np.zeros(16, dtype=F)
    cam[:4] = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    cam[4:9] = np.asarray(D, dtype=np.float64).reshape(-1)[:5]
    cam[9:13] = Ku[0, 2], Ku[1, 2], 1.0 / Ku[0, 0], 1.0 / Ku[1, 1]
    return cam


def undistort(image: np.ndarray, lut: np.ndarray, K, D, K_undist, undist_hw) -> np.ndarray:
    """Steps A and B -> uint8 [uh, uw, 3]."""
    return undistort_f32(image, lut, camera_constants(K, D, K_undist), undist_hw)


def undistort_f32(image: np.ndarray, lut: np.ndarray, cam: np.ndarray, undist_hw) -> np.ndarray:
    """Steps A and B from the fp32 camera constants -> uint8 [uh, uw, 3]."""
    h, w = image.shape[:2]
    uh, uw = int(undist_hw[0]), int(undist_hw[1])
    fx, fy, cx, cy, k1, k2, p1, p2, k3, cxu, cyu, ifxu, ifyu = (F(v) for v in np.asarray(cam, dtype=F)[:13])
    half, one, two = F(0.5), F(1.0), F(2.0)
    x = np.arange(uw, dtype=F)[None, :]
    y = np.arange(uh, dtype=F)[:, None]
    with np.errstate(all="ignore"):
        u = ((x + half) - cxu) * ifxu + np.zeros((uh, 1), dtype=F)
        v = ((y + half) - cyu) * ifyu + np.zeros((1, uw), dtype=F)
        r2 = u * u + v * v
        rad = one + r2 * (k1 + r2 * (k2 + r2 * k3))
        du = (u * rad + ((two * p1) * u) * v) + p2 * (r2 + (two * u) * u)
        dv = (v * rad + p1 * (r2 + (two * v) * v)) + ((two * p2) * u) * v
        xs = (fx * du + cx) - half
        ys = (fy * dv + cy) - half
        inside = (xs >= 0) & (ys >= 0) & (xs <= F(w - 1)) & (ys <= F(h - 1))
    xs, ys = np.where(inside, xs, F(0)), np.where(inside, ys, F(0))
    x0f, y0f = np.floor(xs), np.floor(ys)
    ax, ay = xs - x0f, ys - y0f
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    bx, by = one - ax, one - ay
    out = np.zeros((uh, uw, 3), dtype=np.uint8)
    for c in range(3):
        t = lut[c][image[..., c]]
        val = (bx * t[y0, x0] + ax * t[y0, x1]) * by + (bx * t[y1, x0] + ax * t[y1, x1]) * ay
        out[..., c] = np.where(inside, np.minimum(val.astype(np.int32), 255), 0).astype(np.uint8)
    return out


def _area_axis(a: np.ndarray, n_out: int) -> np.ndarray:
    """fp32 [n_in, ...] -> fp32 [n_out, ...] along axis 0: sums in ascending tap order starting from 0.0f."""
    first, _, wts = area_taps(a.shape[0], n_out)
    acc = np.zeros((n_out,) + a.shape[1:], dtype=F)
    for t in range(wts.shape[1]):
        idx = np.minimum(first + t, a.shape[0] - 1)  # a tap past the count has weight 0: it adds +0
        acc = acc + wts[:, t].reshape((-1,) + (1,) * (a.ndim - 1)) * a[idx]
    return acc


def area_resize(und: np.ndarray, resized_wh) -> np.ndarray:
    """Step C: uint8 [uh, uw, 3] -> uint8 [rh, rw, 3]."""
    rw, rh = int(resized_wh[0]), int(resized_wh[1])
    hp = _area_axis(und.astype(F).transpose(1, 0, 2), rw).transpose(1, 0, 2)  # [uh, rw, 3], fp32
    vp = _area_axis(hp, rh)
    return np.clip(np.rint(vp), 0, 255).astype(np.uint8)


def rectify(image, K, D, ccm, K_undist, undist_hw, resized_wh, cropped_ltrb) -> np.ndarray:
    """uint8 [h, w, 3] RGB -> uint8 [bottom - top, right - left, 3]."""
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] == 3
    left, top, right, bottom = (int(v) for v in cropped_ltrb)
    res = area_resize(undistort(image, colour_table(ccm), K, D, K_undist, undist_hw), resized_wh)
    return np.ascontiguousarray(res[top:bottom, left:right])


def reference64(image, K, D, ccm, K_undist, undist_hw, resized_wh, cropped_ltrb) -> np.ndarray:
    """The same four steps in fp64, written on their own: the colour polynomial evaluated per pixel, the distortion in its textbook
    form, the area resize as two dense matrices of interval overlaps."""
    image = np.asarray(image)
    h, w = image.shape[:2]
    uh, uw = int(undist_hw[0]), int(undist_hw[1])
    rw, rh = int(resized_wh[0]), int(resized_wh[1])
    m = np.array(ccm, dtype=np.float32).astype(np.float64)[[2, 1, 0]]
    b = image.astype(np.float64)
    col = np.clip(b * b * m[:, 0] + b * m[:, 1] + m[:, 2], 0.0, 255.0)  # [h, w, 3]
    K, Ku = np.asarray(K, dtype=np.float32).astype(np.float64), np.asarray(K_undist, dtype=np.float32).astype(np.float64)
    k1, k2, p1, p2, k3 = np.asarray(D, dtype=np.float32).astype(np.float64).reshape(-1)[:5]
    gx, gy = np.meshgrid(np.arange(uw, dtype=np.float64), np.arange(uh, dtype=np.float64))
    u, v = (gx + 0.5 - Ku[0, 2]) / Ku[0, 0], (gy + 0.5 - Ku[1, 2]) / Ku[1, 1]
    r2 = u ** 2 + v ** 2
    radial = 1.0 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    ud = u * radial + 2.0 * p1 * u * v + p2 * (r2 + 2.0 * u ** 2)
    vd = v * radial + p1 * (r2 + 2.0 * v ** 2) + 2.0 * p2 * u * v
    xs, ys = K[0, 0] * ud + K[0, 2] - 0.5, K[1, 1] * vd + K[1, 2] - 0.5
    with np.errstate(invalid="ignore"):
        ok = (xs >= 0) & (ys >= 0) & (xs <= w - 1) & (ys <= h - 1)
    xs, ys = np.where(ok, xs, 0.0), np.where(ok, ys, 0.0)
    x0, y0 = np.floor(xs).astype(int), np.floor(ys).astype(int)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    ax, ay = (xs - x0)[..., None], (ys - y0)[..., None]
    val = (col[y0, x0] * (1 - ax) + col[y0, x1] * ax) * (1 - ay) + (col[y1, x0] * (1 - ax) + col[y1, x1] * ax) * ay
    und = np.where(ok[..., None], np.minimum(np.floor(val), 255.0), 0.0)  # the reference's .astype(np.uint8)

    def overlaps(n_in, n_out):
        s = n_in / n_out
        lo, hi = np.arange(n_out)[:, None] * s, (np.arange(n_out)[:, None] + 1) * s
        cell = np.arange(n_in)[None, :]
        return np.clip(np.minimum(hi, cell + 1) - np.maximum(lo, cell), 0.0, None) / s  # [n_out, n_in]
    res = np.einsum("ij,yjc->yic", overlaps(uw, rw), und)
    res = np.einsum("ij,jxc->ixc", overlaps(uh, rh), res)
    res = np.clip(np.rint(res), 0, 255).astype(np.uint8)
    left, top, right, bottom = (int(t) for t in cropped_ltrb)
    return np.ascontiguousarray(res[top:bottom, left:right])


# -- the seeded cases that the CPU and the GPU tests share ---------------------------------------------------------------------------
def texture(h: int, w: int, seed: int) -> np.ndarray:
    """uint8 [h, w, 3]: smooth gradients plus noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([40 + 170 * xx / max(w - 1, 1), 30 + 190 * yy / max(h - 1, 1), 128 + 100 * np.sin(xx / 9.0 + seed) * np.cos(yy / 7.0)], axis=-1)
    return np.clip(img + rng.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)


def make_case(seed: int, h: int, w: int, sx: float, sy: float, k1: float, crop: str, shift: float = 0.0, uh=None, uw=None) -> dict:
    """One seeded case: a w x h source, an undistorted camera of the same size (or uw x uh), scales sx, sy, a crop that touches the
    border `crop` names ("full", "left", "top", "right", "bottom", "inner"); shift moves the principal point so that border pixels
    sample outside the source."""
    rng = np.random.default_rng(1000 + seed)
    uh, uw = int(uh or h), int(uw or w)
    f = 0.9 * max(h, w)
    K = np.array([[f * (1 + 0.01 * rng.standard_normal()), 0, w / 2 + rng.uniform(-3, 3)], [0, f * (1 + 0.01 * rng.standard_normal()), h / 2 + rng.uniform(-3, 3)],
                  [0, 0, 1]])
    Ku = np.array([[f * 0.97, 0, uw / 2 + shift], [0, f * 0.97, uh / 2 - shift], [0, 0, 1]])
    D = np.array([k1, -0.3 * k1 + 0.02, 0.004 * rng.standard_normal(), 0.004 * rng.standard_normal(), 0.05 * rng.standard_normal()])
    ccm = np.array([[2e-4, 0.95, 1.5], [-1e-4, 1.02, -2.0], [1.5e-4, 0.9, 4.0]]) + 1e-5 * rng.standard_normal((3, 3))
    rw, rh = max(1, int(round(uw / sx))), max(1, int(round(uh / sy)))
    cw, ch = max(1, (2 * rw) // 3), max(1, (2 * rh) // 3)
    ltrb = {"full": (0, 0, rw, rh), "left": (0, 3 % rh, cw, min(rh, 3 % rh + ch)), "top": (2 % rw, 0, min(rw, 2 % rw + cw), ch),
            "right": (rw - cw, 1 % rh, rw, min(rh, 1 % rh + ch)), "bottom": (1 % rw, rh - ch, min(rw, 1 % rw + cw), rh),
            "inner": ((rw - cw) // 2, (rh - ch) // 2, (rw - cw) // 2 + cw, (rh - ch) // 2 + ch)}[crop]
    return dict(image=texture(h, w, seed), K=K, D=D, ccm=ccm, K_undist=Ku, undist_hw=(uh, uw), resized_wh=(rw, rh), cropped_ltrb=ltrb)


def cases() -> list:
    """The 12 seeded cases: sources from 64 x 48 to 301 x 263, barrel and pincushion k1, nonzero p1, p2, k3, scales 1.0, 1.37, 1.83, 2.0
    and 3.5 (different per axis), crops touching each border, and cases whose borders sample outside the source."""
    spec = [(48, 64, 1.0, 1.0, -0.12, "full", 0.0), (48, 64, 2.0, 2.0, 0.10, "full", 0.0), (97, 131, 1.37, 1.83, -0.20, "left", 0.0),
            (97, 131, 1.83, 1.37, 0.15, "top", 0.0), (120, 161, 2.0, 3.5, -0.08, "right", 0.0), (120, 161, 3.5, 2.0, 0.12, "bottom", 0.0),
            (263, 301, 1.37, 1.37, -0.25, "inner", 0.0), (263, 301, 2.0, 1.83, 0.20, "full", 0.0), (75, 203, 3.5, 1.0, -0.15, "full", 9.0),
            (203, 75, 1.0, 3.5, 0.18, "full", -7.0), (150, 150, 1.83, 2.0, 0.30, "full", 14.0), (263, 301, 3.5, 3.5, -0.30, "right", -11.0)]
    return [make_case(i, *s) for i, s in enumerate(spec)]
