"""Pillow's bicubic and bilinear coefficient tables, and the packing of several of them into the one int32 array a launch takes.

The device side applies these tables by one rule (``csrc/image_common.h``); ``host/capture.py``, ``host/jpeg.py``,
``host/skeleton.py`` and ``host/matting.py`` all get them here.  numpy only.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, Tuple

import numpy as np

PRECISION_BITS = 22  # Pillow's fixed-point coefficients for 8-bit images (libImaging/Resample.c)


def _bicubic(x: np.ndarray) -> np.ndarray:
    """Pillow's bicubic kernel, a = -0.5, in its own order of operations."""
    x = np.abs(x)
    near = ((1.5 * x - 2.5) * x) * x + 1.0
    far = (((x - 5.0) * x + 8.0) * x - 4.0) * -0.5
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def _bilinear(x: np.ndarray) -> np.ndarray:
    """Pillow's bilinear (triangle) kernel."""
    x = np.abs(x)
    return np.where(x < 1.0, 1.0 - x, 0.0)


def _table(in_size: int, out_size: int, kernel: Callable[[np.ndarray], np.ndarray], kernel_support: float) -> Tuple[np.ndarray, np.ndarray]:
    """Pillow's coefficients (precompute_coeffs + normalize_coeffs_8bpc) for resizing an axis of `in_size` pixels to `out_size` with the
    filter `kernel` of half-width `kernel_support`: ([out, 2] int32 window {start, length}, [out, ksize] int32 weights with 22
    fractional bits).  float64 throughout, the weights of a window summed left to right (a pairwise sum can move a coefficient by one
    unit), each scaled by 1 / filterscale as a product."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = kernel_support * fs
    ksize = int(math.ceil(support)) * 2 + 1
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    lo = np.maximum(np.trunc(center - support + 0.5), 0).astype(np.int64)  # C's (int) truncates
    hi = np.minimum(np.trunc(center + support + 0.5), in_size).astype(np.int64)
    n = hi - lo
    t = np.arange(ksize)
    w = kernel(((t[None, :] + lo[:, None]) - center[:, None] + 0.5) * (1.0 / fs))
    w = np.where(t[None, :] < n[:, None], w, 0.0)
    total = np.zeros(out_size)
    for j in range(ksize):  # sequential sum; the zero tail adds nothing
        total = total + w[:, j]
    w = np.where(total[:, None] != 0.0, w / np.where(total == 0.0, 1.0, total)[:, None], w)
    scaled = w * float(1 << PRECISION_BITS)
    k = np.trunc(np.where(w < 0, -0.5 + scaled, 0.5 + scaled)).astype(np.int32)
    return np.stack([lo, n], axis=1).astype(np.int32), k


def bicubic_table(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """The table of ``resize(..., Image.BICUBIC)`` (Pillow's default filter) for an axis of `in_size` pixels (the crop) -> `out_size`."""
    return _table(in_size, out_size, _bicubic, 2.0)


def bilinear_table(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """The table of ``resize(..., Image.BILINEAR)``, Pillow's antialiased triangle filter, for an axis of `in_size` pixels -> `out_size`."""
    return _table(in_size, out_size, _bilinear, 1.0)


FILTERS = {"bicubic": bicubic_table, "bilinear": bilinear_table}


class TableSet:
    """One table per distinct (in_size, out_size) pair and filter, each stored as its windows then its weights, end to end in one
    int32 array and addressed by offset.  `tables` is keyed (in_size, out_size) for bicubic, (in_size, out_size, filter) otherwise."""

    def __init__(self) -> None:
        self.tables: Dict[Tuple, Tuple[int, int]] = {}
        self._chunks: List[np.ndarray] = []
        self._len = 0

    def add(self, in_size: int, out_size: int, filter: str = "bicubic") -> Tuple[int, int]:
        """-> (offset of the pair's table in int32 units, its ksize); the table is computed the first time the pair is seen."""
        key = (in_size, out_size) if filter == "bicubic" else (in_size, out_size, filter)
        if key not in self.tables:
            b, k = FILTERS[filter](in_size, out_size)
            self.tables[key] = (self._len, k.shape[1])
            self._chunks += [b.reshape(-1), k.reshape(-1)]
            self._len += b.size + k.size
        return self.tables[key]

    def array(self) -> np.ndarray:
        return np.concatenate(self._chunks).astype(np.int32)
