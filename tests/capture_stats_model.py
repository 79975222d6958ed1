"""numpy model of the two device steps of ``SpaTemDataset(device_decode=True)`` (csrc/capture.hip): ``dm4d_capture_plane_stats_u8`` and
``dm4d_capture_fill_rects_u8``, by their definitions in include/dm4d.h.  No device, no library."""
from typing import List, Sequence

import numpy as np


def plane_stats(plane: np.ndarray) -> List[int]:
    """uint8 [h, w] or [h, w, 3] -> [first column, first row, last column, last row, sum]: the columns and rows of the pixels with at
    least one non-zero channel, [w, h, -1, -1] for a plane without one; the sum of all the plane's bytes."""
    assert plane.dtype == np.uint8 and plane.ndim in (2, 3)
    h, w = plane.shape[:2]
    nz = plane != 0 if plane.ndim == 2 else (plane != 0).any(axis=2)
    rows, cols = np.flatnonzero(nz.any(axis=1)), np.flatnonzero(nz.any(axis=0))
    total = int(plane.sum(dtype=np.int64))
    if rows.size == 0:
        return [w, h, -1, -1, total]
    return [int(cols[0]), int(rows[0]), int(cols[-1]), int(rows[-1]), total]


def fill_rect(h: int, w: int, rect: Sequence[int]) -> np.ndarray:
    """(c0, r0, c1, r1) -> uint8 [h, w]: 255 on rows r0 .. r1 - 1 and columns c0 .. c1 - 1, 0 elsewhere."""
    c0, r0, c1, r1 = (int(v) for v in rect)
    assert 0 <= c0 <= c1 <= w and 0 <= r0 <= r1 <= h
    out = np.zeros((h, w), dtype=np.uint8)
    out[r0:r1, c0:c1] = 255
    return out


def pack_planes(planes: Sequence[np.ndarray], guard: int = 0):
    """The planes in one blob, each on a multiple of 16 bytes after `guard` bytes of 0xA5 -> (blob uint8, int64 [n, 8] plane descriptors
    {byte offset, h, w, channels, 0 ...})."""
    desc = np.zeros((len(planes), 8), dtype=np.int64)
    parts, at = [], 0
    for k, p in enumerate(planes):
        pad = (-(at + guard)) % 16 + guard
        parts.append(np.full(pad, 0xA5, dtype=np.uint8))
        at += pad
        desc[k, :4] = [at, p.shape[0], p.shape[1], 1 if p.ndim == 2 else p.shape[2]]
        parts.append(np.ascontiguousarray(p).reshape(-1))
        at += p.size
    parts.append(np.full(guard, 0xA5, dtype=np.uint8))
    return np.concatenate(parts), desc


def edge_planes() -> List[np.ndarray]:
    """The small edge planes of the issue's list (the two large ones are built by the GPU test)."""
    def one(h, w, *at, c=None):
        p = np.zeros((h, w) if c is None else (h, w, 3), dtype=np.uint8)
        p[at] = 7
        return p
    planes = [np.zeros((1, 1), np.uint8), np.full((1, 1), 9, np.uint8), one(1, 17, 0, 16), one(17, 1, 16, 0)]
    planes += [one(33, 47, r, c) for r, c in ((0, 0), (0, 46), (32, 0), (32, 46))]
    planes += [one(5, 7, 4, 6, 2, c=3), np.zeros((64, 64), np.uint8)]
    return planes
