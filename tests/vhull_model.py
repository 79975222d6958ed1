"""The carving semantics of include/dm4d.h (dm4d_vhull_carve_chunk) restated in numpy fp64, with the same operation order.

Every step is an IEEE fp64 multiply, add, divide or rint in a fixed order, so libdm4d.so is expected to give these points bit
for bit, ties included.  Used by tests/test_vhull_cpu.py (against the recorded reference), tests/test_vhull_gpu.py (seeded scenes
the fixture does not hold) and tests/golden/make_golden_vhull.py (which asserts model == reference when it records).
"""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import torch


def grid_axes(bounds, voxel_size):
    """xs, ys, zs exactly as the reference's build_voxel_grid_linspaces makes them: torch.arange on Python floats (fp32 values)."""
    xmin, xmax, ymin, ymax, zmin, zmax = bounds
    return tuple(torch.arange(lo, hi, voxel_size).numpy() for lo, hi in ((xmin, xmax), (ymin, ymax), (zmin, zmax)))


def project(P: np.ndarray, X: np.ndarray):
    """P [B, 3, 4] fp64, X [M, 3] fp64 -> (u, v, z), each [B, M]: ((p0 X0 + p1 X1) + p2 X2) + p3 per row, then rint of the quotients
    by max(z, 1e-8).  Also returns the unrounded quotients (the fixture's tie margins are measured on them)."""
    X0, X1, X2 = X[None, :, 0], X[None, :, 1], X[None, :, 2]
    r = [((P[:, k, 0:1] * X0 + P[:, k, 1:2] * X1) + P[:, k, 2:3] * X2) + P[:, k, 3:4] for k in range(3)]
    z = r[2]
    den = np.maximum(z, 1e-8)
    with np.errstate(over="ignore", invalid="ignore"):
        qu, qv = r[0] / den, r[1] / den
    return np.rint(qu), np.rint(qv), z, qu, qv


def inside_views(fmasks: np.ndarray, P: np.ndarray, X: np.ndarray) -> np.ndarray:
    """[B, M] bool: view b sees voxel m on foreground."""
    B, H, W = fmasks.shape
    u, v, z, _, _ = project(P, X)
    valid = (z > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)  # in floating point, before any conversion
    ui = np.where(valid, u, 0).astype(np.int64)
    vi = np.where(valid, v, 0).astype(np.int64)
    return valid & fmasks[np.arange(B)[:, None], vi, ui]


def carve(fmasks, Ps, bounds, voxel_size, min_views=None, chunk: int = 200_000) -> np.ndarray:
    """fmasks [B, H, W] bool, Ps [B, 3, 4] -> kept voxel centres fp32 [M, 3] in ascending voxel index (z fastest)."""
    fmasks = np.asarray(fmasks, dtype=bool)
    P = np.asarray(Ps, dtype=np.float64)
    xs, ys, zs = grid_axes(bounds, voxel_size)
    ny, nz = len(ys), len(zs)
    N = len(xs) * ny * nz
    need = fmasks.shape[0] if min_views is None else int(min_views)
    kept = []
    for start in range(0, N, chunk):
        idx = np.arange(start, min(start + chunk, N), dtype=np.int64)
        X = np.stack([xs[idx // (ny * nz)], ys[(idx // nz) % ny], zs[idx % nz]], axis=-1)
        keep = inside_views(fmasks, P, X.astype(np.float64)).sum(axis=0) >= need
        kept.append(X[keep])
    return np.concatenate(kept, axis=0).astype(np.float32).reshape(-1, 3) if kept else np.zeros((0, 3), np.float32)


def margins(fmasks_shape, Ps, bounds, voxel_size, chunk: int = 200_000):
    """(smallest distance of a projected u or v from a half-integer over all voxel-view pairs with z > 0, smallest |z|)."""
    P = np.asarray(Ps, dtype=np.float64)
    xs, ys, zs = grid_axes(bounds, voxel_size)
    ny, nz = len(ys), len(zs)
    N = len(xs) * ny * nz
    tie, zmin = np.inf, np.inf
    for start in range(0, N, chunk):
        idx = np.arange(start, min(start + chunk, N), dtype=np.int64)
        X = np.stack([xs[idx // (ny * nz)], ys[(idx // nz) % ny], zs[idx % nz]], axis=-1).astype(np.float64)
        _, _, z, qu, qv = project(P, X)
        zmin = min(zmin, float(np.abs(z).min()))
        front = z > 0
        if front.any():
            for q in (qu[front], qv[front]):
                tie = min(tie, float(np.abs((q - np.floor(q)) - 0.5).min()))
    return tie, zmin


def read_ply(path):
    """A minimal reader of exactly the layout save_pcd_ply writes."""
    raw = Path(path).read_bytes()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    header = raw[:end].decode("ascii")
    n = int(re.search(r"element vertex (\d+)", header).group(1))
    body = np.frombuffer(raw[end:], dtype=np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("r", "u1"), ("g", "u1"), ("b", "u1")]))
    assert len(body) == n
    return header, np.stack([body["x"], body["y"], body["z"]], -1), np.stack([body["r"], body["g"], body["b"]], -1)
