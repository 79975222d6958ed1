"""The heatmap cases shared by tests/test_pose_gpu.py (and sized on the CPU by tests/test_pose_cpu.py): Gaussian peaks of sigma 2 with
1 % noise, placed so that every path of the decode is taken.  Built once per size and never changed by a test."""
import functools

import numpy as np

SIGMA = 2.0


def peak(Hh, Wh, cx, cy, amp=1.0, noise=0.01, seed=0):
    ys, xs = np.mgrid[0:Hh, 0:Wh].astype(np.float64)
    g = amp * np.exp(-((xs - cx) ** 2 + (ys - cy) ** 2) / (2 * SIGMA * SIGMA))
    if noise:
        g = g + amp * noise * np.random.default_rng(seed).random((Hh, Wh))
    return g.astype(np.float32)


@functools.lru_cache(maxsize=None)
def special_maps(Hh, Wh):
    """name -> float32 [Hh, Wh]: corners, edges, ties, constants, clipped values, non-positive maps, ordinary interior peaks."""
    out = {}
    for name, (cx, cy) in {"corner_tl": (0.2, 0.3), "corner_tr": (Wh - 1.3, 0.2), "corner_bl": (0.3, Hh - 1.2), "corner_br": (Wh - 1.2, Hh - 1.3),
                           "edge_t": (Wh / 2 + 0.3, 0.2), "edge_b": (Wh / 2 - 0.4, Hh - 1.3), "edge_l": (0.3, Hh / 2 + 0.2),
                           "edge_r": (Wh - 1.2, Hh / 2 - 0.3)}.items():
        out[name] = peak(Hh, Wh, cx, cy, seed=len(out))
    out["interior"] = peak(Hh, Wh, Wh / 2 - 0.37, Hh / 2 + 0.21, seed=20)
    out["interior_small"] = peak(Hh, Wh, Wh / 3 + 0.45, Hh / 3 - 0.15, amp=0.3, seed=21)
    tie = np.maximum(peak(Hh, Wh, 1.0, 2.0, noise=0), peak(Hh, Wh, Wh - 2.0, Hh - 2.0, noise=0))  # two maxima of exactly 1.0
    assert tie[2, 1] == tie[Hh - 2, Wh - 2] == tie.max()
    out["tie"] = tie
    out["constant_high"] = np.full((Hh, Wh), 1000.0, dtype=np.float32)  # every blurred value clips to 50: the step must be 0
    out["constant_low"] = np.full((Hh, Wh), 1e-4, dtype=np.float32)     # every value clips to 1e-3: the step must be 0
    out["above_50"] = peak(Hh, Wh, Wh / 2 + 0.25, Hh / 2 - 0.3, amp=400.0, seed=22)
    out["below_1e-3"] = peak(Hh, Wh, Wh / 2 - 0.2, Hh / 2 + 0.4, amp=5e-4, seed=23)
    out["zero"] = np.zeros((Hh, Wh), dtype=np.float32)
    neg = -peak(Hh, Wh, 2.0, 3.0, seed=24) - 0.5
    out["negative"] = neg
    return out


@functools.lru_cache(maxsize=None)
def row_maps(Hh, Wh):
    """[Hh, Hh, Wh]: map k has its peak in row k, the column walking across the map: every band boundary and halo is crossed."""
    return np.stack([peak(Hh, Wh, 0.35 + (k * 7 % (Wh - 1)) + 0.3 * ((k % 3) - 1) * (0 < k * 7 % (Wh - 1) < Wh - 2), k + 0.25 * ((k % 5) - 2) / 2,
                          seed=100 + k) for k in range(Hh)])


@functools.lru_cache(maxsize=None)
def case_maps(Hh, Wh, rows=False):
    """(names, float32 [K, Hh, Wh])."""
    sp = special_maps(Hh, Wh)
    names, maps = list(sp), [sp[k] for k in sp]
    if rows:
        names += [f"row{k}" for k in range(Hh)]
        maps += list(row_maps(Hh, Wh))
    return names, np.stack(maps)
