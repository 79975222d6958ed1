"""CPU: argument validation of dm4d_skeleton_plan_kp3d and dm4d_skeleton_draw_planned_u8.  Like every entry point they return
DM4D_ERR_ARG (-1) with a message in dm4d_last_error() BEFORE anything is launched: the "device" pointers are fake aligned addresses
that are never dereferenced, the host copies are real."""
import numpy as np
import pytest

from diffuman4d_amd.host import lib as L
from diffuman4d_amd.host.resample import TableSet

P = 0x10000
ERR_ARG = -1
F, M, K_PTS, N_LINKS, N_MAPS = 2, 3, 5, 4, 3


@pytest.fixture(scope="module")
def lib():
    return L.load()


def last(lib):
    return lib.dm4d_last_error().decode()


def plan(lib, **kw):
    a = dict(F=F, m=M, k=K_PTS, n=N_MAPS, L=N_LINKS, low=0.5, high=0.9, span=0.4)
    a.update({name: (i + 1) * P for i, name in enumerate(("kp3d", "K", "T", "jobs_dev", "scores", "scale_dev", "sizes_dev", "links_dev",
                                                           "colors_dev", "records", "counts", "status"))})
    a.update({k: v for k, v in kw.items() if not isinstance(v, np.ndarray)})
    n, nl, k = max(a["n"], 1), max(min(a["L"], 1000), 1), max(min(a["k"], 5000), 1)
    host = dict(jobs=np.zeros((n, 2), np.int32), scale=np.tile(np.array([[2.0, 0.0]]), (n, 1)), sizes=np.tile(np.array([[4, 4]], np.int32), (n, 1)),
                links=np.tile(np.array([[0, 1, 0, 2, 2, 0, 0, 0]], np.int32), (nl, 1)), colors=np.tile(np.array([[255, 0, 9, 1]], np.float32), (k + nl, 1)))
    host["links"][:, 2] = np.arange(nl)
    host.update({k_: np.ascontiguousarray(v) for k_, v in kw.items() if isinstance(v, np.ndarray)})
    ptr = {k_: (None if kw.get(k_ + "_host", 0) is None else v.ctypes.data) for k_, v in host.items()}
    return lib.dm4d_skeleton_plan_kp3d(None, a["kp3d"], a["K"], a["T"], a["F"], a["m"], a["k"], ptr["jobs"], a["jobs_dev"], a["n"], a["scores"],
                                       ptr["scale"], a["scale_dev"], ptr["sizes"], a["sizes_dev"], ptr["links"], a["links_dev"], a["L"],
                                       ptr["colors"], a["colors_dev"], a["low"], a["high"], a["span"], a["records"], a["counts"], a["status"])


def test_plan_rejects_null_pointers_and_bad_sizes(lib):
    for name in ("kp3d", "K", "T", "jobs_dev", "scale_dev", "sizes_dev", "links_dev", "colors_dev", "records", "counts", "status",
                 "jobs_host", "scale_host", "sizes_host", "links_host", "colors_host"):
        assert plan(lib, **{name: None}) == ERR_ARG and "null pointer" in last(lib), name
    for name in ("F", "m", "k", "n", "L"):
        for v in (0, -1):
            assert plan(lib, **{name: v}) == ERR_ARG and "empty shape" in last(lib), name
    assert plan(lib, n=65536) == ERR_ARG and "65535 maps" in last(lib)
    assert plan(lib, k=L.SKEL_MAX_KPTS + 1) == ERR_ARG and "DM4D_SKEL_MAX_KPTS" in last(lib)
    assert plan(lib, L=L.SKEL_MAX_PRIMS // 3 + 1) == ERR_ARG and "exceed DM4D_SKEL_MAX_PRIMS" in last(lib)
    for name, off in (("kp3d", 4), ("K", 4), ("T", 4), ("scale_dev", 4), ("records", 8), ("jobs_dev", 2), ("scores", 2), ("sizes_dev", 1),
                      ("links_dev", 2), ("colors_dev", 2), ("counts", 2), ("status", 2)):
        assert plan(lib, **{name: 7 * P + off}) == ERR_ARG and "misaligned" in last(lib), name
    for kw in (dict(low=float("nan")), dict(high=float("inf")), dict(span=0.0), dict(span=-0.4), dict(span=float("nan"))):
        assert plan(lib, **kw) == ERR_ARG and "thresholds" in last(lib), kw


def test_plan_rejects_bad_jobs_parameters_and_tables(lib):
    def jobs(f, c):
        j = np.zeros((N_MAPS, 2), np.int32)
        j[-1] = (f, c)
        return j
    for f, c in ((F, 0), (-1, 0), (0, M), (0, -1)):
        assert plan(lib, jobs=jobs(f, c)) == ERR_ARG and "a job names" in last(lib)
    for bad in (np.nan, np.inf):
        for col in (0, 1):
            scale = np.tile(np.array([[2.0, 0.0]]), (N_MAPS, 1))
            scale[1, col] = bad
            assert plan(lib, scale=scale) == ERR_ARG and "not finite" in last(lib)
    for r, t in ((-1, 4), (4, 0), (L.SKEL_MAX_SIZE // 2 + 1, 4), (4, L.SKEL_MAX_SIZE // 2 + 1)):
        sizes = np.tile(np.array([[4, 4]], np.int32), (N_MAPS, 1))
        sizes[2] = (r, t)
        assert plan(lib, sizes=sizes) == ERR_ARG and "thickness below 1" in last(lib)
    good = np.tile(np.array([[0, 1, 0, 2, 2, 0, 0, 0]], np.int32), (N_LINKS, 1))
    good[:, 2] = np.arange(N_LINKS)
    for col, v, what in ((0, K_PTS, "outside [0, k)"), (1, -1, "outside [0, k)"), (2, N_LINKS, "link id"), (2, -1, "link id"),
                         (3, 0, "multiplier"), (3, 3, "multiplier"), (4, 0, "multiplier")):
        links = good.copy()
        links[3, col] = v
        assert plan(lib, links=links) == ERR_ARG and what in last(lib), (col, v)
    base = np.tile(np.array([[255, 0, 9, 1]], np.float32), (K_PTS + N_LINKS, 1))
    for row, col, v, what in ((0, 0, 256.0, "outside [0, 255]"), (2, 1, -1.0, "outside [0, 255]"), (3, 2, np.nan, "outside [0, 255]"),
                              (1, 3, 0.5, "neither 0 nor 1"), (K_PTS + 1, 3, 0.0, "a link has no colour")):
        colors = base.copy()
        colors[row, col] = v
        assert plan(lib, colors=colors) == ERR_ARG and what in last(lib), (row, col)


def tables(W, w, H, h):
    ts = TableSet()
    (ho, hk), (vo, vk) = ts.add(W, w), ts.add(H, h)
    tab = ts.array()
    return tab[ho:ho + w * (2 + hk)].copy(), hk, tab[vo:vo + h * (2 + vk)].copy(), vk


def draw(lib, **kw):
    H = W = 2048
    h = w = 256
    htab, hk, vtab, vk = tables(W, w, H, h)
    a = dict(records=P, counts=2 * P, n=2, stride=3 * N_LINKS, htab_host=htab, htab_dev=3 * P, hk=hk, vtab_host=vtab, vtab_dev=4 * P, vk=vk,
             H=H, W=W, h=h, w=w, out=5 * P)
    a.update(kw)
    host = [None if a[name] is None else a[name].ctypes.data for name in ("htab_host", "vtab_host")]
    return lib.dm4d_skeleton_draw_planned_u8(None, a["records"], a["counts"], a["n"], a["stride"], host[0], a["htab_dev"], a["hk"], host[1],
                                             a["vtab_dev"], a["vk"], a["H"], a["W"], a["h"], a["w"], a["out"])


def test_draw_planned_rejects_bad_arguments(lib):
    for name in ("records", "counts", "htab_host", "htab_dev", "vtab_host", "vtab_dev", "out"):
        assert draw(lib, **{name: None}) == ERR_ARG and "skeleton_draw_planned: null pointer" in last(lib), name
    for stride in (0, 2, 4, -3, L.SKEL_MAX_PRIMS + 1, 513):
        assert draw(lib, stride=stride) == ERR_ARG and "stride must be 3 L" in last(lib), stride
    for kw in (dict(n=0), dict(n=65536), dict(H=0), dict(W=4097), dict(h=0), dict(w=1 << 16), dict(hk=0), dict(vk=4097)):
        assert draw(lib, **kw) == ERR_ARG and "skeleton_draw_planned: empty or oversized shape" in last(lib), kw
    for name, v in (("records", P + 8), ("counts", 2 * P + 2), ("htab_dev", 3 * P + 1), ("vtab_dev", 4 * P + 2)):
        assert draw(lib, **{name: v}) == ERR_ARG and "aligned" in last(lib), name
    htab, hk, vtab, vk = tables(2048, 256, 2048, 256)
    bad = htab.copy()
    bad[2 * 255] = 2048  # the last window starts past the canvas
    assert draw(lib, htab_host=bad) == ERR_ARG and "windows leave the canvas" in last(lib)
    bad = vtab.copy()
    bad[0], bad[2] = 5, 0  # window starts decrease
    assert draw(lib, vtab_host=bad) == ERR_ARG and "windows leave the canvas" in last(lib)
    # a 32-fold reduction: not even an 8 x 8 tile's part of the canvas fits in LDS beside the list
    htab, hk, vtab, vk = tables(4096, 64, 4096, 64)
    assert draw(lib, htab_host=htab, hk=hk, vtab_host=vtab, vk=vk, H=4096, W=4096, h=64, w=64, stride=510) == ERR_ARG
    assert "does not fit in LDS" in last(lib)


def test_constants_equal_the_header():
    import re
    from pathlib import Path
    header = (Path(__file__).resolve().parent.parent / "include" / "dm4d.h").read_text()
    for name, want in (("SKEL_MAX_KPTS", 2048), ("SKEL_LINK_FIELDS", 8), ("SKEL_ST_NONFINITE", 1), ("SKEL_ST_NOCOLOR", 2),
                       ("SKEL_ST_LINK_SHIFT", 8), ("SKEL_MAX_SIZE", 16384)):
        assert int(re.search(rf"^#define DM4D_{name}[ \t]+(\d+)", header, flags=re.M).group(1)) == getattr(L, name) == want
