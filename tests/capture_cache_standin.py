"""Test-side numpy versions of ops.capture_crop_resize_packed and ops.capture_unpack_cells (tests/test_capture_cache_cpu.py), built
from capture_model.crop_resize and capture_model.epilogue, and the helpers the cache tests on both sides share.  A cell descriptor names
its slab by address: here the slabs are host tensors, and the address is turned back into their bytes."""
import ctypes

import numpy as np
import torch

import capture_model as cm
from diffuman4d_amd.host import capture
from diffuman4d_amd.host import lib as L


def resized_planes(host: np.ndarray, d, H: int, W: int):
    """The three resized uint8 planes (image [H, W, 3], mask [H, W], skeleton [H, W, 3]) of the frame descriptor `d` over the staging
    bytes `host`."""
    oi, om, os_, sh, sw, top, left, ch, cw = (int(v) for v in d[:9])
    plane = lambda o, c: host[o: o + sh * sw * c].reshape(sh, sw, c)
    args = (top, left, ch, cw, H, W)
    return cm.crop_resize(plane(oi, 3), *args), cm.crop_resize(plane(om, 1), *args)[..., 0], cm.crop_resize(plane(os_, 3), *args)


def pack_cell(img: np.ndarray, mask: np.ndarray, skel: np.ndarray) -> np.ndarray:
    """The cell format: [H, W, 8] uint8 = {i0 i1 i2 m s0 s1 s2 0}."""
    return np.concatenate([img, mask[..., None], skel, np.zeros_like(mask)[..., None]], axis=-1)


def cell_view(row, H: int, W: int) -> np.ndarray:
    """The [H, W, 8] bytes a cell descriptor names, in place."""
    addr, nbytes, off = (int(v) for v in row[:3])
    assert addr % 16 == 0 and off % 16 == 0 and 0 <= off and off + H * W * 8 <= nbytes
    return np.frombuffer((ctypes.c_uint8 * nbytes).from_address(addr), np.uint8)[off: off + H * W * 8].reshape(H, W, 8)


def standin_crop_resize_packed(blob, blob_host, n_frames, desc_off, tab_off, tab_len, H, W, cells_host, cells, meta=None):
    """Drop-in for ops.capture_crop_resize_packed on the host."""
    if meta is not None:  # blob holds planes only; blob_host is the host copy of meta
        desc_off, blob = blob.numel() + desc_off, torch.cat([blob, blob_host])
    host = blob.numpy()
    desc = host[desc_off: desc_off + n_frames * capture.FIELDS * 8].view(np.int64).reshape(n_frames, capture.FIELDS)
    assert tuple(cells_host.shape) == (n_frames, L.CAPTURE_CELL_FIELDS) and torch.equal(cells_host, cells)
    for d, row in zip(desc, cells_host.numpy()):
        cell_view(row, H, W)[:] = pack_cell(*resized_planes(host, d, H, W))


def standin_unpack_cells(cells_host, cells, n_out_rows, H, W, out=None):
    """Drop-in for ops.capture_unpack_cells on the host."""
    assert torch.equal(cells_host, cells)
    pix, skel = out if out is not None else (torch.empty(n_out_rows, 3, H, W), torch.empty(n_out_rows, 3, H, W))
    rows = cells_host.numpy()
    assert len(set(rows[:, 3].tolist())) == len(rows) and rows[:, 3].min() >= 0 and rows[:, 3].max() < n_out_rows
    for row in rows:
        c = cell_view(row, H, W)
        assert not c[..., 7].any()
        pix[int(row[3])], skel[int(row[3])] = cm.epilogue(c[..., :3], c[..., 3], c[..., 4:7])
    return pix, skel


# -- what the dataset tests on both sides share -----------------------------------------------------------------------------------------
def same(a, b):
    """Two get_item dicts: every tensor torch.equal (and on one device), every other entry equal."""
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert a[k].device == b[k].device and a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def sequence(ks):
    """spatial(frame 0), spatial(frame 1), temporal(target 03), spatial(frame 0) on kp2d_scene: calls 3 and 4 need no new cell."""
    return [(ks.CAMS, ks.FRAMES[:1]), (ks.CAMS, ks.FRAMES[1:]), (["03"], ks.FRAMES), (ks.CAMS, ks.FRAMES[:1])]


class OpenLog:
    """Counts the image, mask and skeleton files capture.py opens (_open: Pillow's decode; _read: the probe of device_decode=True)."""

    def __init__(self, monkeypatch):
        self.paths = []
        for name in ("_open", "_read"):
            real = getattr(capture, name)
            monkeypatch.setattr(capture, name, lambda path, mode, _real=real: self.paths.append(path) or _real(path, mode))

    def take(self):
        got, self.paths = sorted(self.paths), []
        return got
