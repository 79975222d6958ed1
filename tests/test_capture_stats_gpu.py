"""GPU: dm4d_capture_plane_stats_u8 and dm4d_capture_fill_rects_u8 against tests/capture_stats_model.py: the edge planes in one batch,
each alone, the batch twice; rectangles with guard bytes between the planes."""
import numpy as np
import pytest
import torch

import capture_stats_model as sm
from diffuman4d_amd.host import lib as L
from diffuman4d_amd.host import ops, staging

pytestmark = pytest.mark.gpu


def stats(dev, planes):
    blob, desc = sm.pack_planes(planes)
    meta, meta_host, _, _, desc_off = staging.pack_meta(None, desc, dev)
    out = ops.capture_plane_stats(torch.from_numpy(blob).to(dev), meta, meta_host, len(planes), desc_off)
    return out.cpu().tolist()  # synchronises: meta_host may go


@pytest.fixture(scope="module")
def planes():
    last16 = np.zeros((300, 1000), np.uint8)  # 300 000 bytes: ten blocks' shares, 1000-byte rows
    last16.reshape(-1)[-16:] = 3
    return sm.edge_planes() + [last16, np.full((2902, 2902), 255, np.uint8)]


@pytest.fixture(scope="module")
def want(planes):
    return [sm.plane_stats(p) for p in planes]


def test_the_model_on_the_edge_planes(want):
    assert want[0] == [1, 1, -1, -1, 0] and want[1] == [0, 0, 0, 0, 9] and want[2] == [16, 0, 16, 0, 7] and want[3] == [0, 16, 0, 16, 7]
    assert want[4:8] == [[0, 0, 0, 0, 7], [46, 0, 46, 0, 7], [0, 32, 0, 32, 7], [46, 32, 46, 32, 7]]
    assert want[8] == [6, 4, 6, 4, 7] and want[9] == [64, 64, -1, -1, 0]
    assert want[10] == [984, 299, 999, 299, 48] and want[11] == [0, 0, 2901, 2901, 2147509020]


def test_plane_stats_batch_alone_and_twice(hip_device, planes, want):
    batch = stats(hip_device, planes)
    assert batch == want
    assert stats(hip_device, planes) == batch  # bitwise repeatable
    for k, p in enumerate(planes):
        assert stats(hip_device, [p]) == [want[k]], k
    assert stats(hip_device, planes[::-1]) == want[::-1]


def test_plane_stats_random_planes(hip_device):
    rng = np.random.default_rng(5)
    planes = []
    for _ in range(12):
        h, w = (int(v) for v in rng.integers(1, 200, 2))
        p = np.zeros((h, w, 3) if rng.integers(2) else (h, w), np.uint8)
        if rng.integers(4):
            y, x = int(rng.integers(h)), int(rng.integers(w))
            p[y: y + int(rng.integers(1, 40)), x: x + int(rng.integers(1, 40))] = rng.integers(0, 256, p[y: y + 1, x: x + 1].shape)
        planes.append(p)
    assert stats(hip_device, planes) == [sm.plane_stats(p) for p in planes]


def test_fill_rects_with_guard_bytes(hip_device):
    cases = [(33, 47, (0, 0, 47, 33)), (33, 47, (5, 5, 5, 20)), (1, 1, (0, 0, 1, 1)), (1, 1, (0, 0, 0, 0)), (17, 31, (30, 16, 31, 17)),
             (301, 257, (3, 7, 250, 299)), (64, 64, (0, 10, 64, 11))]
    blob, desc = sm.pack_planes([np.zeros((h, w), np.uint8) for h, w, _ in cases], guard=5)  # planes on multiples of 16 ...
    desc[1::2, 0] -= 3                                                                         # ... and every other one 3 bytes before
    blob[:] = 0xA5
    for row, (_, _, rect) in zip(desc, cases):
        row[3:7] = rect
    meta, meta_host, _, _, desc_off = staging.pack_meta(None, desc, hip_device)
    dev = torch.from_numpy(blob).to(hip_device)
    ops.capture_fill_rects(dev, meta, meta_host, len(cases), desc_off)
    got = dev.cpu().numpy()
    want = blob.copy()
    for row, (h, w, rect) in zip(desc, cases):
        want[row[0]: row[0] + h * w] = sm.fill_rect(h, w, rect).reshape(-1)
    assert (want == 0xA5).sum() >= 2 * len(cases)  # at least two guard bytes in front of every plane
    assert np.array_equal(got, want)


def test_the_wrappers_refuse_what_they_cannot_take(hip_device):
    blob, desc = sm.pack_planes([np.zeros((4, 4), np.uint8)])
    meta, meta_host, _, _, desc_off = staging.pack_meta(None, desc, hip_device)
    with pytest.raises(L.Dm4dError, match="HIP device"):
        ops.capture_plane_stats(torch.from_numpy(blob), meta, meta_host, 1, desc_off)
    with pytest.raises(L.Dm4dError, match="desc_off"):
        ops.capture_plane_stats(torch.from_numpy(blob).to(hip_device), meta, meta_host, 2, desc_off)
    torch.cuda.synchronize()
