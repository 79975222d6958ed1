"""GPU: the device cell cache.  dm4d_capture_crop_resize_packed_u8 and dm4d_capture_unpack_cells_f32 against the numpy definition
(tests/capture_model.py) and against the fused entry on the same staging buffer; SpaTemDataset(device_cache=True) against the flag-off
dataset over a job-like sequence of calls for every skeleton source, with device_decode off and on; four loader threads on overlapping
tasks; error parity and a budget that retains nothing."""
import shutil
import threading

import numpy as np
import pytest
import torch

import capture_cache_standin as cs
import capture_model as cm
import kp2d_scene as ks
from diffuman4d_amd.host import capture, ops, skeleton, triang
from diffuman4d_amd.host.staging import Layout, write_meta

pytestmark = pytest.mark.gpu

PALETTE = skeleton.load_palette(ks.PALETTE_PATH)
OUT = 64
HW = ks.SIZES[0]
SENTINEL = 0xA5

# as tests/test_capture_decode_gpu.py: the device entries, whatever another test module left installed in capture.ops
GENUINE = {name: getattr(ops, name) for name in ("capture_crop_resize", "capture_crop_resize_packed", "capture_unpack_cells", "skeleton_draw",
                                                 "skeleton_box_mask", "capture_plane_stats", "capture_fill_rects")}
assert all(f.__module__ == ops.__name__ for f in GENUINE.values())


@pytest.fixture(autouse=True)
def genuine_ops(monkeypatch):
    for name, f in GENUINE.items():
        monkeypatch.setattr(ops, name, f)


# -- 1. the kernels ---------------------------------------------------------------------------------------------------------------------
def frame(rng, h, w, crop):
    mask = rng.integers(0, 256, (h, w), dtype=np.uint8)
    mask[rng.random((h, w)) < 0.3] = 0
    return {"img": rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "mask": mask, "skel": rng.integers(0, 256, (h, w, 3), dtype=np.uint8),
            "crop": list(crop) + [h, w]}


def stage(frames, H, W):
    """The staging buffer of SpaTemDataset._resize_on_device for `frames` -> (host uint8 blob, desc_off, tab_off, tab_len)."""
    ds = capture.SpaTemDataset.__new__(capture.SpaTemDataset)
    ds.height, ds.width = H, W
    tables, tab = ds._tables(frames)
    lay = Layout()
    plane_offs = [[lay.add(fr[name].size) for name in ("img", "mask", "skel")] for fr in frames]
    tab_off, desc_off = lay.add(tab.nbytes), lay.add(len(frames) * capture.FIELDS * 8)
    desc = ds._descriptors(frames, plane_offs, [fr["skel"].shape[:2] for fr in frames], tables, tab)
    blob = torch.zeros(lay.total, dtype=torch.uint8)
    for fr, offs in zip(frames, plane_offs):
        for o, name in zip(offs, ("img", "mask", "skel")):
            blob.numpy()[o: o + fr[name].size] = fr[name].reshape(-1)
    write_meta(blob.numpy(), tab, tab_off, desc, desc_off)
    return blob, desc_off, tab_off, tab.size


@pytest.mark.parametrize("H,W", [(1, 4), (3, 8), (5, 260)])  # 260: one lane in the second x-block of the grid
def test_the_kernels_equal_the_definition_and_the_fused_entry(hip_device, H, W):
    rng = np.random.default_rng(H * 1000 + W)
    frames = [frame(rng, 37, 53, (-3, -4, 30, 30)),   # the crop leaves the image on the top and left
              frame(rng, 64, 300, (10, 20, 50, 270)),
              frame(rng, 9, 5, (2, 1, 4, 3))]         # upscaled in x for every W here, in y for H = 5
    n, cell = len(frames), H * W * 8
    host, desc_off, tab_off, tab_len = stage(frames, H, W)
    blob = host.to(hip_device)
    # two slabs with 16 sentinel bytes around every cell; frame 0 -> the second cell of slab A, frame 1 -> the very end of slab B, frame 2 -> the
    # first cell of slab A: neither slabs nor offsets come in frame order
    slab_a = torch.full((16 + cell + 16 + cell + 16,), SENTINEL, dtype=torch.uint8, device=hip_device)
    slab_b = torch.full((32 + cell,), SENTINEL, dtype=torch.uint8, device=hip_device)
    at = [(slab_a, 32 + cell), (slab_b, 32), (slab_a, 16)]
    out_rows, n_out = [3, 0, 4], n + 2
    cells = torch.tensor([[s.data_ptr(), s.numel(), off, r] for (s, off), r in zip(at, out_rows)], dtype=torch.int64)
    cells_dev = cells.to(hip_device)

    def run():
        slab_a.fill_(SENTINEL), slab_b.fill_(SENTINEL)
        ops.capture_crop_resize_packed(blob, host, n, desc_off, tab_off, tab_len, H, W, cells, cells_dev)
        out = (torch.full((n_out, 3, H, W), 7.0, device=hip_device), torch.full((n_out, 3, H, W), -7.0, device=hip_device))
        pix, skel = ops.capture_unpack_cells(cells, cells_dev, n_out, H, W, out=out)
        assert pix is out[0] and skel is out[1]
        return slab_a.cpu().numpy().copy(), slab_b.cpu().numpy().copy(), pix.cpu(), skel.cpu()

    a, b, pix, skel = run()
    fused_pix, fused_skel = (t.cpu() for t in ops.capture_crop_resize(blob, host, n, desc_off, tab_off, tab_len, H, W))
    slabs = {slab_a.data_ptr(): a, slab_b.data_ptr(): b}
    covered = {k: np.zeros(v.size, bool) for k, v in slabs.items()}
    for f, (fr, (s, off), r) in enumerate(zip(frames, at, out_rows)):
        args = (*fr["crop"][:4], H, W)
        planes = cm.crop_resize(fr["img"], *args), cm.crop_resize(fr["mask"], *args), cm.crop_resize(fr["skel"], *args)
        got = slabs[s.data_ptr()][off: off + cell].reshape(H, W, 8)
        assert np.array_equal(got, cs.pack_cell(*planes)), f"frame {f}: {int((got != cs.pack_cell(*planes)).sum())} cell bytes differ"
        assert not got[..., 7].any()
        covered[s.data_ptr()][off: off + cell] = True
        want_pix, want_skel = cm.epilogue(*planes)
        assert torch.equal(pix[r], want_pix) and torch.equal(skel[r], want_skel), f"frame {f}: the unpacked row is not the definition's"
        assert torch.equal(pix[r], fused_pix[f]) and torch.equal(skel[r], fused_skel[f]), f"frame {f}: the unpacked row is not the fused entry's"
    for k, v in slabs.items():  # every byte next to a cell still holds its sentinel
        assert (v[~covered[k]] == SENTINEL).all() and (~covered[k]).sum() == v.size - cell * (2 if k == slab_a.data_ptr() else 1)
    for r in set(range(n_out)) - set(out_rows):  # rows no descriptor names are not touched
        assert (pix[r] == 7.0).all() and (skel[r] == -7.0).all()
    a2, b2, pix2, skel2 = run()
    assert np.array_equal(a, a2) and np.array_equal(b, b2) and torch.equal(pix, pix2) and torch.equal(skel, skel2)


def test_the_wrappers_refuse_host_tensors_and_bad_descriptors(hip_device):
    host, desc_off, tab_off, tab_len = stage([frame(np.random.default_rng(0), 9, 5, (2, 1, 4, 3))], 3, 8)
    slab = torch.zeros(3 * 8 * 8, dtype=torch.uint8, device=hip_device)
    cells = torch.tensor([[slab.data_ptr(), slab.numel(), 0, 0]], dtype=torch.int64)
    L = capture._l
    with pytest.raises(L.Dm4dError, match="blob: expected a tensor on a HIP device"):
        ops.capture_crop_resize_packed(host, host, 1, desc_off, tab_off, tab_len, 3, 8, cells, cells.to(hip_device))
    with pytest.raises(L.Dm4dError, match="cells: expected a tensor on a HIP device"):
        ops.capture_crop_resize_packed(host.to(hip_device), host, 1, desc_off, tab_off, tab_len, 3, 8, cells, cells)
    with pytest.raises(L.Dm4dError, match="cells: expected a tensor on a HIP device"):
        ops.capture_unpack_cells(cells, cells, 1, 3, 8)
    with pytest.raises(L.Dm4dError, match="cells: expected contiguous int64"):
        ops.capture_unpack_cells(cells[:, :3].contiguous(), cells.to(hip_device), 1, 3, 8)
    with pytest.raises(L.Dm4dError, match="pixel_values: expected a contiguous"):
        ops.capture_unpack_cells(cells, cells.to(hip_device), 1, 3, 8, out=(torch.empty(2, 3, 3, 8, device=hip_device),) * 2)
    bad = cells.clone()
    bad[0, 2] = 16  # the cell leaves its slab: the library refuses before it launches
    with pytest.raises(L.Dm4dError, match="capture_cells"):
        ops.capture_unpack_cells(bad, bad.to(hip_device), 1, 3, 8)
    with pytest.raises(L.Dm4dError, match="capture_cells"):
        ops.capture_crop_resize_packed(host.to(hip_device), host, 1, desc_off, tab_off, tab_len, 3, 8, bad, bad.to(hip_device))


# -- 2. the dataset ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_root(hip_device, tmp_path_factory):
    """kp2d_scene's first size as tests/test_capture_decode_gpu.py builds it: poses_3d and poses_2d from the native triangulation, skeleton
    PNGs from the native draw; images, masks and skeletons are PNG files, which device_decode=True decodes on the device."""
    root = tmp_path_factory.mktemp("cache_gpu")
    d = ks.write_cameras_and_detections(root, HW)
    triang.triangulate_skeleton(str(d / "transforms.json"), str(d / "poses_sapiens"), str(d / "poses_3d"),
                                out_kp2d_proj_dir=str(d / "poses_2d"), spa_labels_proj=list(range(8)))
    ks.write_images_and_masks(d, HW)
    ks.write_skeleton_pngs(d, HW, PALETTE, skeleton.draw_plans)
    return root


SOURCES = {"files": {}, "kp2d": {"skeleton_source": "kp2d", "palette": PALETTE}, "kp3d": {"skeleton_source": "kp3d", "palette": PALETTE}}


def dataset(root, **kw):
    return capture.SpaTemDataset(data_dir=str(root), scene_label=ks.SCENE, height=OUT, width=OUT, decode_threads=4, **{**ks.patterns(), **kw})


@pytest.mark.parametrize("has_gt_target", [True, False])
@pytest.mark.parametrize("device_decode", [False, True])
@pytest.mark.parametrize("source", sorted(SOURCES))
def test_the_sequence_equals_flag_off(scene_root, monkeypatch, source, device_decode, has_gt_target):
    opened = cs.OpenLog(monkeypatch)
    kw = dict(has_gt_target=has_gt_target, device_decode=device_decode, **SOURCES[source])
    off, on = dataset(scene_root, **kw), dataset(scene_root, device_cache=True, **kw)
    for call, (spa, tem) in enumerate(cs.sequence(ks), 1):
        want = off.get_item(ks.SCENE, spa, tem, ks.INPUTS)
        files_off = opened.take()
        if call == 2:
            decoded_by_two_calls = dict(off.decode_stats)
        got = on.get_item(ks.SCENE, spa, tem, ks.INPUTS)
        files_on = opened.take()
        cs.same(got, want)
        assert got["pixel_values"].is_cuda and got["skeletons"].max() > -1.0
        assert files_on == (files_off if call <= 2 else []), call  # calls 3 and 4 open no image, mask or skeleton file
        assert files_off
    assert on.decode_stats == decoded_by_two_calls  # only the misses were decoded
    assert (on.decode_stats["device"] > 0) == device_decode
    assert on.cache_stats == {"hits": 4 + 8, "misses": 16, "unretained": 0, "cells": 16, "bytes": 64 * OUT * OUT * 8}


# -- 3. four loader threads -------------------------------------------------------------------------------------------------------------
def test_four_threads_on_overlapping_tasks_decode_each_cell_once(scene_root):
    off, on = dataset(scene_root), dataset(scene_root, device_cache=True)
    near = {}
    for cam in ks.CAMS:
        if cam not in ks.INPUTS:
            near.setdefault(off.nearest_input_camera(int(cam), [int(c) for c in ks.INPUTS]), []).append(cam)
    t1, t2 = next(v for v in near.values() if len(v) >= 2)[:2]  # two targets with the same conditioning camera
    tasks = [(ks.CAMS, ks.FRAMES[:1]), (ks.CAMS, ks.FRAMES[1:]), ([t1], ks.FRAMES), ([t2], ks.FRAMES)]
    want = [off.get_item(ks.SCENE, spa, tem, ks.INPUTS) for spa, tem in tasks]
    start, got, errors = threading.Barrier(len(tasks)), [None] * len(tasks), []

    def run(i):
        try:
            start.wait(timeout=60)
            got[i] = on.get_item(ks.SCENE, *tasks[i], ks.INPUTS)
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    ts = [threading.Thread(target=run, args=(i,), daemon=True) for i in range(len(tasks))]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
    assert not errors and not any(t.is_alive() for t in ts), errors
    for g, w in zip(got, want):
        cs.same(g, w)
    distinct = {lab for w in want for lab in w["labels"]}
    st = on.cache_stats
    assert len(distinct) == 16 and st["misses"] == st["cells"] == 16 and st["unretained"] == 0  # each cell was loaded once
    assert st["hits"] == sum(len(w["labels"]) for w in want) - 16


# -- 4. error parity and the budget -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_decode", [False, True])
def test_a_truncated_mask_raises_the_same_and_leaves_the_calls_cells_absent(scene_root, tmp_path, device_decode):
    shutil.copytree(scene_root / ks.SCENE, tmp_path / ks.SCENE)
    mask = tmp_path / ks.SCENE / "fmasks" / "04" / f"{ks.FRAMES[1]}.png"
    whole = mask.read_bytes()
    mask.write_bytes(whole[: len(whole) // 2])
    off, on = dataset(tmp_path, device_decode=device_decode), dataset(tmp_path, device_decode=device_decode, device_cache=True)
    (spa0, tem0), (spa1, tem1) = cs.sequence(ks)[:2]
    cs.same(on.get_item(ks.SCENE, spa0, tem0, ks.INPUTS), off.get_item(ks.SCENE, spa0, tem0, ks.INPUTS))
    errors = []
    for ds in (off, on):
        with pytest.raises(Exception) as e:
            ds.get_item(ks.SCENE, spa1, tem1, ks.INPUTS)
        errors.append((type(e.value), str(e.value)))
    assert errors[0] == errors[1]
    cache = on._cache(on._device())
    key = lambda s, t: (on._device().index, ks.SCENE, s, t, s in ks.INPUTS)
    assert all(cache.state(key(s, tem1[0])) == "absent" for s in spa1) and all(cache.state(key(s, tem0[0])) == "ready" for s in spa0)
    assert on.cache_stats["cells"] == 8
    mask.write_bytes(whole)
    cs.same(on.get_item(ks.SCENE, spa1, tem1, ks.INPUTS), off.get_item(ks.SCENE, spa1, tem1, ks.INPUTS))
    assert on.cache_stats["cells"] == 16


def test_a_budget_of_five_cells(scene_root):
    off = dataset(scene_root)
    on = dataset(scene_root, device_cache=True, device_cache_bytes=5 * OUT * OUT * 8)
    for spa, tem in cs.sequence(ks):
        cs.same(on.get_item(ks.SCENE, spa, tem, ks.INPUTS), off.get_item(ks.SCENE, spa, tem, ks.INPUTS))
        st = on.cache_stats
        assert st["cells"] <= 5 and st["bytes"] <= 5 * OUT * OUT * 8
    assert st["unretained"] > 0 and st["unretained"] == st["misses"] - st["cells"]
    on.clear_device_cache()
    assert on.cache_stats["cells"] == 0 and on.cache_stats["bytes"] == 0
