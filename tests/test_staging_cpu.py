"""CPU: diffuman4d_amd/host/staging.py (offsets, pinned fill, the {tables | descriptors} pack, the small helpers), the layouts that
host/pose.py and host/matting.py build with it, and ops._check_meta, the one check of "meta_host is the host copy of meta, offsets in
range and aligned".  No device: buffers are pageable, tensors are plain CPU tensors.  Every comparison is for equality."""
import os
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch
from PIL import Image

CPU = torch.device("cpu")


def a16(n):
    return -(-n // 16) * 16


# -- allocator -------------------------------------------------------------------------------------------------------------------------
def test_layout_offsets():
    from diffuman4d_amd.host.staging import Layout
    lay = Layout()
    offs = [lay.add(n) for n in [1, 15, 16, 17, 0, 48]]
    assert offs == [0, 16, 32, 48, 80, 80] and lay.total == 128 and all(o % 16 == 0 for o in offs)
    lay = Layout(37)  # a buffer whose first 37 bytes are somebody else's
    assert lay.total == 48 and lay.add(5) == 48 and lay.total == 64
    assert Layout().total == 0


# -- fill ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pooled", [False, True])
def test_fill_arrays_and_images(pooled):
    from diffuman4d_amd.host import staging
    rng = np.random.default_rng(3)
    rgb = Image.fromarray(rng.integers(0, 256, (5, 7, 3), dtype=np.uint8))
    grey = Image.fromarray(rng.integers(0, 256, (4, 3), dtype=np.uint8))
    one = Image.fromarray(rng.integers(0, 2, (6, 5), dtype=np.uint8).astype(bool))
    assert one.mode == "1"
    sources = [rng.integers(0, 256, (3, 5), dtype=np.uint8), rng.random((2, 3), dtype=np.float32), (rgb, "RGB"), (grey, "L"), (grey, "RGB"),
               (one, "L"), (one, "1"), rng.integers(0, 256, (4, 6), dtype=np.uint8)[:, ::2]]  # the last one is not contiguous
    want = [np.ascontiguousarray(s if isinstance(s, np.ndarray) else np.asarray(s[0].convert(s[1]))).reshape(-1).view(np.uint8) for s in sources]
    lay = staging.Layout()
    offs = [lay.add(w.size) for w in want]
    buf = staging.pinned(lay.total, CPU)
    assert buf.dtype == torch.uint8 and buf.numel() == lay.total and buf.device.type == "cpu"
    view = buf.numpy()
    view[:] = 0xA5
    pool = ThreadPoolExecutor(max_workers=3) if pooled else None
    try:
        staging.fill(view, list(zip(offs, sources)), pool)
    finally:
        if pool is not None:
            pool.shutdown()
    covered = np.zeros(lay.total, dtype=bool)
    for o, w in zip(offs, want):
        assert np.array_equal(view[o: o + w.size], w)
        covered[o: o + w.size] = True
    assert not covered.all() and np.all(view[~covered] == 0xA5)  # the alignment gaps are nobody's


def test_pool_map_keeps_order_with_and_without_a_pool():
    from diffuman4d_amd.host.staging import pool_map
    with ThreadPoolExecutor(max_workers=4) as pool:
        assert pool_map(pool, lambda x: x * x, range(20)) == pool_map(None, lambda x: x * x, range(20)) == [x * x for x in range(20)]


# -- meta pack -------------------------------------------------------------------------------------------------------------------------
def test_pack_meta_is_tab_pad_desc():
    from diffuman4d_amd.host import staging
    tab = np.arange(100, 105, dtype=np.int32)
    desc = np.arange(24, dtype=np.int64).reshape(3, 8) - 5
    meta, host, tab_off, tab_len, desc_off = staging.pack_meta(tab, desc, CPU)
    assert (tab_off, tab_len, desc_off) == (0, 5, 32)
    assert host.numpy().tobytes() == tab.tobytes() + bytes(12) + desc.tobytes()
    assert meta.device.type == "cpu" and torch.equal(meta, host)
    meta, host, tab_off, tab_len, desc_off = staging.pack_meta(None, desc, CPU)
    assert (tab_off, tab_len, desc_off) == (0, 0, 0) and host.numpy().tobytes() == desc.tobytes()


def test_write_meta_leaves_the_other_bytes_alone():
    from diffuman4d_amd.host import staging
    tab = np.arange(5, dtype=np.int32)
    desc = np.arange(24, dtype=np.int64).reshape(3, 8)
    view = np.full(400, 0x5A, dtype=np.uint8)
    staging.write_meta(view, tab, 48, desc, 80)
    want = np.full(400, 0x5A, dtype=np.uint8)
    want[48: 68] = np.frombuffer(tab.tobytes(), dtype=np.uint8)
    want[80: 272] = np.frombuffer(desc.tobytes(), dtype=np.uint8)
    assert np.array_equal(view, want)
    view[:] = 0x5A
    staging.write_meta(view, None, 48, desc, 80)
    want[48: 68] = 0x5A
    assert np.array_equal(view, want)


# -- the layouts the stages build ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("to_net", [True, False])
@pytest.mark.parametrize("rot", [0, 1, 2, 3])
def test_matting_plan_offsets_are_running_multiples_of_16(rot, to_net):
    from diffuman4d_amd.host import matting
    sizes, net = [(7, 9), (16, 16), (16, 40), (1, 1)], (16, 16)
    desc, tab, plane_bytes, scratch_bytes = matting._plan(sizes, net, rot, to_net)
    plane = scratch = 0
    for k, (h, w) in enumerate(sizes):
        rh, rw = (w, h) if rot & 1 else (h, w)
        assert desc[k, :3].tolist() == [plane, h, w]
        plane = a16(plane + h * w * (3 if to_net else 1))
        if desc[k, 3] >= 0:  # a horizontal pass: its scratch region
            assert desc[k, 7] == scratch
            scratch = a16(scratch + (rh * net[1] * 4 if to_net else net[0] * rw))
        else:
            assert desc[k, 7] == 0
    assert (plane_bytes, scratch_bytes) == (plane, max(scratch, 16))
    assert tab.dtype == np.int32 and tab.size >= 1


def test_pose_planes_and_descriptor_rows():
    from diffuman4d_amd.host import pose
    sizes = [(7, 9), (16, 16), (5, 3)]
    image_off, mask_off, total = pose.plane_layout(sizes, True, [True, False, True])
    # the order of the planes: image, then its mask, each at the next multiple of 16
    assert image_off == [0, a16(189) + 64, a16(189) + 64 + 768] and mask_off == [a16(189), -1, a16(189) + 64 + 768 + 48]
    assert total == mask_off[2] + 16
    rows = [(0, 0), (1, 220), (1, 440), (2, 660)]
    desc = pose.descriptors(rows, sizes, image_off, mask_off)
    assert desc.dtype == np.int64 and desc.shape == (4, pose.FIELDS) and pose.FIELDS == 8
    for r, (k, toff) in enumerate(rows):
        assert desc[r].tolist() == [image_off[k], mask_off[k], sizes[k][0], sizes[k][1], toff, 0, 0, 0]
    assert desc[1, 1] == -1 and desc[2, 1] == -1
    # masks alone (fmask_boxes): no image plane at all
    image_off, mask_off, total = pose.plane_layout(sizes, False, [True, True, True])
    assert image_off == [-1, -1, -1] and mask_off == [0, 64, 320] and total == 336


def test_pose_open_all_checks():
    from diffuman4d_amd.host import pose
    a = np.zeros((4, 6, 3), dtype=np.uint8)
    ims, mks, sizes = pose._open_all([a, a], None, None)
    assert mks == [None, None] and sizes == [(4, 6), (4, 6)] and all(isinstance(im, Image.Image) for im in ims)
    with pytest.raises(ValueError, match="images do not match"):
        pose._open_all([a], [np.zeros((4, 5), dtype=np.uint8)], None)
    with pytest.raises(ValueError, match=r"fmasks\[1\]: mode 'RGB'"):
        pose._open_all([a, a], [None, a], None)
    with pytest.raises(ValueError, match="at least one image"):
        pose._open_all([], None, None)


# -- ops._check_meta -------------------------------------------------------------------------------------------------------------------
def _meta(n=256):
    return torch.zeros(n, dtype=torch.uint8), torch.zeros(n, dtype=torch.uint8)


def test_check_meta_accepts_what_fits():
    from diffuman4d_amd.host import ops
    meta, host = _meta()
    ops._check_meta(meta, host, 8, 3, 64)                       # 64 + 3 * 64 = 256: ends at the end
    ops._check_meta(meta, host, 8, 1, 192, tab_off=0, tab_len=48)
    ops._check_meta(meta, host, 8, 1, 0, tab_off=252, tab_len=1, what="blob")


@pytest.mark.parametrize("case", ["short host", "long host", "strided host", "int8 host", "rows 0", "desc negative", "desc odd", "desc past",
                                  "tab negative", "tab odd", "tab past", "tab empty"])
def test_check_meta_refuses(case):
    from diffuman4d_amd.host import lib as L, ops
    meta, host = _meta()
    kw = dict(fields=8, rows=2, desc_off=64, tab_off=0, tab_len=16)
    if case == "short host":
        host = host[:-1]
    elif case == "long host":
        host = torch.zeros(257, dtype=torch.uint8)
    elif case == "strided host":
        host = torch.zeros(512, dtype=torch.uint8)[::2]
    elif case == "int8 host":
        host = host.view(torch.int8)
    else:
        kw.update({"rows 0": dict(rows=0), "desc negative": dict(desc_off=-8), "desc odd": dict(desc_off=68), "desc past": dict(desc_off=136),
                   "tab negative": dict(tab_off=-4), "tab odd": dict(tab_off=2), "tab past": dict(tab_off=196), "tab empty": dict(tab_len=0)}[case])
    text = "host copy" if "host" in case else "desc_off" if case.startswith(("rows", "desc")) else "tab_off"
    with pytest.raises(L.Dm4dError, match=text):
        ops._check_meta(meta, host, kw["fields"], kw["rows"], kw["desc_off"], kw["tab_off"], kw["tab_len"])


def test_the_operators_go_through_check_meta(monkeypatch):
    """With _req out of the way (plain CPU tensors), each of the five wrappers refuses a bad meta before it reaches the library."""
    from diffuman4d_amd.host import lib as L, ops

    def no_library(*a, **k):
        raise AssertionError("refused before the library is called")
    monkeypatch.setattr(ops, "_req", lambda t, name, dtype=ops.BF16: t)
    monkeypatch.setattr(L, "call", no_library)
    blob, (meta, host) = torch.zeros(64, dtype=torch.uint8), _meta()
    lut, norm = torch.zeros(3, 256, dtype=torch.float16), torch.zeros(6)
    logits = torch.zeros(1, 1, 4, 4, dtype=torch.float16)
    calls = {
        "pose_input": lambda h, d, t: ops.pose_input(blob, meta, h, 1, d, t, 4, 8, 8, norm),
        "pose_mask_box": lambda h, d, t: ops.pose_mask_box(blob, meta, h, 1, d),
        "matting_input": lambda h, d, t: ops.matting_input(blob, meta, h, 1, d, t, 4, lut, blob, 8, 8, 0),
        "matting_mask": lambda h, d, t: ops.matting_mask(logits, meta, h, 1, d, t, 4, blob, blob, 64, 0),
        "capture_crop_resize": lambda h, d, t: ops.capture_crop_resize(blob, h, 1, d, t, 4, 8, 8, meta=meta),
    }
    for name, fn in calls.items():
        with pytest.raises(L.Dm4dError, match="host copy"):
            fn(host[:-1], 64, 0)
        with pytest.raises(L.Dm4dError, match="desc_off"):
            fn(host, 252, 0)
        if name != "pose_mask_box":  # it takes no table
            with pytest.raises(L.Dm4dError, match="tab_off"):
                fn(host, 64, 244)


# -- atomic write ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a.json", "mask.png", "noext"])
def test_atomic_write(tmp_path, name):
    from diffuman4d_amd.host.staging import atomic_write
    target = tmp_path / "sub" / "dir" / name
    seen = []

    def write(tmp, text="first"):
        seen.append(tmp)
        assert not target.exists() or target.read_text() == "first"  # the target is not touched while the file is written
        with open(tmp, "w") as f:
            f.write(text)
    atomic_write(str(target), write)
    assert target.read_text() == "first" and os.listdir(target.parent) == [name]
    tmp = seen[0]
    assert os.path.dirname(tmp) == str(target.parent) and tmp != str(target) and str(threading.get_ident()) in os.path.basename(tmp)
    ext = os.path.splitext(name)[1]
    assert not ext or os.path.splitext(tmp)[1] == ext  # Pillow picks the format by it

    def fails(tmp):
        raise RuntimeError("disk full")
    with pytest.raises(RuntimeError, match="disk full"):
        atomic_write(str(target), fails)
    assert target.read_text() == "first"  # unchanged
    atomic_write(str(target), lambda tmp: write(tmp, "second"))
    assert target.read_text() == "second" and os.listdir(target.parent) == [name]


def test_atomic_write_after_a_failure_leaves_no_target(tmp_path):
    from diffuman4d_amd.host.staging import atomic_write

    def fails(tmp):
        raise RuntimeError("no")
    with pytest.raises(RuntimeError):
        atomic_write(str(tmp_path / "x.png"), fails)
    assert not (tmp_path / "x.png").exists()


def test_atomic_write_with_pillow_and_a_bare_file_name(tmp_path, monkeypatch):
    from diffuman4d_amd.host.staging import atomic_write
    monkeypatch.chdir(tmp_path)
    im = Image.fromarray(np.arange(12, dtype=np.uint8).reshape(3, 4))
    atomic_write("m.png", im.save)
    assert os.listdir(tmp_path) == ["m.png"] and np.array_equal(np.asarray(Image.open("m.png")), np.asarray(im))


# -- size check and the rest -----------------------------------------------------------------------------------------------------------
def test_check_sizes_messages():
    from diffuman4d_amd.host import lib as L, matting, pose, staging
    assert staging.check_sizes([(np.int64(3), 4.0), (16384, 1)], 16384, "images") == [(3, 4), (16384, 1)]
    with pytest.raises(ValueError) as e:
        staging.check_sizes([(4, 4), (7, 16385)], L.POSE_MAX_SIDE, "images")
    assert str(e.value) == "images[1]: size 16385 x 7 is outside 1..16384"
    with pytest.raises(ValueError) as e:
        staging.check_sizes([(0, 4)], L.MATTING_MAX_SIDE, "sizes")
    assert str(e.value) == "sizes[0]: 4 x 0 is outside 1..16384"
    wide = Image.new("L", (16385, 1))
    with pytest.raises(ValueError) as e:  # pose's and matting's "images" message, through the modules
        pose._open_all([np.zeros((2, 2, 3), dtype=np.uint8), wide], None, None)
    assert str(e.value) == "images[1]: size 16385 x 1 is outside 1..16384"
    with pytest.raises(ValueError) as e:
        matting._open_all([wide], None)
    assert str(e.value) == "images[0]: size 16385 x 1 is outside 1..16384"


def test_open_image_and_the_shared_constant(tmp_path):
    from diffuman4d_amd.host import matting, pose, skeleton, staging, triang, vhull
    a = np.arange(24, dtype=np.uint8).reshape(2, 4, 3)
    im = Image.fromarray(a)
    im.save(tmp_path / "a.png")
    assert staging.open_image(im) is im
    for src in (a, str(tmp_path / "a.png"), tmp_path / "a.png"):
        assert np.array_equal(np.asarray(staging.open_image(src)), a)
    assert all(m.MAX_HOST_THREADS is staging.MAX_HOST_THREADS for m in (pose, matting, skeleton, triang, vhull)) and staging.MAX_HOST_THREADS == 16


def test_run_stage_refuses_a_device_that_is_not_there(monkeypatch):
    """Device resolution comes first: nothing is loaded, no pool is left behind.  (With a device: tests/test_pose_gpu.py.)"""
    from diffuman4d_amd.host import lib as L, staging
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 0)

    def never(*a):
        raise AssertionError("not reached")
    with pytest.raises(L.Dm4dError, match="^my_stage: no HIP device is available"):
        staging.run_stage("my_stage", None, 4, "dm4d-test-stage", [[0]], never, never)
    assert not [t for t in threading.enumerate() if t.name.startswith("dm4d-test-stage")]
