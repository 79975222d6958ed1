"""GPU: the two dm4d_matting_* entry points and remove_background against tests/matting_model.py (Pillow's own resize and rotate, torch
CPU arithmetic).  Every comparison is for equality: the network input bit for bit, the masks byte for byte."""
import functools
import os
import threading

import numpy as np
import pytest
import torch
from PIL import Image

import matting_model as M

pytestmark = pytest.mark.gpu

NET_SIZES = [(16, 16), (32, 24)]
IMAGE_SIZES = [(7, 9), (37, 50), (64, 64), (100, 23), (16, 16), (16, 40), (5, 5), (1, 1)]  # (h, w); one mixed batch
ROTATIONS = [0, 90, 180, 270]


def bits(t: torch.Tensor) -> np.ndarray:
    t = t.detach().cpu().contiguous()
    return t.numpy().view(np.uint16 if t.dtype == torch.float16 else np.uint32)


@functools.lru_cache(maxsize=None)
def images():
    rng = np.random.default_rng(11)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in IMAGE_SIZES]


@functools.lru_cache(maxsize=None)
def input_reference(size, rot, dtype):
    return [M.matting_input(a, size, rot, dtype) for a in images()]


@functools.lru_cache(maxsize=None)
def logits(size):
    """fp16 [n, 1, S_h, S_w], one plane per image: normal * 4, the first row of every plane +inf and the last -inf."""
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(len(IMAGE_SIZES), 1, *size, generator=g) * 4).half()
    x[:, :, 0, :] = float("inf")
    x[:, :, -1, :] = float("-inf")
    return x


@functools.lru_cache(maxsize=None)
def mask_reference(size, rot):
    return [M.matting_mask(logits(size)[k], hw, rot) for k, hw in enumerate(IMAGE_SIZES)]


# -- network input ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot", ROTATIONS)
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("size", NET_SIZES)
def test_input_is_bit_equal_to_the_model_alone_and_in_a_batch(hip_device, size, dtype, rot):
    from diffuman4d_amd.host import matting
    want = input_reference(size, rot, dtype)
    got = matting.matting_inputs(images(), size, hip_device, rotate_clockwise=rot, dtype=dtype)
    assert got.dtype == dtype and tuple(got.shape) == (len(IMAGE_SIZES), 3) + size and got.device.type == "cuda"
    for k, w in enumerate(want):
        assert np.array_equal(bits(got[k]), bits(w)), (IMAGE_SIZES[k], size, rot)
    again = matting.matting_inputs(images(), size, hip_device, rotate_clockwise=rot, dtype=dtype)
    assert np.array_equal(bits(again), bits(got))
    for k, a in enumerate(images()):
        alone = matting.matting_inputs([a], size, hip_device, rotate_clockwise=rot, dtype=dtype)
        assert np.array_equal(bits(alone[0]), bits(got[k])), (IMAGE_SIZES[k], size, rot)


def test_input_takes_paths_pil_images_and_other_modes(hip_device, tmp_path):
    from diffuman4d_amd.host import matting
    a = images()[1]
    Image.fromarray(a).save(tmp_path / "a.png")
    grey = Image.fromarray(a[..., 0])
    got = matting.matting_inputs([str(tmp_path / "a.png"), Image.fromarray(a), grey], (16, 16), hip_device)
    want = M.matting_input(a, (16, 16))
    assert np.array_equal(bits(got[0]), bits(want)) and np.array_equal(bits(got[1]), bits(want))
    assert np.array_equal(bits(got[2]), bits(M.matting_input(np.asarray(grey.convert("RGB")), (16, 16))))


# -- quantiser -------------------------------------------------------------------------------------------------------------------------
def test_quantiser_over_every_fp16_pattern(hip_device):
    from diffuman4d_amd.host import matting
    patterns = torch.from_numpy(np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).copy()).reshape(1, 1, 256, 256)
    got = matting.matting_masks(patterns.to(hip_device), [(256, 256)])  # 256 x 256 -> 256 x 256: both passes are skipped
    assert len(got) == 1 and got[0].dtype == np.uint8 and got[0].shape == (256, 256)
    assert np.array_equal(got[0], M.quantise(patterns[0, 0]).numpy())


# -- masks -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot", ROTATIONS)
@pytest.mark.parametrize("size", NET_SIZES)
def test_masks_are_byte_equal_to_the_model_alone_and_in_a_batch(hip_device, size, rot):
    from diffuman4d_amd.host import matting
    want = mask_reference(size, rot)
    x = logits(size).to(hip_device)
    got = matting.matting_masks(x, IMAGE_SIZES, rotate_clockwise=rot)
    assert len(got) == len(IMAGE_SIZES)
    for k, w in enumerate(want):
        assert got[k].dtype == np.uint8 and got[k].shape == IMAGE_SIZES[k] and np.array_equal(got[k], w), (IMAGE_SIZES[k], size, rot)
    again = matting.matting_masks(x, IMAGE_SIZES, rotate_clockwise=rot)
    assert all(np.array_equal(a, b) for a, b in zip(again, got))
    for k, hw in enumerate(IMAGE_SIZES):
        alone = matting.matting_masks(x[k: k + 1], [hw], rotate_clockwise=rot)
        assert np.array_equal(alone[0], got[k]), (hw, size, rot)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_other_logit_types_equal_their_half(hip_device, dtype):
    from diffuman4d_amd.host import matting
    g = torch.Generator().manual_seed(9)
    x = (torch.randn(len(IMAGE_SIZES), 1, 32, 24, generator=g) * 4).to(dtype)
    x[:, :, 3, :] = float("inf")
    x[:, :, 4, :] = float("-inf")
    x[:, :, 5, 0] = float("nan")
    got = matting.matting_masks(x.to(hip_device), IMAGE_SIZES)
    want = matting.matting_masks(x.half().to(hip_device), IMAGE_SIZES)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert np.array_equal(got[1], M.matting_mask(x[1].half(), IMAGE_SIZES[1]))


def test_masks_refuse_bad_arguments(hip_device):
    from diffuman4d_amd.host import matting
    x = torch.zeros(2, 1, 16, 16, dtype=torch.float16, device=hip_device)
    with pytest.raises(ValueError, match="one .h, w. per logit plane"):
        matting.matting_masks(x, [(4, 4)])
    with pytest.raises(ValueError, match=r"expected \[n, 1, S_h, S_w\]"):
        matting.matting_masks(x.reshape(1, 2, 16, 16), [(4, 4)])
    with pytest.raises(ValueError, match="outside 1..16384"):
        matting.matting_masks(x, [(4, 4), (0, 4)])
    with pytest.raises(ValueError, match="rotate_clockwise"):
        matting.matting_masks(x, [(4, 4), (4, 4)], rotate_clockwise=1)


# -- more than one workgroup along a row ----------------------------------------------------------------------------------------------
WIDE_NET = (2, 2056)                 # 514 lanes of 4 columns, 257 of 8: the second and third workgroup of a row
WIDE_SIZES = [(3, 4208), (3, 4200)]  # 263 lanes of 16 columns; a multiple of 16 (16-byte stores) and not


@pytest.mark.parametrize("rot", [0, 270])
def test_rows_wider_than_one_workgroup(hip_device, rot):
    from diffuman4d_amd.host import matting
    sizes = WIDE_SIZES if rot == 0 else [(w, h) for h, w in WIDE_SIZES]  # stored turned, so that the rotated rows are the wide ones
    rng = np.random.default_rng(13)
    wide = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    for dtype in (torch.float16, torch.float32):
        got = matting.matting_inputs(wide, WIDE_NET, hip_device, rotate_clockwise=rot, dtype=dtype)
        for k, a in enumerate(wide):
            assert np.array_equal(bits(got[k]), bits(M.matting_input(a, WIDE_NET, rot, dtype))), (sizes[k], dtype)
    x = (torch.randn(len(sizes), 1, *WIDE_NET, generator=torch.Generator().manual_seed(3)) * 4).half()
    masks = matting.matting_masks(x.to(hip_device), sizes, rotate_clockwise=rot)
    for k, hw in enumerate(sizes):
        assert np.array_equal(masks[k], M.matting_mask(x[k], hw, rot)), hw


# -- network sizes that are no multiple of a lane's columns: the scalar stores ------------------------------------------------------------
@pytest.mark.parametrize("rot", [0, 90])
@pytest.mark.parametrize("size", [(9, 13), (6, 12)])  # 13: no multiple of 4; 12: whole 16-byte scratch and fp32 stores, half an fp16 one
def test_odd_network_sizes(hip_device, size, rot):
    from diffuman4d_amd.host import matting
    for dtype in (torch.float16, torch.float32):
        got = matting.matting_inputs(images(), size, hip_device, rotate_clockwise=rot, dtype=dtype)
        for k, a in enumerate(images()):
            assert np.array_equal(bits(got[k]), bits(M.matting_input(a, size, rot, dtype))), (IMAGE_SIZES[k], size, dtype)
    x = (torch.randn(len(IMAGE_SIZES), 1, *size, generator=torch.Generator().manual_seed(4)) * 4).half()
    masks = matting.matting_masks(x.to(hip_device), IMAGE_SIZES, rotate_clockwise=rot)
    for k, hw in enumerate(IMAGE_SIZES):
        assert np.array_equal(masks[k], M.matting_mask(x[k], hw, rot)), (hw, size)


# -- the stage -------------------------------------------------------------------------------------------------------------------------
def _scene(tmp_path):
    paths = []
    for k, a in enumerate(images()):
        path = tmp_path / "images" / f"{k % 3:02d}" / f"{k:06d}.webp"
        path.parent.mkdir(parents=True, exist_ok=True)
        Image.fromarray(a).save(path, lossless=True, exact=True)
        assert np.array_equal(np.asarray(Image.open(path).convert("RGB")), a)
        paths.append(path)
    return paths


@pytest.mark.parametrize("rot", [0, 90])
def test_remove_background_end_to_end(hip_device, tmp_path, rot):
    from diffuman4d_amd.host import lib as L, matting
    paths = _scene(tmp_path)
    images_dir, out, alpha = str(tmp_path / "images"), str(tmp_path / "fmasks"), str(tmp_path / "rgba")
    seen = []

    def model(x):
        seen.append((x.dtype, tuple(x.shape), x.device.type))
        return [x, x[:, :1] * 4]  # a list whose last entry is taken; scaling fp16 by 4 is exact
    res = matting.remove_background(images_dir, out, alpha, rotate_clockwise=rot, batch_size=3, matting_model=model, image_size=(16, 16), gpu_ids=[0])
    assert res == {"images": 8, "written": 8, "skipped": 0}
    assert sorted(s[1][0] for s in seen) == [2, 3, 3] and all(s[0] == torch.float16 and s[1][1:] == (3, 16, 16) and s[2] == "cuda" for s in seen)
    for k, (path, a) in enumerate(zip(paths, images())):
        want = M.matting_mask(M.matting_input(a, (16, 16), rot)[0:1] * 4, IMAGE_SIZES[k], rot)
        fmask = Image.open(tmp_path / "fmasks" / path.parent.name / (path.stem + ".png"))
        assert fmask.mode == "L" and np.array_equal(np.asarray(fmask), want), (IMAGE_SIZES[k], rot)
        rgba = Image.open(tmp_path / "rgba" / path.parent.name / (path.stem + ".png"))
        assert rgba.mode == "RGBA" and np.array_equal(np.asarray(rgba)[..., :3], a) and np.array_equal(np.asarray(rgba)[..., 3], want)
    files = sorted(p for p in (tmp_path / "fmasks").rglob("*"))
    assert len([p for p in files if p.is_file()]) == 8 and all(".tmp" not in p.name for p in files)
    stamps = {p: os.stat(p).st_mtime_ns for p in files if p.is_file()}

    def never(x):
        raise AssertionError("every mask exists and verifies")
    res = matting.remove_background(images_dir, out, alpha, rotate_clockwise=rot, batch_size=3, matting_model=never, image_size=(16, 16),
                                    skip_exists=True, gpu_ids=[0])
    assert res == {"images": 8, "written": 0, "skipped": 8} and stamps == {p: os.stat(p).st_mtime_ns for p in stamps}
    with pytest.raises(L.Dm4dError, match="on the device"):
        matting.remove_background(images_dir, out, matting_model=lambda x: x[:, :1].cpu(), image_size=(16, 16), gpu_ids=[0])
    with pytest.raises(L.Dm4dError, match="on the device"):
        matting.remove_background(images_dir, out, matting_model=lambda x: x, image_size=(16, 16), gpu_ids=[0])  # three channels


def test_remove_background_with_two_workers_equals_one(hip_device, tmp_path):
    """The stage driver (host/staging.py run_stage) with two worker threads on one device, one image per batch: the same files byte for
    byte as with one worker; skip_exists then writes nothing; a network that fails in one worker reaches the caller and leaves no thread."""
    from diffuman4d_amd.host import matting
    rng = np.random.default_rng(17)
    for k, (h, w) in enumerate([(5, 7), (16, 16), (33, 20)]):
        path = tmp_path / "images" / "00" / f"{k:06d}.webp"
        path.parent.mkdir(parents=True, exist_ok=True)
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(path, lossless=True, exact=True)

    def run(out, gpu_ids, skip_exists, model=lambda x: [x, x[:, :1] * 4]):
        return matting.remove_background(str(tmp_path / "images"), str(tmp_path / out), str(tmp_path / (out + "_rgba")), batch_size=1,
                                         num_workers=2, skip_exists=skip_exists, gpu_ids=gpu_ids, matting_model=model, image_size=(16, 24))
    assert run("one", [0], False) == {"images": 3, "written": 3, "skipped": 0}
    assert run("two", [0, 0], False) == {"images": 3, "written": 3, "skipped": 0}
    for d in ("one", "one_rgba"):
        files = sorted(p.relative_to(tmp_path / d) for p in (tmp_path / d).rglob("*") if p.is_file())
        other = tmp_path / d.replace("one", "two")
        assert len(files) == 3 and files == sorted(p.relative_to(other) for p in other.rglob("*") if p.is_file())
        for f in files:
            assert (tmp_path / d / f).read_bytes() == (other / f).read_bytes(), f
    assert run("two", [0, 0], True) == {"images": 3, "written": 0, "skipped": 3}

    def fails_in_the_second_worker(x):
        if threading.current_thread().name.endswith("gpu_1"):
            raise RuntimeError("the network fails")
        return x[:, :1]
    with pytest.raises(RuntimeError, match="the network fails"):
        run("three", [0, 0], False, fails_in_the_second_worker)
    assert len([p for p in (tmp_path / "three").rglob("*.png")]) == 2  # the first worker's batches, 0 and 2, were written
    assert not [t.name for t in threading.enumerate() if t.name.startswith("dm4d-matting")]


def test_there_is_no_cpu_path(hip_device):
    from diffuman4d_amd.host import lib as L, matting
    with pytest.raises(L.Dm4dError, match="no CPU fallback"):
        matting.matting_inputs(images(), (16, 16), device="cpu")
    with pytest.raises(L.Dm4dError, match="no CPU fallback"):
        matting.matting_masks(logits((16, 16)), IMAGE_SIZES)
