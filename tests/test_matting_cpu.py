"""CPU: the foreground-mask stage's definition (tests/matting_model.py) against Pillow and torch CPU, the host side of
diffuman4d_amd/host/matting.py (tables, paths, skip_exists, errors), the argument checks of the two dm4d_matting_* entry points, which
return DM4D_ERR_ARG before anything is launched (fake aligned "device" addresses that are never dereferenced, real host tables), and
the driver tools/preprocess.py with recorders in place of the stages.  Every comparison is for equality."""
import ctypes
import importlib.util
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image

import matting_model as M

ROOT = Path(__file__).resolve().parent.parent
P = 0x10000
ERR_ARG = -1
IMAGE_SIZES = [(7, 9), (37, 50), (64, 64), (100, 23), (16, 40), (5, 5), (77, 130)]
NET_SIZES = [(16, 16), (24, 24), (32, 32), (32, 24)]
# both passes skipped, one pass skipped (either axis), and a single pixel
EXTRA = [((16, 16), (16, 16)), ((32, 24), (32, 24)), ((16, 40), (16, 16)), ((9, 16), (16, 16)), ((32, 7), (32, 24)), ((1, 1), (16, 16)),
         ((1, 1), (32, 24))]


def image(h, w, seed=0, channels=3):
    rng = np.random.default_rng(1000 * h + w + seed)
    return rng.integers(0, 256, (h, w, channels) if channels else (h, w), dtype=np.uint8)


# -- tables against Pillow ---------------------------------------------------------------------------------------------------------------
def test_bilinear_table_reproduces_pillow():
    from diffuman4d_amd.host import resample
    for (h, w), (S_h, S_w) in [(i, n) for i in IMAGE_SIZES for n in NET_SIZES] + EXTRA:
        a = image(h, w)
        want = np.asarray(Image.fromarray(a).resize((S_w, S_h), Image.BILINEAR))
        assert np.array_equal(M.table_resize(a, (S_h, S_w), resample.bilinear_table), want), ((h, w), (S_h, S_w))


def test_bicubic_table_reproduces_pillows_default_resize_of_an_L_plane():
    from diffuman4d_amd.host import resample
    for (h, w), (S_h, S_w) in [(i, n) for i in IMAGE_SIZES for n in NET_SIZES] + EXTRA:
        a = image(S_h, S_w, seed=7, channels=0)
        want = np.asarray(Image.fromarray(a).resize((w, h)))
        assert np.array_equal(M.table_resize(a, (h, w), resample.bicubic_table), want), ((S_h, S_w), (h, w))


def _parent_bicubic_table(in_size, out_size):
    """host/resample.py::bicubic_table as it stood before the bilinear filter joined it, restated."""
    import math

    def kernel(x):
        x = np.abs(x)
        near = ((1.5 * x - 2.5) * x) * x + 1.0
        far = (((x - 5.0) * x + 8.0) * x - 4.0) * -0.5
        return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    lo = np.maximum(np.trunc(center - support + 0.5), 0).astype(np.int64)
    hi = np.minimum(np.trunc(center + support + 0.5), in_size).astype(np.int64)
    n = hi - lo
    t = np.arange(ksize)
    w = kernel(((t[None, :] + lo[:, None]) - center[:, None] + 0.5) * (1.0 / fs))
    w = np.where(t[None, :] < n[:, None], w, 0.0)
    total = np.zeros(out_size)
    for j in range(ksize):
        total = total + w[:, j]
    w = np.where(total[:, None] != 0.0, w / np.where(total == 0.0, 1.0, total)[:, None], w)
    scaled = w * float(1 << 22)
    k = np.trunc(np.where(w < 0, -0.5 + scaled, 0.5 + scaled)).astype(np.int32)
    return np.stack([lo, n], axis=1).astype(np.int32), k


def test_bicubic_table_is_unchanged():
    from diffuman4d_amd.host import capture, resample
    assert capture.bicubic_table is resample.bicubic_table
    for pair in [(1400, 1024), (37, 50), (1024, 2448)]:
        (b, k), (b0, k0) = resample.bicubic_table(*pair), _parent_bicubic_table(*pair)
        assert b.dtype == b0.dtype and k.dtype == k0.dtype and np.array_equal(b, b0) and np.array_equal(k, k0)
    ts = resample.TableSet()
    assert ts.add(37, 50) == (0, 5) and list(ts.tables) == [(37, 50)]       # existing callers: the same keys and offsets
    off, ks = ts.add(37, 50, "bilinear")
    assert off == 50 * 7 and list(ts.tables)[1] == (37, 50, "bilinear") and ts.add(37, 50) == (0, 5)
    b, k = resample.bilinear_table(37, 50)
    assert ks == k.shape[1] and np.array_equal(ts.array()[off:], np.concatenate([b.reshape(-1), k.reshape(-1)]))


# -- the two value tables ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_normalisation_table_equals_the_model(dtype):
    from diffuman4d_amd.host import matting
    assert matting.MEAN == tuple(M.MEAN) and matting.STD == tuple(M.STD)
    rng = np.random.default_rng(3)
    a = np.stack([rng.permutation(256).reshape(16, 16) for _ in range(3)], axis=-1).astype(np.uint8)  # every byte once per channel
    want = M.matting_input(a, (16, 16), 0, dtype)
    lut = matting.normalisation_table(dtype)
    assert lut.dtype == dtype and lut.shape == (3, 256) and want.dtype == dtype
    got = torch.stack([lut[c][torch.from_numpy(a[..., c].astype(np.int64))] for c in range(3)])
    assert torch.equal(got, want)
    with pytest.raises(ValueError, match="dtype"):
        matting.normalisation_table(torch.bfloat16)


def test_quantiser_definition():
    from diffuman4d_amd.host import matting
    bits = torch.from_numpy(np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).copy())  # every fp16 pattern, by index
    q = M.quantise(bits).numpy()
    assert np.array_equal(matting.quantiser_table(), q)  # the host's table (numpy) and the model (torch, fp64): two routes, one map
    x = bits.double().numpy()
    finite = ~np.isnan(x)
    order = np.argsort(x[finite], kind="stable")
    in_order = q[finite][order]
    assert np.all(np.diff(in_order.astype(np.int64)) >= 0)  # monotone in value order
    assert set(np.unique(q).tolist()) == set(range(256))      # and onto
    half = lambda v: int(np.array(v, dtype=np.float16).view(np.uint16))
    assert q[half(-np.inf)] == 0 and q[half(np.inf)] == 255 and q[half(0.0)] == 127 and np.all(q[~finite] == 0) and (~finite).sum() == 2046
    torch_own = bits.sigmoid().mul(255).to(torch.uint8).numpy()
    differs = int((torch_own[finite] != q[finite]).sum())
    print(f"quantiser: differs from torch CPU's fp16 sigmoid().mul(255).byte() on {differs} of {int(finite.sum())} non-NaN patterns")
    assert differs <= 1


def test_rotation_by_hand():
    a = np.arange(18, dtype=np.uint8).reshape(2, 3, 3)
    p = a[..., 0] // 3  # pixel numbers 0..5: [[0, 1, 2], [3, 4, 5]]
    by_hand = {0: [[0, 1, 2], [3, 4, 5]], 90: [[3, 0], [4, 1], [5, 2]], 180: [[5, 4, 3], [2, 1, 0]], 270: [[2, 5], [1, 4], [0, 3]]}
    for angle, want in by_hand.items():
        got = np.asarray(M.rotated(Image.fromarray(a), angle))
        assert np.array_equal(got[..., 0] // 3, np.array(want)) and np.array_equal(got, np.rot90(a, -(angle // 90)))
        assert np.array_equal(np.asarray(Image.fromarray(a).rotate(-angle, expand=True)), got)
        back = np.asarray(Image.fromarray(got).rotate(angle, expand=True))  # the way the mask goes
        assert np.array_equal(back, a)
    assert p.tolist() == by_hand[0]


# -- paths, skip_exists, errors ---------------------------------------------------------------------------------------------------------
def _scene(tmp_path, n=5):
    for k in range(n):
        path = tmp_path / "images" / f"{k % 2:02d}" / f"{k:06d}.webp"
        path.parent.mkdir(parents=True, exist_ok=True)
        Image.fromarray(image(6, 5, seed=k)).save(path, lossless=True)
    return str(tmp_path / "images")


def test_paths_and_skip_exists(tmp_path):
    from diffuman4d_amd.host import lib as L, matting
    images_dir = _scene(tmp_path)
    out, alpha = str(tmp_path / "fmasks"), str(tmp_path / "rgba")
    images, fmasks, alphas = matting.list_inputs(images_dir, out, alpha)
    assert [os.path.relpath(p, images_dir) for p in images] == ["00/000000.webp", "00/000002.webp", "00/000004.webp", "01/000001.webp", "01/000003.webp"]
    assert [os.path.relpath(p, out) for p in fmasks] == [r.replace(".webp", ".png") for r in (os.path.relpath(p, images_dir) for p in images)]
    assert alphas[3] == os.path.join(alpha, "01", "000001.png") and matting.list_inputs(images_dir, out)[2] == [None] * 5
    assert matting.list_inputs(images_dir, out, image_ext=".jpg")[0] == []
    assert matting.pending_batches(fmasks, 2, False) == ([[0, 1], [2, 3], [4]], 0)
    assert matting.pending_batches(fmasks, 2, True) == ([[0, 1], [2, 3], [4]], 0)  # nothing exists yet
    for p in fmasks:
        matting.write_mask(image(6, 5, channels=0), p)
    assert not [f for f in os.listdir(os.path.dirname(fmasks[0])) if "tmp" in f]
    assert matting.pending_batches(fmasks, 2, True) == ([], 5)

    def model(x):
        raise AssertionError("every mask exists and verifies: nothing to predict")
    assert matting.remove_background(images_dir, out, matting_model=model, batch_size=2, skip_exists=True) == {"images": 5, "written": 0, "skipped": 5}
    os.remove(fmasks[3])                      # one missing mask reruns its whole batch, and only that one
    assert matting.pending_batches(fmasks, 2, True) == ([[2, 3]], 3)
    data = open(fmasks[0], "rb").read()
    with open(fmasks[0], "wb") as f:          # present but truncated: not "existing"
        f.write(data[: len(data) // 2])
    assert matting.pending_batches(fmasks, 2, True) == ([[0, 1], [2, 3]], 1)
    assert matting.pending_batches(fmasks, 8, True) == ([[0, 1, 2, 3, 4]], 0)
    # the stage then goes on to the device, of which gpu_ids=[] names none; without skip_exists it does so at once
    with pytest.raises(L.Dm4dError, match="no HIP device"):
        matting.remove_background(images_dir, out, matting_model=model, batch_size=2, skip_exists=True, gpu_ids=[])
    with pytest.raises(L.Dm4dError, match="no HIP device"):
        matting.remove_background(images_dir, out, matting_model=model, gpu_ids=[])


def test_write_mask_with_alpha(tmp_path):
    from diffuman4d_amd.host import matting
    a, m = image(6, 5), image(6, 5, channels=0)
    matting.write_mask(m, str(tmp_path / "f" / "0.png"), a, str(tmp_path / "a" / "0.png"))
    rgba = Image.open(tmp_path / "a" / "0.png")
    assert rgba.mode == "RGBA" and np.array_equal(np.asarray(rgba)[..., :3], a) and np.array_equal(np.asarray(rgba)[..., 3], m)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "f" / "0.png")), m)


def test_errors(tmp_path):
    from diffuman4d_amd.host import lib as L, matting
    images_dir = _scene(tmp_path, 1)
    out = str(tmp_path / "fmasks")
    with pytest.raises(ValueError, match="rotate_clockwise must be one of 0, 90, 180, 270"):
        matting.remove_background(images_dir, out, matting_model=lambda x: x, rotate_clockwise=45)
    with pytest.raises(ValueError, match="rotate_clockwise"):
        matting.matting_inputs([image(4, 4)], (16, 16), rotate_clockwise=45)
    with pytest.raises(ValueError, match="name the matting network"):
        matting.remove_background(images_dir, out)
    with pytest.raises(FileNotFoundError, match="never downloaded"):
        matting.remove_background(images_dir, out, model_name="ZhengPeng7/BiRefNet")
    with pytest.raises(FileNotFoundError, match="never downloaded"):
        matting.load_matting_model(str(tmp_path / "fmasks" / "absent"), "cpu")
    with pytest.raises(ValueError, match="at least one image"):
        matting.matting_inputs([], (16, 16))
    with pytest.raises(ValueError, match="dtype"):
        matting.matting_inputs([image(4, 4)], (16, 16), dtype=torch.bfloat16)
    with pytest.raises(L.Dm4dError, match="no CPU fallback"):
        matting.matting_inputs([image(4, 4)], (16, 16), device="cpu")
    with pytest.raises(L.Dm4dError, match="no CPU fallback"):
        matting.matting_masks(torch.zeros(1, 1, 16, 16, dtype=torch.float16), [(4, 4)])


def test_a_hub_name_is_refused_before_transformers_is_imported():
    code = ("import sys\n"
            "from diffuman4d_amd.host import matting\n"
            "try:\n"
            "    matting.load_matting_model('ZhengPeng7/BiRefNet', 'cpu')\n"
            "except FileNotFoundError as e:\n"
            "    assert 'never downloaded' in str(e), str(e)\n"
            "else:\n"
            "    raise SystemExit('no FileNotFoundError')\n"
            "assert 'transformers' not in sys.modules\n"
            "print('refused')\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(ROOT)] + [p for p in [os.environ.get("PYTHONPATH")] if p]))
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=str(ROOT))
    assert res.returncode == 0 and res.stdout.strip() == "refused", res.stderr


# -- the C entry points ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from diffuman4d_amd.host import lib as L
    return L.load()


def last(lib):
    return lib.dm4d_last_error().decode()


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _plan(to_net, sizes=((7, 9), (37, 50)), net=(16, 16), rot=0):
    from diffuman4d_amd.host import matting
    return matting._plan(list(sizes), net, rot, to_net)


def call_input(lib, desc, tab, plane_bytes, scratch_bytes, n=None, net=(16, 16), rot=0, out=P, scratch=P, lut=P, f32=0):
    desc, tab = np.ascontiguousarray(desc, dtype=np.int64), np.ascontiguousarray(tab, dtype=np.int32)
    return lib.dm4d_matting_input_u8(None, P, plane_bytes, ptr(desc), P, len(desc) if n is None else n, ptr(tab), P, len(tab), lut, scratch,
                                     scratch_bytes, out, net[0], net[1], rot, f32)


def call_mask(lib, desc, tab, plane_bytes, scratch_bytes, n=None, net=(16, 16), rot=0, blob=P, logits=P):
    desc, tab = np.ascontiguousarray(desc, dtype=np.int64), np.ascontiguousarray(tab, dtype=np.int32)
    return lib.dm4d_matting_mask_f16_u8(None, logits, ptr(desc), P, len(desc) if n is None else n, ptr(tab), P, len(tab), P, P, scratch_bytes, blob,
                                        plane_bytes, net[0], net[1], rot)


@pytest.mark.parametrize("to_net", [True, False])
def test_entry_points_reject_bad_arguments(lib, to_net):
    desc, tab, plane_bytes, scratch_bytes = _plan(to_net)
    call = call_input if to_net else call_mask
    what = "matting_input" if to_net else "matting_mask"

    def bad(row, field, value):
        d = desc.copy()
        d[row, field] = value
        return d
    if to_net:
        assert lib.dm4d_matting_input_u8(None, None, 1, None, P, 1, None, P, 1, P, P, 1, P, 16, 16, 0, 0) == ERR_ARG and "null" in last(lib)
        assert call(lib, desc, tab, plane_bytes, scratch_bytes, lut=None) == ERR_ARG and "null" in last(lib)
        assert call(lib, desc, tab, plane_bytes, scratch_bytes, out=P + 8) == ERR_ARG and "aligned" in last(lib)
    else:
        assert lib.dm4d_matting_mask_f16_u8(None, None, None, P, 1, None, P, 1, P, P, 1, P, 1, 16, 16, 0) == ERR_ARG and "null" in last(lib)
        assert call(lib, desc, tab, plane_bytes, scratch_bytes, blob=None) == ERR_ARG and "null" in last(lib)
        assert call(lib, desc, tab, plane_bytes, scratch_bytes, blob=P + 8) == ERR_ARG and "aligned" in last(lib)
        assert call(lib, bad(1, 0, desc[1, 0] + 4), tab, plane_bytes + 16, scratch_bytes) == ERR_ARG and "image 1: mask offset is not 16-byte aligned" in last(lib)
    assert last(lib).startswith(what)
    for n in (0, -1, 65536):
        assert call(lib, desc, tab, plane_bytes, scratch_bytes, n=n) == ERR_ARG and "n outside 1..65535" in last(lib)
    assert call(lib, desc, tab, plane_bytes, scratch_bytes, net=(0, 16)) == ERR_ARG and "size outside 1..16384" in last(lib)
    assert call(lib, desc, tab, plane_bytes, scratch_bytes, net=(16, 16385)) == ERR_ARG and "size outside 1..16384" in last(lib)
    for rot in (-1, 4):
        assert call(lib, desc, tab, plane_bytes, scratch_bytes, rot=rot) == ERR_ARG and "rot outside 0..3" in last(lib)
    # a plane outside its buffer: by its offset, and by a buffer one byte short
    outside = "image outside the staging buffer" if to_net else "mask outside the blob"
    assert call(lib, bad(1, 0, plane_bytes), tab, plane_bytes, scratch_bytes) == ERR_ARG and f"image 1: {outside}" in last(lib)
    assert call(lib, bad(0, 0, -16), tab, plane_bytes, scratch_bytes) == ERR_ARG and f"image 0: {outside}" in last(lib)
    short = int(desc[1, 0]) + 37 * 50 * (3 if to_net else 1) - 1
    assert call(lib, desc, tab, short, scratch_bytes) == ERR_ARG and f"image 1: {outside}" in last(lib)
    # sizes
    for field in (1, 2):
        for value in (0, -3, 16385):
            assert call(lib, bad(0, field, value), tab, plane_bytes, scratch_bytes) == ERR_ARG and "image 0: image size outside 1..16384" in last(lib)
    # tables: missing, superfluous, outside tab, a window that leaves its axis
    assert call(lib, bad(0, 3, -1), tab, plane_bytes, scratch_bytes) == ERR_ARG and "needs a table" in last(lib)
    assert call(lib, bad(1, 5, -1), tab, plane_bytes, scratch_bytes) == ERR_ARG and "needs a table" in last(lib)
    assert call(lib, bad(0, 3, len(tab) - 3), tab, plane_bytes, scratch_bytes) == ERR_ARG and "horizontal table" in last(lib)
    assert call(lib, bad(0, 6, 0), tab, plane_bytes, scratch_bytes) == ERR_ARG and "vertical table" in last(lib)
    n_out_h = 16 if to_net else 9
    t = tab.copy()
    t[desc[0, 3] + 2 * (n_out_h - 1)] += 1          # the last horizontal window of image 0 now ends one past its axis
    assert call(lib, desc, t, plane_bytes, scratch_bytes) == ERR_ARG and "image 0: the horizontal table is out of range or a window leaves its axis" in last(lib)
    t = tab.copy()
    t[desc[1, 5]] = -1                               # the first vertical window of image 1 starts before its axis
    assert call(lib, desc, t, plane_bytes, scratch_bytes) == ERR_ARG and "image 1: the vertical table" in last(lib)
    # scratch
    assert call(lib, desc, tab, plane_bytes, scratch_bytes - 16) == ERR_ARG and "image 1: scratch region" in last(lib)
    assert call(lib, bad(0, 7, 8), tab, plane_bytes, scratch_bytes + 16) == ERR_ARG and "image 0: scratch region" in last(lib)
    # an image of the network's own size takes no table; naming one is refused too
    d1, t1, p1, s1 = _plan(to_net, sizes=((16, 16),))
    assert d1[0, 3] == -1 and d1[0, 5] == -1 and len(t1) == 1
    d1[0, 3], d1[0, 4] = 0, 1
    assert call(lib, d1, t1, p1, s1) == ERR_ARG and "keeps it none" in last(lib)
    # a quarter turn swaps the axes the tables belong to: the unrotated plan is refused under rot = 1
    if to_net:
        assert call(lib, desc, tab, plane_bytes, scratch_bytes, rot=1) == ERR_ARG and "image 0: the horizontal table" in last(lib)


def test_plan_offsets():
    from diffuman4d_amd.host import matting
    for to_net in (True, False):
        for rot in range(4):
            desc, tab, plane_bytes, scratch_bytes = matting._plan([(7, 9), (16, 16), (16, 40), (1, 1)], (16, 16), rot, to_net)
            bpp = 3 if to_net else 1
            assert desc[:, 0].tolist() == [0, 16 * ((7 * 9 * bpp + 15) // 16), 16 * ((7 * 9 * bpp + 15) // 16) + 256 * bpp,
                                           16 * ((7 * 9 * bpp + 15) // 16) + 256 * bpp + 640 * bpp]
            assert plane_bytes % 16 == 0 and np.all(desc[:, 7] % 16 == 0) and desc[1, 3] == -1 and desc[1, 5] == -1
            rw40 = 16 if rot & 1 else 40   # (16, 40): rotated by a quarter turn it is 40 x 16, and the other axis keeps its size
            assert (desc[2, 3] < 0) == (rw40 == 16) and (desc[2, 5] < 0) == (rw40 != 16)


def test_abi_tables_hold_the_new_surface():
    from test_abi import header_constants, header_functions
    from diffuman4d_amd.host import lib as L, ops
    fns = header_functions()
    for name, n_args in (("dm4d_matting_input_u8", 17), ("dm4d_matting_mask_f16_u8", 16)):
        assert fns[name] == n_args and len(L.SIGNATURES[name][1]) == n_args
    consts = header_constants()
    for name, value in (("MATTING_FIELDS", 8), ("MATTING_MAX_SIDE", 16384)):
        assert int(consts[name]) == value == getattr(L, name)
    assert callable(ops.matting_input) and callable(ops.matting_mask)


# -- tools/preprocess.py -------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def driver(monkeypatch):
    spec = importlib.util.spec_from_file_location("dm4d_tools_preprocess", ROOT / "tools" / "preprocess.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    calls = []

    def recorder(name):
        def stage(*args, **kw):
            calls.append((name, args, kw))
            if name == "carve_vhull":
                os.makedirs(args[2], exist_ok=True)
                with open(os.path.join(args[2], "000000.ply"), "wb") as f:
                    f.write(b"ply of frame 0")
            return {"stage": name}
        return stage
    monkeypatch.setattr(mod, "STAGES", {name: recorder(name) for name in mod.STAGES})
    return mod, calls


def test_preprocess_runs_the_reference_order_and_directories(driver, tmp_path, capsys):
    mod, calls = driver
    d = str(tmp_path)
    assert mod.ALL_ACTIONS == ("remove_background", "carve_vhull", "predict_keypoints", "triangulate_skeleton", "draw_skeleton")
    assert mod.main(["--data_dir", d, "--matting_model_dir", "M", "--sapiens_ckpt_path", "S", "--palette", "P"]) == 0
    assert [c[0] for c in calls] == list(mod.ALL_ACTIONS)
    assert calls[0][1] == (f"{d}/images", f"{d}/fmasks") and calls[0][2] == {"model_name": "M", "batch_size": 8}
    assert calls[1][1] == (f"{d}/fmasks", f"{d}/transforms.json", f"{d}/surfs")
    assert calls[2][1] == (f"{d}/images", f"{d}/poses_sapiens", f"{d}/fmasks", "S")
    assert calls[3][1] == (f"{d}/transforms.json", f"{d}/poses_sapiens", f"{d}/poses_3d")
    assert calls[3][2] == {"out_pcd_dir": f"{d}/poses_pcd", "out_kp2d_proj_dir": f"{d}/poses_2d"}
    assert calls[4][1] == (f"{d}/poses_2d", f"{d}/skeletons") and calls[4][2] == {"palette": "P"}
    assert open(tmp_path / "sparse_pcd.ply", "rb").read() == b"ply of frame 0"
    assert capsys.readouterr().out.count('"action"') == 5


def test_preprocess_runs_a_subset_in_the_given_order(driver, tmp_path):
    mod, calls = driver
    assert mod.main(["--data_dir", str(tmp_path), "--actions", "triangulate_skeleton,carve_vhull"]) == 0
    assert [c[0] for c in calls] == ["triangulate_skeleton", "carve_vhull"] and (tmp_path / "sparse_pcd.ply").exists()
    assert mod.parse_actions("draw_skeleton, carve_vhull") == ["draw_skeleton", "carve_vhull"] and mod.parse_actions(None) == list(mod.ALL_ACTIONS)


def test_preprocess_refuses_an_unknown_action_before_any_stage_runs(driver, tmp_path, capsys):
    mod, calls = driver
    with pytest.raises(ValueError, match="Invalid action: carve_hull"):
        mod.parse_actions("carve_vhull,carve_hull")
    with pytest.raises(SystemExit) as e:
        mod.main(["--data_dir", str(tmp_path), "--actions", "carve_vhull,carve_hull"])
    assert e.value.code == 2 and "Invalid action: carve_hull" in capsys.readouterr().err
    with pytest.raises(SystemExit):  # a stage whose file was not named is refused up front as well
        mod.main(["--data_dir", str(tmp_path), "--actions", "carve_vhull,remove_background"])
    assert calls == [] and not (tmp_path / "sparse_pcd.ply").exists()
