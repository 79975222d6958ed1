"""CPU: the keypoint stage's model (tests/pose_model.py) against Pillow and its own sanity bounds, the host side of
diffuman4d_amd/host/pose.py (tables, JSON, paths, errors), and the argument checks of the three dm4d_pose_* entry points, which return
DM4D_ERR_ARG before anything is launched (fake aligned "device" addresses that are never dereferenced, real host tables)."""
import ctypes
import json
import os

import numpy as np
import pytest
from PIL import Image

import pose_cases
import pose_model as M

P = 0x10000
ERR_ARG = -1


# -- the model -------------------------------------------------------------------------------------------------------------------------
def test_composite_equals_pillow_for_every_pair():
    p, m = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8))
    image = Image.fromarray(np.stack([p, p, p], axis=-1))
    want = np.asarray(Image.composite(image, Image.new("RGB", image.size, (0, 0, 0)), Image.fromarray(m)))
    got = M.composite(np.stack([p, p, p], axis=-1), m[..., None])
    assert np.array_equal(got, want)
    one = Image.fromarray(m >= 128)  # mode "1": staged as its "L" conversion
    assert one.mode == "1"
    want1 = np.asarray(Image.composite(image, Image.new("RGB", image.size, (0, 0, 0)), one))
    assert np.array_equal(M.composite(np.stack([p, p, p], axis=-1), np.asarray(one.convert("L"))[..., None]), want1)


def test_weight_table():
    tab = M.weight_table()
    assert tab.shape == (32, 32, 4) and np.all(tab.sum(axis=-1) == 32768) and tab.min() >= 0
    assert tab[0, 0].tolist() == [32768, 0, 0, 0]
    assert tab[0, 16].tolist() == [16384, 16384, 0, 0] and tab[16, 0].tolist() == [16384, 0, 16384, 0]


def test_warp_of_the_identity_box_returns_the_image():
    """UDP maps the box's corners onto the first and last pixel CENTRES of the output, so the box that is 'equal to the image' at an
    equal output size is the one through the image's corner pixel centres, [0, 0, w - 1, h - 1]: scale (W - 1) / (w - 1) = 1.  The
    aspect fix keeps that box only where (w - 1) / (h - 1) = w / h, a square image; for the others the same centre and scale are
    given to the matrix directly."""
    rng = np.random.default_rng(0)
    for h, w in [(8, 8), (7, 9), (32, 24)]:
        image = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        center, scale = np.array([(w - 1) / 2, (h - 1) / 2]), np.array([w - 1.0, h - 1.0])
        if h == w:
            c, s = M.center_scale([0, 0, w - 1, h - 1], (h, w), padding=1.0)
            assert np.array_equal(c, center) and np.array_equal(s, scale)
        mat = M.udp_matrix(center, scale, (h, w))
        assert np.array_equal(mat, np.array([[1, 0, 0], [0, 1, 0]], dtype=np.float32))
        assert np.array_equal(M.warp(image, None, M.warp_tables(mat, (h, w)), (h, w)), image)
        ramp = np.tile(np.arange(w, dtype=np.uint8) * 9, (h, 1))
        assert np.array_equal(M.warp(image, ramp, M.warp_tables(mat, (h, w)), (h, w)), M.composite(image, ramp[..., None]))


def test_box_geometry_by_hand():
    """Centre, scale and matrix against values worked out by hand, and the matrix by what it must do: send the box's two corners to the
    first and the last pixel centre of the network input.  Shares no code with the host."""
    c, s = M.center_scale([10, 20, 50, 40], (32, 24))  # 40 x 20 padded to 50 x 25, wider than 3 : 4 -> the height grows to 50 / 0.75
    assert c.tolist() == [30.0, 30.0] and s[0] == 50.0 and abs(s[1] - 200 / 3) < 1e-12
    c, s = M.center_scale([0, 0, 30, 80], (32, 24))    # 30 x 80 padded to 37.5 x 100, narrower than 3 : 4 -> the width grows to 75
    assert c.tolist() == [15.0, 40.0] and s.tolist() == [75.0, 100.0]
    c, s = M.center_scale([0, 0, 30, 40], (32, 24), padding=1.0)
    assert s.tolist() == [30.0, 40.0]
    for box, shape in [([10, 20, 50, 40], (32, 24)), ([3.3, 2.2, 40.7, 30.1], (40, 28)), ([-20, -10, 80, 60], (1024, 768))]:
        c, s = M.center_scale(box, shape)
        m = M.udp_matrix(c, s, shape).astype(np.float64)
        assert m[0, 1] == 0 and m[1, 0] == 0
        first, last = m @ np.append(c - s / 2, 1), m @ np.append(c + s / 2, 1)
        tol = 2.0 ** -22 * max(shape) * (1 + np.abs(c).max() / s.min())  # two float32 entries, each good to 2^-24 relative
        assert np.abs(first).max() <= tol and np.abs(last - [shape[1] - 1, shape[0] - 1]).max() <= tol


def test_tables_land_where_the_matrix_sends_the_point():
    """The integer tables hold the inverse map; here they are checked with the forward matrix alone.  The source point of output pixel
    (x, y), read from the tables in 1/32 pixel, must come back to (x, y) under the float32 matrix: within the gain times 1/64 pixel (the
    floor to 1/32 after the rounding offset of 1/64) + 2/1024 (the two rounded table entries that are added)."""
    for box, shape in [([0, 0, 50, 37], (32, 24)), ([3.3, 2.2, 40.7, 30.1], (40, 28)), ([-20, -10, 80, 60], (32, 24)),
                       ([3.2, 2.1, 4.9, 4.4], (64, 48)), ([-64, -64, 128, 128], (32, 24))]:
        H, W = shape
        c, s = M.center_scale(box, shape)
        m = M.udp_matrix(c, s, shape).astype(np.float64)
        adelta, bdelta, X0, Y0 = M.warp_tables(m.astype(np.float32), shape)
        X = ((X0[:, None] + adelta[None, :]) >> 5) / 32.0   # [H, W] source x in pixels
        Y = ((Y0[:, None] + bdelta[None, :]) >> 5) / 32.0
        back_x, back_y = m[0, 0] * X + m[0, 2], m[1, 1] * Y + m[1, 2]
        ys, xs = np.mgrid[0:H, 0:W]
        slack = 1 / 64 + 2 / 1024 + 1e-9
        assert np.abs(back_x - xs).max() <= m[0, 0] * slack + 1e-4 and np.abs(back_y - ys).max() <= m[1, 1] * slack + 1e-4


def test_warp_doubles_an_image_by_hand():
    """The box through the corner pixel centres onto 2 h - 1 by 2 w - 1 pixels: even outputs are the source pixels, odd ones the rounded
    mean of two neighbours, odd / odd ones of four.  The expected image is written out with slices."""
    rng = np.random.default_rng(5)
    h, w = 6, 5
    a = rng.integers(0, 256, (h, w, 3)).astype(np.int64)
    shape = (2 * h - 1, 2 * w - 1)
    mat = M.udp_matrix(np.array([(w - 1) / 2, (h - 1) / 2]), np.array([w - 1.0, h - 1.0]), shape)
    assert np.array_equal(mat, np.array([[2, 0, 0], [0, 2, 0]], dtype=np.float32))
    want = np.zeros(shape + (3,), dtype=np.int64)
    want[::2, ::2] = a
    want[::2, 1::2] = (a[:, :-1] + a[:, 1:] + 1) >> 1
    want[1::2, ::2] = (a[:-1] + a[1:] + 1) >> 1
    want[1::2, 1::2] = (a[:-1, :-1] + a[:-1, 1:] + a[1:, :-1] + a[1:, 1:] + 2) >> 2
    assert np.array_equal(M.warp(a.astype(np.uint8), None, M.warp_tables(mat, shape), shape), want)
    # and halved again: every second pixel of the doubled image is the source
    back = M.udp_matrix(np.array([w - 1.0, h - 1.0]), np.array([2 * w - 2.0, 2 * h - 2.0]), (h, w))
    assert np.array_equal(back, np.array([[0.5, 0, 0], [0, 0.5, 0]], dtype=np.float32))
    assert np.array_equal(M.warp(want.astype(np.uint8), None, M.warp_tables(back, (h, w)), (h, w)), a)


def test_host_tables_equal_the_model():
    from diffuman4d_amd.host import pose
    for box, shape in [([0, 0, 50, 37], (32, 24)), ([3.3, 2.2, 40.7, 30.1], (40, 28)), ([-20, -10, 80, 60], (32, 24)), ([3.2, 2.1, 4.9, 4.4], (1024, 768))]:
        c, s = pose.box_center_scale(box, shape)
        cm, sm = M.center_scale(box, shape)
        assert np.array_equal(c, cm) and np.array_equal(s, sm) and c.dtype == np.float64
        mat = pose.udp_warp_matrix(c, s, shape)
        assert mat.dtype == np.float32 and np.array_equal(mat, M.udp_matrix(cm, sm, shape))
        assert np.array_equal(pose.warp_tables(mat, shape), np.concatenate(M.warp_tables(mat, shape)))
    for bad in ([0, 0, 0, 5], [0, 5, 3, 5], [0, 0, float("nan"), 4], [-1e8, -1e8, 1e8, 1e8], [1e9, 1e9, 1e9 + 4096, 1e9 + 4096]):
        with pytest.raises(ValueError, match="bbox"):
            c, s = pose.box_center_scale(bad, (32, 24))
            pose.warp_tables(pose.udp_warp_matrix(c, s, (32, 24)), (32, 24))


def test_decode_recovers_a_noise_free_centre():
    """A sanity bound on the model, not a tolerance on the device."""
    for (Hh, Wh), (cx, cy) in [((64, 48), (20.37, 30.81)), ((23, 17), (8.45, 11.2)), ((64, 48), (10.5, 40.5))]:
        locs, scores = M.udp_decode(pose_cases.peak(Hh, Wh, cx, cy, noise=0)[None], np.float64)
        assert np.abs(locs[0] - [cx, cy]).max() < 0.05
        assert scores.dtype == np.float32


def test_decode_cases_are_well_conditioned_and_cover_the_paths():
    for Hh, Wh in [(8, 6), (23, 17), (64, 48), (14, 1024)]:
        names, maps = pose_cases.case_maps(Hh, Wh)
        locs, scores, conds = M.udp_decode(maps, np.float64, details=True)
        assert conds.max() < 100
        at = dict(zip(names, locs))
        assert at["tie"][0] < Wh / 2 and at["tie"][1] < Hh / 2  # the first of the two maxima
        for k in ("constant_high", "constant_low"):
            assert at[k].tolist() == [0, 0]
        for k in ("zero", "negative"):
            assert at[k].tolist() == [-1, -1]
        assert scores[names.index("negative")] < 0
    for Hh, Wh in [(64, 48), (12, 400), (14, 1024)]:
        rows = pose_cases.row_maps(Hh, Wh)
        assert all(np.argmax(rows[k]) // Wh == k for k in range(Hh))


# -- host side ---------------------------------------------------------------------------------------------------------------------------
def test_json_is_read_back_by_read_kp2d(tmp_path):
    from diffuman4d_amd.host import pose, triang
    rng = np.random.default_rng(1)
    kp, sc = rng.random((1, 133, 2)) * 1000, rng.random((1, 133)).astype(np.float32)
    path = str(tmp_path / "cam" / "000003.json")
    pose.write_instances(path, kp, sc)
    text = open(path).read()
    assert text.startswith('{\n\t"instance_info": [\n\t\t{\n\t\t\t"keypoints"')
    assert set(json.loads(text)["instance_info"][0]) == {"keypoints", "keypoint_scores"}
    got_kp, depth, got_sc = triang.read_kp2d(path)
    want = sc[0].astype(np.float64)
    want[92:112] *= want[91] ** 2
    want[113:133] *= want[112] ** 2
    assert np.array_equal(got_kp, kp[0]) and depth is None and np.array_equal(got_sc, want)


def _scene(tmp_path, n=3, masks=True):
    rng = np.random.default_rng(2)
    for k in range(n):
        for d, ext in (("images", ".jpg" if k else ".webp"),) + ((("fmasks", ".png"),) if masks else ()):
            path = tmp_path / d / f"{k % 2:02d}" / f"{k:06d}{ext}"
            path.parent.mkdir(parents=True, exist_ok=True)
            a = rng.integers(0, 256, (20, 16, 3), dtype=np.uint8)
            (Image.fromarray(a[..., 0]) if d == "fmasks" else Image.fromarray(a)).save(path)
    return str(tmp_path / "images"), str(tmp_path / "fmasks")


def test_paths_and_skip_exists(tmp_path):
    from diffuman4d_amd.host import lib as L, pose
    assert pose.output_path("out", "/d/images/03/000012.jpg") == os.path.join("out", "03", "000012.json")
    assert pose.output_path("out", "images/03/000012.webp") == os.path.join("out", "03", "000012.json")
    images_dir, fmasks_dir = _scene(tmp_path)
    images, fmasks = pose.list_inputs(images_dir, fmasks_dir)
    assert [os.path.basename(p) for p in images] == ["000000.webp", "000002.jpg", "000001.jpg"] and len(fmasks) == 3
    assert pose.list_inputs(images_dir, None)[1] is None and pose.list_inputs(images_dir, "None")[1] is None
    out = tmp_path / "kp"
    for p in images:
        pose.write_instances(pose.output_path(str(out), p), np.zeros((1, 2, 2)), np.zeros((1, 2)))

    def model(x):
        raise AssertionError("every file exists and parses: nothing to predict")
    assert pose.predict_keypoints(images_dir, str(out), fmasks_dir, pose_model=model) == {"images": 3, "written": 0, "skipped": 3}
    # a file that does not parse is not trusted: the stage goes on to the device (of which gpu_ids=[] names none)
    with open(pose.output_path(str(out), images[1]), "w") as f:
        f.write('{"instance_info": [')
    with pytest.raises(L.Dm4dError, match="no HIP device"):
        pose.predict_keypoints(images_dir, str(out), fmasks_dir, pose_model=model, gpu_ids=[])
    with pytest.raises(L.Dm4dError, match="no HIP device"):
        pose.predict_keypoints(images_dir, str(out), fmasks_dir, pose_model=model, gpu_ids=[], skip_exists=False)


def test_errors(tmp_path):
    from diffuman4d_amd.host import pose
    images_dir, fmasks_dir = _scene(tmp_path)
    os.remove(sorted((tmp_path / "fmasks" / "00").iterdir())[0])
    with pytest.raises(ValueError, match="fmask_paths and image_paths must have the same length"):
        pose.predict_keypoints(images_dir, str(tmp_path / "kp"), fmasks_dir, pose_model=lambda x: x)
    with pytest.raises(NotImplementedError, match="mmdet"):
        pose.predict_keypoints(images_dir, str(tmp_path / "kp"), None, pose_model=lambda x: x, detector_ckpt_path="rtmdet.pth")
    with pytest.raises(ValueError, match="name the pose network"):
        pose.predict_keypoints(images_dir, str(tmp_path / "kp"))
    with pytest.raises(ValueError, match="bbox_source"):
        pose.predict_keypoints(images_dir, str(tmp_path / "kp"), pose_model=lambda x: x, bbox_source="detector")
    with pytest.raises(ValueError, match="needs fmasks_dir"):
        pose.predict_keypoints(images_dir, str(tmp_path / "kp"), pose_model=lambda x: x, bbox_source="fmask")
    with pytest.raises(FileNotFoundError, match="never downloaded"):
        pose.load_pose_model(str(tmp_path / "sapiens_2b_torchscript.pt2"), "cpu")
    image = np.zeros((5, 4, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match="mode 'RGB'"):
        pose.pose_inputs([image], [np.zeros((5, 4, 3), dtype=np.uint8)], shape=(32, 24))
    with pytest.raises(ValueError, match="^images do not match$"):
        pose.pose_inputs([image], [np.zeros((4, 5), dtype=np.uint8)], shape=(32, 24))
    with pytest.raises(ValueError, match="same length"):
        pose.pose_inputs([image, image], [np.zeros((5, 4), dtype=np.uint8)], shape=(32, 24))
    with pytest.raises(ValueError, match="one entry per image"):
        pose.pose_inputs([image], None, [[0, 0, 1, 1], [0, 0, 2, 2]], shape=(32, 24))
    with pytest.raises(ValueError, match="needs a mask"):
        pose.pose_inputs([image], None, shape=(32, 24), bbox_source="fmask")
    try:  # the same text as Pillow's own
        Image.composite(Image.fromarray(image), Image.new("RGB", (4, 5)), Image.new("L", (5, 4)))
    except ValueError as e:
        assert str(e) == "images do not match"


# -- the C entry points ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from diffuman4d_amd.host import lib as L
    return L.load()


def last(lib):
    return lib.dm4d_last_error().decode()


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


H, W = 32, 24
PER_ROW = 2 * (H + W)
NORM = np.array(M.MEAN + M.STD, dtype=np.float32)


def pose_input(lib, desc, tab=None, staging_bytes=1 << 20, norm=NORM, out=P, H=H, W=W, rows=None, desc_dev=P, tab_dev=P):
    desc = np.ascontiguousarray(desc, dtype=np.int64)
    tab = np.zeros(PER_ROW * len(desc), dtype=np.int32) if tab is None else np.ascontiguousarray(tab, dtype=np.int32)
    return lib.dm4d_pose_input_u8_f32(None, P, staging_bytes, ptr(desc), desc_dev, len(desc) if rows is None else rows, ptr(tab), tab_dev, len(tab),
                                      ptr(norm), out, H, W)


def test_pose_input_rejects_bad_arguments(lib):
    good = [0, -1, 7, 9, 0, 0, 0, 0]

    def bad(**kw):
        d = list(good)
        for k, v in kw.items():
            d[int(k[1:])] = v
        return [d]
    assert lib.dm4d_pose_input_u8_f32(None, None, 1, None, P, 1, None, P, 1, None, P, H, W) == ERR_ARG and "null" in last(lib)
    assert pose_input(lib, [good], rows=0) == ERR_ARG and "rows" in last(lib)
    assert pose_input(lib, [good], H=0) == ERR_ARG and "1..4096" in last(lib)
    assert pose_input(lib, [good], W=4097) == ERR_ARG and "1..4096" in last(lib)
    assert pose_input(lib, [good], out=P + 2) == ERR_ARG and "aligned" in last(lib)
    assert pose_input(lib, [good], desc_dev=P + 4) == ERR_ARG and "aligned" in last(lib)
    assert pose_input(lib, [good], norm=np.array([0, 0, 0, 1, 0, 1], dtype=np.float32)) == ERR_ARG and "std" in last(lib)
    assert pose_input(lib, [good], norm=np.array([np.nan, 0, 0, 1, 1, 1], dtype=np.float32)) == ERR_ARG and "finite" in last(lib)
    assert pose_input(lib, bad(f2=0)) == ERR_ARG and "row 0: image size" in last(lib)
    assert pose_input(lib, bad(f3=16385)) == ERR_ARG and "image size" in last(lib)
    assert pose_input(lib, bad(f0=-1)) == ERR_ARG and "image outside" in last(lib)
    assert pose_input(lib, [good], staging_bytes=7 * 9 * 3 - 1) == ERR_ARG and "image outside" in last(lib)
    assert pose_input(lib, [good, bad(f0=(1 << 20) - 7 * 9 * 3 + 1)[0]]) == ERR_ARG and "row 1: image outside" in last(lib)
    assert pose_input(lib, bad(f1=-2)) == ERR_ARG and "mask offset" in last(lib)
    assert pose_input(lib, bad(f1=(1 << 20) - 62)) == ERR_ARG and "mask outside" in last(lib)
    assert pose_input(lib, bad(f6=1)) == ERR_ARG and "spare" in last(lib)
    assert pose_input(lib, bad(f4=1)) == ERR_ARG and "outside tab" in last(lib)
    assert pose_input(lib, bad(f4=-1)) == ERR_ARG and "outside tab" in last(lib)
    tab = np.zeros(PER_ROW, dtype=np.int32)
    tab[PER_ROW - 1] = (1 << 29) + 1
    assert pose_input(lib, [good], tab=tab) == ERR_ARG and "2^29" in last(lib)
    tab[PER_ROW - 1], tab[0] = 0, -(1 << 29) - 1
    assert pose_input(lib, [good], tab=tab) == ERR_ARG and "2^29" in last(lib)


def test_pose_mask_box_rejects_bad_arguments(lib):
    def box(desc, staging_bytes=1 << 20, n=None, boxes=P):
        desc = np.ascontiguousarray(desc, dtype=np.int64)
        return lib.dm4d_pose_mask_box_u8(None, P, staging_bytes, ptr(desc), P, len(desc) if n is None else n, boxes)
    good = [-1, 0, 7, 9, 0, 0, 0, 0]
    assert lib.dm4d_pose_mask_box_u8(None, P, 1, None, P, 1, P) == ERR_ARG and "null" in last(lib)
    assert box([good], n=0) == ERR_ARG and "1..65535" in last(lib)
    assert box([good], boxes=P + 1) == ERR_ARG and "aligned" in last(lib)
    assert box([[0, -1, 7, 9, 0, 0, 0, 0]]) == ERR_ARG and "mask offset" in last(lib)
    assert box([good], staging_bytes=62) == ERR_ARG and "mask outside" in last(lib)
    assert box([[-1, 0, 7, 0, 0, 0, 0, 0]]) == ERR_ARG and "image size" in last(lib)
    assert box([[-1, 0, 7, 9, 0, 0, 0, 3]]) == ERR_ARG and "spare" in last(lib)


def test_pose_udp_decode_rejects_bad_arguments(lib):
    def dec(n=1, K=17, Hh=64, Wh=48, heat=P, scores=P, locs=P):
        return lib.dm4d_pose_udp_decode_f32(None, heat, n, K, Hh, Wh, scores, locs)
    assert dec(heat=None) == ERR_ARG and "null" in last(lib)
    assert dec(locs=None) == ERR_ARG and "null" in last(lib)
    assert dec(n=0) == ERR_ARG and "n * K" in last(lib)
    assert dec(K=0) == ERR_ARG and "n * K" in last(lib)
    assert dec(n=1 << 13, K=1 << 12) == ERR_ARG and "n * K" in last(lib)
    for Hh, Wh in [(1, 48), (64, 1), (4097, 48), (64, 1025)]:
        assert dec(Hh=Hh, Wh=Wh) == ERR_ARG and "heatmap size" in last(lib)
    assert dec(scores=P + 2) == ERR_ARG and "aligned" in last(lib)


def test_abi_tables_hold_the_new_surface():
    from test_abi import _constant, header_constants, header_functions
    from diffuman4d_amd.host import lib as L
    fns = header_functions()
    for name, n_args in (("dm4d_pose_input_u8_f32", 13), ("dm4d_pose_mask_box_u8", 7), ("dm4d_pose_udp_decode_f32", 8)):
        assert fns[name] == n_args and len(L.SIGNATURES[name][1]) == n_args
    consts = header_constants()
    for name, value in (("POSE_FIELDS", 8), ("POSE_MAX_SIDE", 16384), ("POSE_MAX_HEATMAP_H", 4096), ("POSE_MAX_HEATMAP_W", 1024)):
        assert int(consts[name]) == value == getattr(L, name)
    assert _constant(consts["POSE_TAB_LIMIT"]) == 1 << 29 == L.POSE_TAB_LIMIT
