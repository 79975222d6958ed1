"""CPU: the host half of visual-hull carving (diffuman4d_amd/host/vhull.py) and the numpy model of its kernels
(tests/vhull_model.py) against the reference's recorded results (tests/golden/vhull_reference.pt, made by
tests/golden/make_golden_vhull.py from the reference's own carve_visual_hull and main on tests/golden/vhull_scene/body6)."""
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image

import vhull_model
from vhull_model import read_ply
from diffuman4d_amd.host import lib as L
from diffuman4d_amd.host import vhull

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
SCENE = GOLDEN / "vhull_scene" / "body6"
REF = torch.load(GOLDEN / "vhull_reference.pt", weights_only=False)
ENTRIES = ("dm4d_vhull_pack_masks", "dm4d_vhull_ws_bytes", "dm4d_vhull_carve_chunk")


def frame_masks(frame: int, labels=None) -> torch.Tensor:
    return torch.stack([vhull.load_binary_mask(str(SCENE / "fmasks" / lab / f"{frame:06d}.png")) for lab in (labels or REF["labels"])])


@pytest.mark.parametrize("case", REF["cases"], ids=[c["name"] for c in REF["cases"]])
def test_model_reproduces_the_reference(case):
    got = vhull_model.carve(frame_masks(case["frame"]).numpy(), REF["P"].numpy(), case["bounds"], case["voxel_size"], case["min_views"])
    want = case["points"].numpy()
    assert got.dtype == np.float32 and want.dtype == np.float32
    assert np.array_equal(got, want)  # values, count and order
    assert tuple(len(a) for a in vhull_model.grid_axes(case["bounds"], case["voxel_size"])) == tuple(case["grid"])


def test_fixture_covers_what_it_is_for():
    by = {c["name"]: c for c in REF["cases"]}
    for c in REF["cases"]:
        assert c["tie_margin"] >= 1e-9 and c["z_margin"] >= 1e-9, c["name"]
    assert len(by["empty"]["points"]) == 0
    assert tuple(by["dense10"]["grid"]) == (10, 10, 10) and len(by["dense10"]["points"]) == 1000  # every voxel kept
    assert by["arange4"]["grid"] == (4, 4, 4)  # torch.arange's count, not round((max - min) / voxel_size) = 3
    assert by["cube67_all"]["grid"][2] % 64 != 0 and int(np.prod(by["cube67_all"]["grid"])) % 256 != 0
    assert 0 < len(by["slab_min6"]["points"]) < len(by["slab_min1"]["points"])
    assert len(by["cube40_all"]["points"]) < len(by["cube40_min4"]["points"])


def test_main_route_of_the_fixture_is_the_model_too():
    m = REF["main"]
    for t, (label, pts) in enumerate(sorted(m["frames"].items())):
        got = vhull_model.carve(frame_masks(t).numpy(), REF["P"].numpy(), m["kw"]["bounds"], m["kw"]["voxel_size"], m["kw"]["min_views"])
        assert np.array_equal(got, pts.numpy()), label
    allp = np.concatenate([p.numpy() for p in m["frames"].values()])
    assert m["bounds_json"] == [allp.min(axis=0).astype(np.float64).tolist(), allp.max(axis=0).astype(np.float64).tolist()]


# -- load_binary_mask -------------------------------------------------------------------------------------------------------------
def test_load_binary_mask_thresholds_and_modes(tmp_path):
    a = np.array([[0, 127, 128, 255], [126, 129, 1, 254]], dtype=np.uint8)
    Image.fromarray(a).save(tmp_path / "l.png")
    m = vhull.load_binary_mask(str(tmp_path / "l.png"))
    assert m.dtype == torch.bool and tuple(m.shape) == (2, 4)
    assert m.tolist() == [[False, False, True, True], [False, True, False, True]]
    # the same decision as to_tensor(m) > 0.5 in float32
    assert torch.equal(m, torch.from_numpy(a).to(torch.float32).div(255) > 0.5)
    Image.fromarray(np.where(a >= 128, 255, 0).astype(np.uint8)).convert("1", dither=Image.Dither.NONE).save(tmp_path / "one.png")
    with Image.open(tmp_path / "one.png") as im:
        assert im.mode == "1"
    assert torch.equal(vhull.load_binary_mask(str(tmp_path / "one.png")), m)
    Image.fromarray(np.stack([a, a, a], axis=-1)).save(tmp_path / "rgb.png")
    with pytest.raises(ValueError, match="RGB"):
        vhull.load_binary_mask(str(tmp_path / "rgb.png"))


def test_scene_has_a_mode_1_camera_and_soft_pixels():
    modes = set()
    for lab in REF["labels"]:
        with Image.open(SCENE / "fmasks" / lab / "000000.png") as im:
            modes.add(im.mode)
            if im.mode == "L":
                vals = set(np.unique(np.asarray(im)).tolist())
                assert {127, 128} <= vals
    assert modes == {"L", "1"}


# -- save_pcd_ply -----------------------------------------------------------------------------------------------------------------
def test_save_pcd_ply_header_round_trip_and_empty(tmp_path):
    rng = np.random.default_rng(0)
    pts = rng.standard_normal((37, 3)).astype(np.float32)
    colors = rng.integers(0, 256, (37, 3), dtype=np.uint8)
    path = tmp_path / "a" / "b" / "cloud.ply"  # parent directories are created
    vhull.save_pcd_ply(str(path), pts, colors)
    header, p, c = read_ply(path)
    assert header == ("ply\nformat binary_little_endian 1.0\nelement vertex 37\nproperty float x\nproperty float y\nproperty float z\n"
                      "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    assert np.array_equal(p, pts) and np.array_equal(c, colors)
    assert path.stat().st_size == len(header) + 37 * 15
    vhull.save_pcd_ply(str(tmp_path / "white.ply"), torch.from_numpy(pts))
    _, p, c = read_ply(tmp_path / "white.ply")
    assert np.array_equal(p, pts) and (c == 255).all()
    vhull.save_pcd_ply(str(tmp_path / "empty.ply"), np.zeros((0, 3), np.float32))
    header, p, _ = read_ply(tmp_path / "empty.ply")
    assert "element vertex 0\n" in header and p.shape == (0, 3)


# -- cameras ----------------------------------------------------------------------------------------------------------------------
def test_projections_equal_the_reference_bit_for_bit():
    P = vhull.read_projections(str(SCENE / "transforms.json"), REF["labels"])
    assert P.dtype == torch.float64 and torch.equal(P, REF["P"])


def test_cameras_are_matched_by_label(tmp_path):
    every = vhull.read_projections(str(SCENE / "transforms.json"), REF["labels"])
    some = vhull.read_projections(str(SCENE / "transforms.json"), REF["labels"][::2])
    assert torch.equal(some, every[::2])
    tf = json.loads((SCENE / "transforms.json").read_text())
    tf["frames"] = tf["frames"][::-1]  # file order is not the sorted order
    (tmp_path / "reversed.json").write_text(json.dumps(tf))
    assert torch.equal(vhull.read_projections(str(tmp_path / "reversed.json"), REF["labels"]), every)
    with pytest.raises(ValueError, match="camera_label"):
        vhull.read_projections(str(SCENE / "transforms.json"), ["00", "77"])


def test_cameras_without_labels_go_by_position_and_a_mismatch_raises(tmp_path):
    tf = json.loads((SCENE / "transforms.json").read_text())
    for fr in tf["frames"]:
        del fr["camera_label"]
    (tmp_path / "plain.json").write_text(json.dumps(tf))
    assert torch.equal(vhull.read_projections(str(tmp_path / "plain.json"), REF["labels"]), REF["P"])
    with pytest.raises(ValueError, match="position"):
        vhull.read_projections(str(tmp_path / "plain.json"), REF["labels"][:3])


def test_easyvolcap_cameras_are_refused(tmp_path):
    with pytest.raises(NotImplementedError, match="EasyVolcap"):
        vhull.read_projections(str(tmp_path / "cameras"), ["00"])
    with pytest.raises(NotImplementedError, match="EasyVolcap"):
        vhull.carve_scene(str(SCENE / "fmasks"), str(tmp_path / "intri.yml"), str(tmp_path / "surfs"))


# -- arguments and ABI ------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    fm, P, b = torch.zeros(2, 4, 4, dtype=torch.bool), torch.zeros(2, 3, 4, dtype=torch.float64), (-1, 1, -1, 1, -1, 1)
    with pytest.raises(ValueError, match="fmasks / Ps"):
        vhull.carve_visual_hull(fm, P[:1], b)
    with pytest.raises(ValueError, match="min_views"):
        vhull.carve_visual_hull(fm, P, b, min_views=0)
    with pytest.raises(ValueError, match="voxel_size"):
        vhull.carve_visual_hull(fm, P, b, voxel_size=0.0)
    with pytest.raises(ValueError, match="voxel_size"):
        vhull.carve_visual_hull(fm, P, b, voxel_size=-0.1)
    with pytest.raises(ValueError, match="bounds.*y axis"):
        vhull.carve_visual_hull(fm, P, (-1, 1, 1, 1, -1, 1))
    with pytest.raises(ValueError, match="Ps"):
        vhull.carve_visual_hull(fm, P.to(torch.float16), b)
    with pytest.raises(ValueError, match="fmasks"):
        vhull.carve_visual_hull(fm.to(torch.uint8), P, b)


def test_there_is_no_cpu_path():
    fm, P = torch.ones(2, 4, 4, dtype=torch.bool), torch.zeros(2, 3, 4, dtype=torch.float64)
    with pytest.raises(L.Dm4dError, match="HIP device"):
        vhull.carve_visual_hull(fm, P, (-1, 1, -1, 1, -1, 1), voxel_size=0.5, device="cpu")
    from diffuman4d_amd.host import ops
    with pytest.raises(L.Dm4dError, match="HIP device"):
        ops.vhull_pack_masks(fm)


def test_batch_size_becomes_whole_blocks():
    assert vhull._chunk_voxels(1) == 256 and vhull._chunk_voxels(256) == 256 and vhull._chunk_voxels(7777) == 7680
    assert vhull._chunk_voxels(1e6) == 999936 and vhull._chunk_voxels(1e12) == 1 << 26


def test_abi_entries_are_in_header_library_and_table():
    header = (ROOT / "include" / "dm4d.h").read_text()
    lib = L.load()
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert lib.dm4d_vhull_ws_bytes(0) == 0 and lib.dm4d_vhull_ws_bytes((1 << 26) + 1) == 0
    assert lib.dm4d_vhull_ws_bytes(256) == 16 + 36 and lib.dm4d_vhull_ws_bytes(257) == 16 + 72
    from diffuman4d_amd import build
    assert "vhull.hip" in build.SOURCES and "-ffp-contract=off" in build.EXTRA_FLAGS["vhull.hip"]
