"""GPU: visual-hull carving (dm4d_vhull_pack_masks + dm4d_vhull_carve_chunk through diffuman4d_amd/host/vhull.py) against the
reference's recorded points (tests/golden/vhull_reference.pt) and, for scenes the fixture does not hold, against the numpy model
(tests/vhull_model.py).  Equality is exact everywhere: values, count and order."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import vhull_model
from diffuman4d_amd.host import ops, vhull
from vhull_model import read_ply

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
SCENE = ROOT / "tests" / "golden" / "vhull_scene" / "body6"
REF = torch.load(ROOT / "tests" / "golden" / "vhull_reference.pt", weights_only=False)
CASES = {c["name"]: c for c in REF["cases"]}


def frame_masks(frame: int, labels=None) -> torch.Tensor:
    return torch.stack([vhull.load_binary_mask(str(SCENE / "fmasks" / lab / f"{frame:06d}.png")) for lab in (labels or REF["labels"])])


def native(case, **over):
    kw = {k: case[k] for k in ("voxel_size", "batch_size", "min_views")}
    kw.update(over)
    return vhull.carve_visual_hull(frame_masks(case["frame"]), REF["P"], case["bounds"], device="cuda", **kw)


@pytest.mark.parametrize("name", list(CASES))
def test_fixture_case_is_reproduced_exactly(hip_device, name):
    got = native(CASES[name])
    assert got.is_cuda and got.dtype == torch.float32 and got.dim() == 2 and got.shape[1] == 3
    assert torch.equal(got.cpu(), CASES[name]["points"])


def test_result_does_not_depend_on_batch_size_and_runs_repeat(hip_device):
    case = CASES["cube67_all"]
    runs = [native(case, batch_size=b).cpu() for b in (1e6, 7777, 256, 1e6)]
    for r in runs:
        assert torch.equal(r, case["points"])


def test_float32_projections_are_widened(hip_device):
    case = CASES["cube40_all"]
    P32 = REF["P"].to(torch.float32)
    got = vhull.carve_visual_hull(frame_masks(0), P32, case["bounds"], voxel_size=case["voxel_size"], device="cuda").cpu()
    want = vhull_model.carve(frame_masks(0).numpy(), P32.to(torch.float64).numpy(), case["bounds"], case["voxel_size"])
    assert np.array_equal(got.numpy(), want)


def test_a_hull_larger_than_the_first_buffer_is_carved_again(hip_device):
    """_carve sizes its output before the count is known; with room for 100 points the 4231-point hull takes the second pass."""
    case = CASES["cube67_all"]
    dev = torch.device("cuda", torch.cuda.current_device())
    bits = ops.vhull_pack_masks(frame_masks(0).to(dev))
    axes = tuple(a.to(dev) for a in vhull.build_voxel_grid_linspaces(case["bounds"], case["voxel_size"]))
    for cap in (100, len(case["points"]), len(case["points"]) + 1):
        got = vhull._carve(bits, (96, 80), REF["P"].to(dev), axes, 5000, None, capacity=cap)
        assert torch.equal(got.cpu(), case["points"]), cap


def seeded_scene(seed, B, H, W):
    """Random blobby masks and cameras on a ring: compared with the model, which needs no tie margin (same operations, same order)."""
    rng = np.random.default_rng(seed)
    masks = np.zeros((B, H, W), bool)
    yy, xx = np.mgrid[:H, :W]
    P = np.zeros((B, 3, 4))
    for b in range(B):
        for _ in range(6):
            cx, cy, r = rng.uniform(0.2 * W, 0.8 * W), rng.uniform(0.2 * H, 0.8 * H), rng.uniform(0.15, 0.4) * min(H, W)
            masks[b] |= (xx - cx) ** 2 + (yy - cy) ** 2 < r * r
        masks[b] ^= rng.random((H, W)) < 0.05
        masks[b, :, W - 1] = True  # the last column: the tail of a row's last word
        a = rng.uniform(0, 2 * np.pi)
        o = np.array([2.5 * np.cos(a), rng.uniform(-0.3, 0.3), 2.5 * np.sin(a)])
        fwd = -o / np.linalg.norm(o)
        right = np.cross(fwd, [0.0, 1.0, 0.0])
        right /= np.linalg.norm(right)
        R = np.stack([right, np.cross(fwd, right), fwd])
        f = rng.uniform(0.9, 1.3) * W
        K = np.array([[f, 0, W / 2 + rng.uniform(-2, 2)], [0, f, H / 2 + rng.uniform(-2, 2)], [0, 0, 1]])
        P[b] = K @ np.concatenate([R, (-R @ o)[:, None]], axis=1)
    return torch.from_numpy(masks), torch.from_numpy(P)


@pytest.mark.parametrize("seed,B,H,W,min_views", [(1, 5, 64, 75, None), (2, 4, 51, 96, 2), (3, 1, 33, 31, None), (4, 3, 40, 65, 4)])
def test_seeded_scenes_against_the_model(hip_device, seed, B, H, W, min_views):
    """Widths that are no multiple of 32, an odd height, B = 1, and min_views > B (which keeps nothing)."""
    masks, P = seeded_scene(seed, B, H, W)
    bounds = (-1.5, 1.5, -0.9, 0.9, -1.5, 1.5)  # wider than the views: voxels leave the image on every side
    got = vhull.carve_visual_hull(masks, P, bounds, voxel_size=0.06, batch_size=5000, min_views=min_views, device="cuda").cpu().numpy()
    want = vhull_model.carve(masks.numpy(), P.numpy(), bounds, 0.06, min_views)
    assert np.array_equal(got, want)
    assert (len(want) == 0) == (min_views is not None and min_views > B)
    assert got.shape == (len(want), 3)


def test_pack_masks_bits(hip_device):
    masks, _ = seeded_scene(9, 3, 7, 75)
    bits = ops.vhull_pack_masks(masks.cuda()).cpu().numpy().view(np.uint32)
    assert bits.shape == (3, 7, 3)
    x = np.arange(96)
    unpacked = ((bits[:, :, x >> 5] >> (x & 31).astype(np.uint32)) & 1).astype(bool)
    assert np.array_equal(unpacked[:, :, :75], masks.numpy()) and not unpacked[:, :, 75:].any()


def check_outputs(out: Path, sparse: Path):
    m = REF["main"]
    for label, pts in m["frames"].items():
        _, p, c = read_ply(out / f"{label}.ply")
        assert np.array_equal(p, pts.numpy()) and (c == 255).all(), label
    assert json.loads(Path(str(out) + "_bounds.json").read_text()) == m["bounds_json"]
    _, p, _ = read_ply(sparse)
    assert np.array_equal(p, m["frames"][sorted(m["frames"])[0]].numpy())


def test_carve_scene_equals_the_reference_main(hip_device, tmp_path):
    m = REF["main"]
    out, sparse = tmp_path / "surfs", tmp_path / "export" / "sparse_pcd.ply"
    res = vhull.carve_scene(str(SCENE / "fmasks"), str(SCENE / "transforms.json"), str(out), sparse_pcd_path=str(sparse), **m["kw"])
    check_outputs(out, sparse)
    assert res["frames"] == {k: len(v) for k, v in m["frames"].items()} and res["bounds"] == m["bounds_json"]
    # every second camera: the views are matched to transforms.json by camera_label
    res = vhull.carve_scene(str(SCENE / "fmasks"), str(SCENE / "transforms.json"), str(tmp_path / "half"), camera_range=(0, None, 2),
                            frame_range=(1, None, 1), **m["kw"])
    labels = REF["labels"][::2]
    want = vhull_model.carve(frame_masks(1, labels).numpy(), REF["P"][::2].numpy(), m["kw"]["bounds"], m["kw"]["voxel_size"])
    _, p, _ = read_ply(tmp_path / "half" / "000001.ply")
    assert np.array_equal(p, want) and list(res["frames"]) == ["000001"] and len(want) > len(m["frames"]["000001"])


def test_an_empty_hull_is_an_error_of_carve_scene(hip_device, tmp_path):
    with pytest.raises(ValueError, match="enlarge bounds or lower min_views"):
        vhull.carve_scene(str(SCENE / "fmasks"), str(SCENE / "transforms.json"), str(tmp_path / "surfs"), bounds=CASES["empty"]["bounds"],
                          voxel_size=0.05)


def test_cli_writes_the_same_files(hip_device, tmp_path):
    m = REF["main"]
    out, sparse = tmp_path / "surfs", tmp_path / "sparse_pcd.ply"
    cmd = [sys.executable, str(ROOT / "tools" / "carve_visual_hull.py"), "--fmasks_dir", str(SCENE / "fmasks"), "--cameras_path",
           str(SCENE / "transforms.json"), "--out_vhull_dir", str(out), "--bounds=" + ",".join(str(v) for v in m["kw"]["bounds"]),
           "--voxel_size", str(m["kw"]["voxel_size"]), "--batch_size", str(m["kw"]["batch_size"]), "--camera_range", "0,None,1",
           "--sparse_pcd", str(sparse)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    check_outputs(out, sparse)
    assert json.loads(r.stdout.strip().splitlines()[-1])["bounds"] == m["bounds_json"]
