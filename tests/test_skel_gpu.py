"""GPU: skeleton maps (dm4d_skeleton_draw_u8 through diffuman4d_amd/host/skeleton.py) against the numpy model of the rasteriser reduced
by Pillow itself (tests/skel_model.py), byte for byte, on the draw calls the reference recorded (tests/golden/skel_reference.json); and
draw_skeleton end to end on a copy of the ring8 scene, whose files must hold the bytes of Pillow's own encoding of the expected maps."""
import functools
import io
import json
import os
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
from PIL import Image

import skel_model
from diffuman4d_amd.host import skeleton, triang

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
RING8 = GOLDEN / "triang_scene" / "ring8"
PALETTE_PATH = GOLDEN / "skel_palette.json"
CASES = {c["name"]: c for c in json.loads((GOLDEN / "skel_reference.json").read_text())["cases"]}
PALETTE = skeleton.load_palette(PALETTE_PATH)
SQUARE = ("scores_only", "depths_with_a_tie", "ones_no_depths", "hands_in_one_tile", "off_canvas_inside_range")  # all 1024 x 1024


@functools.lru_cache(maxsize=None)
def plan(name):
    c = CASES[name]
    return skeleton.plan_draw_calls(c["instance"], c["score_instance"], (c["kp2d_canvas_shape"], c["out_kpmap_shape"]), PALETTE)


def expect(p):
    return skel_model.expected_map(p.calls, p.canvas_shape, p.out_size)


@functools.lru_cache(maxsize=None)
def expected(name):
    m = expect(plan(name))
    m.setflags(write=False)
    return m


def differing(a, b):
    return f"{int((a != b).any(axis=-1).sum())} of {a.shape[0] * a.shape[1]} pixels differ, max |d| {int(np.abs(a.astype(int) - b.astype(int)).max())}"


@pytest.mark.parametrize("name", list(CASES))
def test_map_equals_the_model_reduced_by_pillow(hip_device, name):
    """Every sort branch, the thresholds, rounding ties, the output shapes (tiles of 32 and of 16 outputs, ragged last tiles, a map
    as large as the canvas, an enlargement), 40 and more links in one tile with two of length zero, and primitives that leave the canvas."""
    p = plan(name)
    got = skeleton.draw_plans([p])
    want = expected(name)
    assert got.dtype == np.uint8 and got.shape == (1, p.out_size[1], p.out_size[0], 3) and want.any()
    assert np.array_equal(got[0], want), differing(got[0], want)


def test_two_runs_give_the_same_bytes(hip_device):
    for name in ("hands_in_one_tile", "shape_1000x600", "shape_512x512"):
        assert np.array_equal(skeleton.draw_plans([plan(name)]), skeleton.draw_plans([plan(name)])), name


def test_a_frame_alone_equals_the_frame_in_a_batch_of_five(hip_device):
    batch = skeleton.draw_plans([plan(n) for n in SQUARE])
    assert batch.shape == (5, 1024, 1024, 3)
    for k, name in enumerate(SQUARE):
        assert np.array_equal(batch[k], skeleton.draw_plans([plan(name)])[0]), name
        assert np.array_equal(batch[k], expected(name)), name


def test_a_batch_cut_into_several_launches(hip_device, monkeypatch):
    """The frame axis is cut where a launch's maps would pass LAUNCH_BYTES: with room for two maps, five frames take three launches."""
    monkeypatch.setattr(skeleton, "LAUNCH_BYTES", 2 * 1024 * 1024 * 3)
    got = skeleton.draw_plans([plan(n) for n in SQUARE])
    assert got.shape == (5, 1024, 1024, 3)
    for k, name in enumerate(SQUARE):
        assert np.array_equal(got[k], expected(name)), name


def test_a_batch_with_different_counts_and_an_empty_frame(hip_device):
    inst = dict(CASES["scores_only"]["instance"], keypoint_scores=[0.2] * 133)  # no link reaches low_thr
    empty = skeleton.plan_draw_calls(inst, None, ((1024, 1024), (1024, 1024)), PALETTE)
    assert empty.calls == []
    plans = [plan("score_override"), empty, plan("ones_no_depths")]
    assert [len(p.calls) for p in plans] == [114, 0, 201]
    got = skeleton.draw_plans(plans)
    assert np.array_equal(got[0], expected("score_override")) and not got[1].any() and np.array_equal(got[2], expected("ones_no_depths"))
    alone = skeleton.draw_plans([empty])
    assert alone.shape == (1, 1024, 1024, 3) and not alone.any()


def test_the_smallest_supported_output(hip_device):
    """max(out_kpmap_shape) = 256: a canvas eight times the map, the only ratio at which the library takes tiles of 8 outputs."""
    c = CASES["scores_only"]
    for shape in ((256, 256), (200, 256)):
        p = skeleton.plan_draw_calls(c["instance"], None, ((1024, 1024), shape), PALETTE)
        assert p.canvas_shape == (2048 * shape[0] // 256, 2048) and p.out_size == (256, shape[0])
        got, want = skeleton.draw_plans([p])[0], expect(p)
        assert want.any() and np.array_equal(got, want), differing(got, want)


# -- the file route ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(hip_device, tmp_path_factory):
    """A copy of ring8 with poses_2d written by the native triangulate_skeleton for the cameras 0 and 4 -> (root, expected bytes by
    relative path of the .webp files)."""
    root = tmp_path_factory.mktemp("skel_scene")
    shutil.copytree(RING8, root / "ring8")
    d = root / "ring8"
    triang.triangulate_skeleton(str(d / "transforms.json"), str(d / "poses_sapiens"), str(d / "poses_3d"), out_kp2d_proj_dir=str(d / "poses_2d"),
                                spa_labels_proj=[0, 4])
    want = {}
    for cam in ("00", "04"):
        for frame in ("000000", "000001"):
            inst = json.loads((d / "poses_2d" / cam / f"{frame}.json").read_text())["instance_info"][0]
            p = skeleton.plan_draw_calls(inst, None, ((1024, 1024), (1024, 1024)), PALETTE)
            assert len(p.calls) > 60  # depths present, invalid keypoints at -1e6 are left out by their zeroed score
            buf = io.BytesIO()
            Image.fromarray(expect(p)).save(buf, format="WEBP", quality=85)
            want[f"{cam}/{frame}.webp"] = buf.getvalue()
    return d, want


def files(root: Path):
    return {str(p.relative_to(root)): p.read_bytes() for p in sorted(root.rglob("*")) if p.is_file()}


def test_draw_skeleton_writes_pillow_s_encoding_of_the_expected_maps(scene, tmp_path):
    d, want = scene
    out = tmp_path / "skeletons"
    res = skeleton.draw_skeleton(str(d / "poses_2d"), str(out), spa_labels=[0, 4], palette=str(PALETTE_PATH))
    assert res["frames"] == 4 and res["skipped"] == 0 and res["files"] == 4 and res["dropped_links"] == 0
    got = files(out)
    assert sorted(got) == sorted(want)
    for path in want:
        assert got[path] == want[path], path
    # labels default to the listings; the same bytes again
    out2 = tmp_path / "listing"
    skeleton.draw_skeleton(str(d / "poses_2d"), str(out2), palette=PALETTE, num_workers=2)
    assert files(out2) == want
    # skip_exists: a valid file keeps its bytes and its time stamp, a truncated one is written again
    marker = io.BytesIO()
    Image.new("RGB", (8, 8), (1, 2, 3)).save(marker, format="WEBP", quality=85)
    (out / "00" / "000000.webp").write_bytes(marker.getvalue())
    os.utime(out / "00" / "000000.webp", ns=(10**18, 10**18))
    (out / "04" / "000001.webp").write_bytes(want["04/000001.webp"][:100])
    (out / "04" / "000000.webp").unlink()
    res = skeleton.draw_skeleton(str(d / "poses_2d"), str(out), spa_labels=[0, 4], palette=PALETTE, skip_exists=True)
    assert res["frames"] == 2 and res["skipped"] == 2 and res["files"] == 2
    got = files(out)
    assert got["00/000000.webp"] == marker.getvalue() and (out / "00" / "000000.webp").stat().st_mtime_ns == 10**18
    assert all(got[p] == want[p] for p in ("00/000001.webp", "04/000000.webp", "04/000001.webp"))
    # without a palette there is nothing to draw with
    with pytest.raises(ValueError, match="no palette given"):
        skeleton.draw_skeleton(str(d / "poses_2d"), str(tmp_path / "none"))


def test_score_override_directory_and_other_shapes(scene, tmp_path):
    """kp2d_score_dir replaces the scores file by file; out_kpmap_shape (1000, 600) gives 599 x 1000 files."""
    d, _ = scene
    scores = tmp_path / "scores"
    rng = np.random.default_rng(5)
    for cam in ("00",):
        for frame in ("000000", "000001"):
            (scores / cam).mkdir(parents=True, exist_ok=True)
            (scores / cam / f"{frame}.json").write_text(json.dumps({"instance_info": [{"keypoint_scores": rng.uniform(0.3, 1.0, 133).tolist()}]}))
    out = tmp_path / "out"
    res = skeleton.draw_skeleton(str(d / "poses_2d"), str(out), kp2d_score_dir=str(scores), out_kpmap_shape=(1000, 600), spa_labels=[0],
                                 tem_labels=[0, 1], image_ext=".png", palette=PALETTE)
    assert res["files"] == 2
    for frame in ("000000", "000001"):
        inst = json.loads((d / "poses_2d" / "00" / f"{frame}.json").read_text())["instance_info"][0]
        sc = json.loads((scores / "00" / f"{frame}.json").read_text())["instance_info"][0]
        p = skeleton.plan_draw_calls(inst, sc, ((1024, 1024), (1000, 600)), PALETTE)
        with Image.open(out / "00" / f"{frame}.png") as im:
            assert im.size == (599, 1000)
            assert np.array_equal(np.asarray(im.convert("RGB")), expect(p))


def test_cli_help_and_the_same_files(scene, tmp_path):
    d, want = scene
    tool = str(ROOT / "tools" / "draw_skeleton.py")
    r = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--palette" in r.stdout and "--kp2d_dir" in r.stdout
    out = tmp_path / "cli"
    r = subprocess.run([sys.executable, tool, "--kp2d_dir", str(d / "poses_2d"), "--out_kpmap_dir", str(out), "--spa_labels", "0,4",
                        "--palette", str(PALETTE_PATH)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert files(out) == want
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["frames"] == 4 and res["files"] == 4
