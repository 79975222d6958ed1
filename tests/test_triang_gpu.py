"""GPU: skeleton triangulation (dm4d_triangulate_points_f64 + dm4d_project_points_f64 through diffuman4d_amd/host/triang.py) against
the reference's recorded results (tests/golden/triang_reference.pt).

The bound on a triangulated point is not invented: it is the reference's own measured distance from the minimiser of its cost, read
from the fixture, |native - converged| <= d_ref + d_conv per case (the Euclidean distance in metres for the point, pixels for reproj), with n_views and the
INVALID pattern exactly the reference's.  Repeatability and batch invariance are asked bit for bit."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from diffuman4d_amd.host import triang

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
SCENES = ROOT / "tests" / "golden" / "triang_scene"
REF = torch.load(ROOT / "tests" / "golden" / "triang_reference.pt", weights_only=False)
CASES = {c["name"]: c for c in REF["cases"]}


def native(c):
    return triang.triangulate_points(c["Ks"], c["Ts"], c["kp2d"], c["score"])


def check_points(name, kp3d, reproj, n_views, want):
    """`want`: a fixture entry with n_views, kp3d_converged, reproj_converged and the four distances."""
    assert np.array_equal(n_views, want["n_views"]), name
    invalid = want["n_views"] < 3
    assert np.array_equal((kp3d == -1e6).all(axis=-1), invalid) and np.array_equal((kp3d == -1e6).any(axis=-1), invalid), name
    assert np.array_equal(reproj == -1e6, invalid), name
    e_m = np.linalg.norm(kp3d[~invalid] - want["kp3d_converged"][~invalid], axis=-1).max()
    e_px = np.abs(reproj[~invalid] - want["reproj_converged"][~invalid]).max()
    print(f"{name}: point {e_m:.3e} m (bound {want['d_ref_m'] + want['d_conv_m']:.3e}), reproj {e_px:.3e} px "
          f"(bound {want['d_ref_px'] + want['d_conv_px']:.3e})")
    assert e_m <= want["d_ref_m"] + want["d_conv_m"], name
    assert e_px <= want["d_ref_px"] + want["d_conv_px"], name


@pytest.mark.parametrize("name", list(CASES))
def test_case_is_within_the_reference_s_own_distance_from_the_minimiser(hip_device, name):
    """Covers n = 3 (exactly min_views), Huber's two branches, INVALID, negative u, the percentile threshold, ties, and n = 70 (more
    views than a wave has lanes)."""
    c = CASES[name]
    kp3d, reproj, n_views = native(c)
    k = c["kp2d"].shape[1]
    assert kp3d.shape == (k, 3) and reproj.shape == (k,) and n_views.shape == (k,)
    assert kp3d.dtype == np.float64 and reproj.dtype == np.float64 and n_views.dtype == np.int32
    check_points(name, kp3d, reproj, n_views, c)
    if name == "n8_views_2_3_8":
        assert np.array_equal(c["kp3d"] == -1e6, kp3d == -1e6) and np.array_equal(c["reproj"] == -1e6, reproj == -1e6)


def test_scores_default_to_one(hip_device):
    c = CASES["n8_outliers"]
    a = triang.triangulate_points(c["Ks"], c["Ts"], c["kp2d"])
    b = triang.triangulate_points(c["Ks"], c["Ts"], c["kp2d"], np.ones((8, 133)))
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and (a[2] == 8).all()


def test_two_runs_give_the_same_bits(hip_device):
    for name in ("n8_outliers", "n70_k4", "n30_ties"):
        a, b = native(CASES[name]), native(CASES[name])
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), name


def test_a_batch_equals_its_frames_run_singly(hip_device):
    frames = [CASES[f"batch3_f{t}"] for t in range(3)]
    kp3d, reproj, n_views = triang.triangulate_points(frames[0]["Ks"], frames[0]["Ts"], np.stack([c["kp2d"] for c in frames]),
                                                      np.stack([c["score"] for c in frames]))
    assert kp3d.shape == (3, 133, 3) and reproj.shape == (3, 133) and n_views.shape == (3, 133)
    for t, c in enumerate(frames):
        single = native(c)
        assert np.array_equal(kp3d[t], single[0]) and np.array_equal(reproj[t], single[1]) and np.array_equal(n_views[t], single[2]), t
        check_points(c["name"], kp3d[t], reproj[t], n_views[t], c)


def test_projection_is_the_reference_s(hip_device):
    """Four-term fp64 dot products of magnitude <= 1e4 carry about 2e-11 before the division by a depth >= 1, and the summation order of
    the reference's BLAS is not ours: 1e-9 px and 1e-9 in depth.  -1e6 rows are exact."""
    p = REF["projections"][0]
    uv, depth, score = triang.project_points(p["kp3d"], p["Ks"], p["Ts"])
    assert score is None and uv.shape == p["kp2d"].shape and depth.shape == p["depth"].shape
    bad = (p["kp3d"] == -1e6).any(axis=-1)
    assert bad.any() and (uv[:, bad] == -1e6).all() and (depth[:, bad] == -1e6).all()
    assert np.array_equal(uv == -1e6, p["kp2d"] == -1e6) and np.array_equal(depth == -1e6, p["depth"] == -1e6)
    assert np.abs(uv - p["kp2d"]).max() <= 1e-9 and np.abs(depth - p["depth"]).max() <= 1e-9
    # a frame axis, and one coordinate of a point set to -1e6
    pts = np.stack([p["kp3d"], p["kp3d"][::-1]])
    pts[1, 7, 1] = -1e6
    uv2, depth2, _ = triang.project_points(pts, p["Ks"], p["Ts"])
    assert np.array_equal(uv2[0], uv) and np.array_equal(depth2[0], depth)
    assert (uv2[1, :, 7] == -1e6).all() and (depth2[1, :, 7] == -1e6).all()
    keep = np.arange(133) != 7
    assert np.array_equal(uv2[1][:, keep], uv[:, ::-1][:, keep])


def test_face_scores_are_the_reference_s(hip_device):
    p = REF["projections"][1]
    _, _, score = triang.project_points(p["kp3d"], p["Ks"], p["Ts"], kp3d_score=p["kp3d_score"])
    assert score.shape == p["kp2d_score"].shape and np.abs(score - p["kp2d_score"]).max() <= 1e-12
    assert np.array_equal(score[:, 3:23], np.repeat(p["kp3d_score"][None, 3:23], 8, axis=0))


# -- the file route ---------------------------------------------------------------------------------------------------------------
def read_tree(root: Path):
    return {str(p.relative_to(root)): json.loads(p.read_text()) for p in sorted(root.rglob("*.json"))}


def run_scene(name, tmp: Path, **kw):
    return triang.triangulate_skeleton(str(SCENES / name / "transforms.json"), str(SCENES / name / "poses_sapiens"), str(tmp / "poses_3d"),
                                       out_kp2d_proj_dir=str(tmp / "poses_2d"), **kw)


@pytest.mark.parametrize("name", list(REF["scenes"]))
def test_triangulate_skeleton_writes_the_reference_s_files(hip_device, tmp_path, name):
    scene = REF["scenes"][name]
    res = run_scene(name, tmp_path)
    got = read_tree(tmp_path)
    assert sorted(got) == sorted(scene["files"])  # the same file set
    n, frames = len(scene["labels"]), len(scene["frames"])
    assert res["frames"] == frames and res["skipped"] == 0 and res["cameras"] == n and res["cameras_proj"] == n and res["keypoints"] == 133
    assert res["files"] == len(got) and res["valid"] == sum(int((fr["n_views"] >= 3).sum()) for fr in scene["frames"])
    fx_max = scene["Ks"][:, :2, :2].max()
    for path, want in scene["files"].items():
        assert list(got[path]) == ["instance_info"] and len(got[path]["instance_info"]) == 1
        inst = {k: np.array(v) for k, v in got[path]["instance_info"][0].items()}
        assert list(inst) == list(want), path  # the same keys in the same order
        fr = scene["frames"][int(Path(path).stem)]
        if path.startswith("poses_3d"):
            invalid = fr["n_views"] < 3
            assert np.array_equal((want["keypoints"] == -1e6).any(axis=-1), invalid)
            check_points(path, inst["keypoints"], inst["keypoint_reproj"], fr["n_views"], fr)
        else:
            # a point moved by d shifts its projection by at most (f / depth) d pixels and its depth by at most d
            assert np.array_equal(inst["keypoints"] == -1e6, want["keypoints"] == -1e6), path
            assert np.array_equal(inst["keypoint_depths"] == -1e6, want["keypoint_depths"] == -1e6), path
            d = fr["d_ref_m"] + fr["d_conv_m"]
            min_depth = want["keypoint_depths"][want["keypoint_depths"] != -1e6].min()
            assert min_depth > 1.0
            assert np.abs(inst["keypoints"] - want["keypoints"]).max() <= (fx_max / min_depth) * d + 1e-9, path
            assert np.abs(inst["keypoint_depths"] - want["keypoint_depths"]).max() <= d + 1e-9, path


def test_projection_subset_skip_exists_and_point_clouds(hip_device, tmp_path):
    full = tmp_path / "full"
    run_scene("ring8", full)
    sub = tmp_path / "sub"
    res = triang.triangulate_skeleton(str(SCENES / "ring8" / "transforms.json"), str(SCENES / "ring8" / "poses_sapiens"), str(sub / "poses_3d"),
                                      out_pcd_dir=str(sub / "poses_pcd"), out_kp2d_proj_dir=str(sub / "poses_2d"), spa_labels_proj=[1, 6],
                                      tem_labels=[1])
    assert res["frames"] == 1 and res["cameras_proj"] == 2 and res["files"] == 4
    want = read_tree(full)
    got = read_tree(sub)
    assert sorted(got) == ["poses_2d/01/000001.json", "poses_2d/06/000001.json", "poses_3d/000001.json"]
    for path in got:
        assert got[path] == want[path], path  # the same bits as in the full run
    from vhull_model import read_ply
    _, pts, colors = read_ply(sub / "poses_pcd" / "000001.ply")
    kp3d = np.array(got["poses_3d/000001.json"]["instance_info"][0]["keypoints"])
    assert np.array_equal(pts, kp3d.astype(np.float32)) and (colors == 255).all() and (pts == np.float32(-1e6)).any()
    # skip_exists: a valid file stays as it is (with everything that belongs to its frame), a broken one is made again
    marker = {"instance_info": [{"keypoints": [], "keypoint_reproj": [], "marker": 1}]}
    (full / "poses_3d" / "000000.json").write_text(json.dumps(marker))
    (full / "poses_3d" / "000001.json").write_text("{ broken")
    (full / "poses_2d" / "03" / "000000.json").unlink()
    res = run_scene("ring8", full, skip_exists=True)
    assert res["frames"] == 1 and res["skipped"] == 1
    assert json.loads((full / "poses_3d" / "000000.json").read_text()) == marker and not (full / "poses_2d" / "03" / "000000.json").exists()
    assert json.loads((full / "poses_3d" / "000001.json").read_text()) == want["poses_3d/000001.json"]
    # a subset of the views gives other points: the cameras are matched to transforms.json by label
    half = tmp_path / "half"
    triang.triangulate_skeleton(str(SCENES / "ring8" / "transforms.json"), str(SCENES / "ring8" / "poses_sapiens"), str(half / "poses_3d"),
                                spa_label_range=(0, 8, 2), tem_labels=[0])
    scene = REF["scenes"]["ring8"]
    labels = scene["labels"][::2]
    read = [triang.read_kp2d(str(SCENES / "ring8" / "poses_sapiens" / lab / "000000.json")) for lab in labels]
    direct = triang.triangulate_points(scene["Ks"][::2], scene["Ts"][::2], np.stack([r[0] for r in read]), np.stack([r[2] for r in read]))
    inst = json.loads((half / "poses_3d" / "000000.json").read_text())["instance_info"][0]
    assert np.array_equal(np.array(inst["keypoints"]), direct[0]) and np.array_equal(np.array(inst["keypoint_reproj"]), direct[1])
    assert sorted(p.name for p in half.iterdir()) == ["poses_3d"]


def test_padding_and_intrinsic_scale(hip_device, tmp_path):
    """kp2d_padding is added to every observation and intri_scale multiplies K (K[2, 2] stays 1), for triangulation and projection
    alike: the files hold the bits of the direct calls with those inputs."""
    scene = REF["scenes"]["ring8"]
    read = [triang.read_kp2d(str(SCENES / "ring8" / "poses_sapiens" / lab / "000000.json")) for lab in scene["labels"]]
    kp2d, score = np.stack([r[0] for r in read]), np.stack([r[2] for r in read])
    run_scene("ring8", tmp_path, kp2d_padding=[3.0, -2.0], intri_scale=2.0, tem_labels=[0])
    K = scene["Ks"] * 2.0
    K[:, 2, 2] = 1.0
    direct = triang.triangulate_points(K, scene["Ts"], kp2d + np.array([3.0, -2.0]), score)
    inst = json.loads((tmp_path / "poses_3d" / "000000.json").read_text())["instance_info"][0]
    assert np.array_equal(np.array(inst["keypoints"]), direct[0])
    uv, depth, _ = triang.project_points(direct[0], K, scene["Ts"])
    got = json.loads((tmp_path / "poses_2d" / "05" / "000000.json").read_text())["instance_info"][0]
    assert np.array_equal(np.array(got["keypoints"]), uv[5]) and np.array_equal(np.array(got["keypoint_depths"]), depth[5])


def test_cli_writes_the_same_files(hip_device, tmp_path):
    run_scene("ring8", tmp_path / "fn")
    out = tmp_path / "cli"
    cmd = [sys.executable, str(ROOT / "tools" / "triangulate_skeleton.py"), "--camera_path", str(SCENES / "ring8" / "transforms.json"),
           "--kp2d_dir", str(SCENES / "ring8" / "poses_sapiens"), "--out_kp3d_dir", str(out / "poses_3d"), "--out_kp2d_proj_dir",
           str(out / "poses_2d"), "--spa_label_range", "0,8,1", "--tem_labels", "0,1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert read_tree(out) == read_tree(tmp_path / "fn")
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["frames"] == 2 and res["cameras"] == 8 and res["files"] == 18
