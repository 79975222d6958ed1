"""CPU: the host half of skeleton triangulation (diffuman4d_amd/host/triang.py) and the numpy model of its kernels
(tests/triang_model.py) against the reference's recorded results (tests/golden/triang_reference.pt, made by
tests/golden/make_golden_triang.py from the reference's own triangulate_points, project_points and triangulate_skeleton on
tests/golden/triang_scene).

The bound on a triangulated point is the reference's own measured distance from the minimiser of its cost, read from the fixture:
|x - converged| <= d_ref + d_conv per case, as a Euclidean distance in metres for the point and in pixels for reproj."""
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import triang_model
from diffuman4d_amd.host import capture
from diffuman4d_amd.host import lib as L
from diffuman4d_amd.host import triang

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
SCENES = GOLDEN / "triang_scene"
REF = torch.load(GOLDEN / "triang_reference.pt", weights_only=False)
CASES = {c["name"]: c for c in REF["cases"]}
ENTRIES = ("dm4d_triangulate_points_f64", "dm4d_project_points_f64")


def reference_thresholds(score, score_thr=0.6, max_views=24):
    """triangulate_one_point's expression (triang_utils.py:66-70), one keypoint column at a time."""
    n = score.shape[0]
    max_views = min(max_views, n)
    return np.array([max(score_thr, np.percentile(score[:, i], 100 * (1 - max_views / n))) for i in range(score.shape[1])])


# -- the model, held to the bound the kernels get -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_model_is_within_the_reference_s_own_distance_from_the_minimiser(name):
    c = CASES[name]
    thr = triang.score_thresholds(c["score"])
    kp3d, reproj, n_views = triang_model.triangulate(c["Ks"], c["Ts"], c["kp2d"][None], c["score"][None], thr[None])
    kp3d, reproj, n_views = kp3d[0], reproj[0], n_views[0]
    assert np.array_equal(n_views, c["n_views"])
    invalid = (c["kp3d"] == -1e6).any(axis=-1)
    assert np.array_equal((kp3d == -1e6).all(axis=-1), invalid) and np.array_equal(reproj == -1e6, invalid)
    assert np.array_equal(invalid, c["n_views"] < 3) and np.array_equal(c["reproj"] == -1e6, invalid)
    e_m = np.linalg.norm(kp3d[~invalid] - c["kp3d_converged"][~invalid], axis=-1).max()
    e_px = np.abs(reproj[~invalid] - c["reproj_converged"][~invalid]).max()
    print(f"{name}: point {e_m:.2e} m (bound {c['d_ref_m'] + c['d_conv_m']:.2e}), reproj {e_px:.2e} px (bound {c['d_ref_px'] + c['d_conv_px']:.2e})")
    assert e_m <= c["d_ref_m"] + c["d_conv_m"]
    assert e_px <= c["d_ref_px"] + c["d_conv_px"]


def test_model_projection_matches_the_reference():
    p = REF["projections"][0]
    uv, depth = triang_model.project(p["kp3d"][None], p["Ks"], p["Ts"])
    bad = (p["kp3d"] == -1e6).any(axis=-1)
    assert bad.any() and not bad.all()
    assert (uv[0][:, bad] == -1e6).all() and (depth[0][:, bad] == -1e6).all()
    assert np.array_equal(uv[0] == -1e6, p["kp2d"] == -1e6) and np.array_equal(depth[0] == -1e6, p["depth"] == -1e6)
    assert np.abs(uv[0] - p["kp2d"]).max() <= 1e-9 and np.abs(depth[0] - p["depth"]).max() <= 1e-9


def test_fixture_covers_what_it_is_for():
    assert set(CASES["n3_min_views"]["n_views"].tolist()) == {3}
    assert np.array_equal(triang.score_thresholds(CASES["n3_min_views"]["score"]), CASES["n3_min_views"]["score"].min(axis=0))
    assert CASES["n8_clean"]["reproj"].max() < 1e-6  # the scene projects without the 1e-9 of the reference's denominator: 2e-7 px
    assert set(CASES["n8_views_2_3_8"]["n_views"].tolist()) == {2, 3, 8}
    neg = CASES["n8_negative_u"]
    assert ((neg["kp2d"][2, :, 0] < 0) & (neg["score"][2] >= triang.score_thresholds(neg["score"]))).sum() >= 10
    assert (triang.score_thresholds(CASES["n30_percentile"]["score"]) > 0.6).all() and set(CASES["n30_percentile"]["n_views"].tolist()) == {24}
    assert CASES["n30_ties"]["n_views"].min() > 24
    assert CASES["n70_k4"]["kp2d"].shape == (70, 4, 2) and CASES["n70_k4"]["n_views"].tolist() == [24, 70, 24, 2]
    out = CASES["n8_outliers"]  # Huber's linear branch is in use at the minimum
    P = triang_model.projections(out["Ks"], out["Ts"])
    h = np.einsum("nrc,kc->nkr", P[:, :, :3], out["kp3d_converged"]) + P[:, None, :, 3]
    r = (h[..., :2] / (h[..., 2:] + 1e-9) - out["kp2d"]) * np.sqrt(out["score"])[..., None]
    assert (np.abs(r).max(axis=(0, 2)) > 10).sum() >= 30
    for c in REF["cases"]:
        assert c["d_conv_m"] <= 1e-3 * c["d_ref_m"] or c["d_conv_m"] < 1e-12
        assert c["d_ref_m"] <= 1e-6
    for scene in REF["scenes"].values():
        assert scene["ref_cpu_seconds_per_frame"] > 0
        for fr in scene["frames"]:
            assert 0 < (fr["n_views"] >= 3).sum() < 133  # the right hand's fingers are INVALID in the file route


# -- host: threshold, cameras, files, labels ------------------------------------------------------------------------------------------
def test_thresholds_equal_the_reference_expression_bit_for_bit():
    for c in REF["cases"]:
        assert np.array_equal(triang.score_thresholds(c["score"]), reference_thresholds(c["score"])), c["name"]
    batch = np.stack([CASES[f"batch3_f{t}"]["score"] for t in range(3)])
    got = triang.score_thresholds(batch)
    assert got.shape == (3, 133)
    for t in range(3):
        assert np.array_equal(got[t], reference_thresholds(batch[t]))
    rng = np.random.default_rng(0)
    for n in (3, 5, 24, 25, 48, 70):
        s = np.round(rng.uniform(0.3, 1.0, size=(2, n, 17)), 2)  # two decimals: many ties
        for f in range(2):
            assert np.array_equal(triang.score_thresholds(s)[f], reference_thresholds(s[f])), n
    assert np.array_equal(triang.score_thresholds(batch[0], score_thr=0.9), reference_thresholds(batch[0], score_thr=0.9))


@pytest.mark.parametrize("name", list(REF["scenes"]))
def test_cameras_are_the_reference_s(name):
    scene = REF["scenes"][name]
    Ks, Ts = triang.scene_cameras(str(SCENES / name / "transforms.json"), scene["labels"])
    assert Ks.dtype == np.float64 and Ts.dtype == np.float64
    assert np.array_equal(Ks, scene["Ks"])
    assert np.array_equal(Ks, Ks.astype(np.float32).astype(np.float64))  # float32 values, widened
    # the inverse is taken by LAPACK in float32 and builds may differ: 2 float32 ulp at the size of each matrix's largest entry
    ulp = np.spacing(np.abs(scene["Ts"]).max(axis=(1, 2)).astype(np.float32)).astype(np.float64)
    assert (np.abs(Ts - scene["Ts"]) <= 2 * ulp[:, None, None]).all()
    sub_K, sub_T = triang.scene_cameras(str(SCENES / name / "transforms.json"), scene["labels"][::3])
    assert np.array_equal(sub_K, Ks[::3]) and np.array_equal(sub_T, Ts[::3])
    Ks2, Ts2 = triang.scene_cameras(str(SCENES / name / "transforms.json"), scene["labels"], intri_scale=0.5)
    assert np.array_equal(Ks2[:, :2], Ks[:, :2] * 0.5) and (Ks2[:, 2, 2] == 1.0).all() and np.array_equal(Ts2, Ts)
    with pytest.raises(ValueError, match="camera_label"):
        triang.scene_cameras(str(SCENES / name / "transforms.json"), ["00", "77"])


def test_read_cameras_keeps_its_default():
    path = str(SCENES / "ring8" / "transforms.json")
    default, normalised, raw = capture.read_cameras(path), capture.read_cameras(path, normalize_scene=True), capture.read_cameras(path, normalize_scene=False)
    tf = {fr["camera_label"]: fr for fr in json.loads(Path(path).read_text())["frames"]}
    for lab in default:
        assert torch.equal(default[lab]["pose"], normalised[lab]["pose"]) and torch.equal(default[lab]["K"], raw[lab]["K"])
        assert torch.equal(raw[lab]["pose"][:3, 3], torch.tensor(tf[lab]["transform_matrix"])[:3, 3])
        assert not torch.equal(raw[lab]["pose"][:3, 3], default[lab]["pose"][:3, 3])
        assert torch.equal(raw[lab]["pose"][:3, :3], default[lab]["pose"][:3, :3])


def test_label_parsing_and_its_errors(tmp_path):
    assert triang._labels([3, "7"], None, "spa_labels", "spa_label_range", 2, None) == ["03", "07"]
    assert triang._labels(None, (0, 8, 3), "spa_labels", "spa_label_range", 2, None) == ["00", "03", "06"]
    assert triang._labels(None, (5, 20, 5), "tem_labels", "tem_label_range", 6, None) == ["000005", "000010", "000015"]
    assert triang._labels(None, None, "spa_labels", "spa_label_range", 2, lambda: ["a"]) == ["a"]
    kw = dict(camera_path=str(SCENES / "ring8" / "transforms.json"), kp2d_dir=str(SCENES / "ring8" / "poses_sapiens"),
              out_kp3d_dir=str(tmp_path / "poses_3d"))
    with pytest.raises(ValueError, match="^spa_labels and spa_label_range cannot be specified together$"):
        triang.triangulate_skeleton(spa_labels=[0, 1, 2], spa_label_range=(0, 8, 1), **kw)
    with pytest.raises(ValueError, match="^spa_labels_proj and spa_label_proj_range cannot be specified together$"):
        triang.triangulate_skeleton(spa_labels_proj=[0], spa_label_proj_range=(0, 8, 1), **kw)
    with pytest.raises(ValueError, match="^tem_labels and tem_label_range cannot be specified together$"):
        triang.triangulate_skeleton(tem_labels=[0], tem_label_range=(0, 2, 1), **kw)
    assert not (tmp_path / "poses_3d").exists()


def test_read_kp2d_rescales_the_fingers_and_requires_scores(tmp_path):
    rng = np.random.default_rng(1)
    kp, score = rng.uniform(0, 1000, size=(133, 2)), rng.uniform(0.2, 1.0, size=133)
    (tmp_path / "a.json").write_text(json.dumps({"instance_info": [{"keypoints": kp.tolist(), "keypoint_scores": score.tolist()}]}))
    got_kp, got_depth, got_score = triang.read_kp2d(str(tmp_path / "a.json"))
    want = score.copy()
    want[92:112] *= want[91] ** 2
    want[113:133] *= want[112] ** 2
    assert got_depth is None and got_kp.dtype == np.float64 and np.array_equal(got_kp, kp) and np.array_equal(got_score, want)
    assert np.array_equal(got_score[:92], score[:92]) and got_score[112] == score[112] and not np.array_equal(got_score[113:], score[113:])
    (tmp_path / "b.json").write_text(json.dumps({"instance_info": [{"keypoints": kp.tolist(), "keypoint_depths": score.tolist()}]}))
    with pytest.raises(ValueError, match="keypoint_scores"):
        triang.read_kp2d(str(tmp_path / "b.json"))
    # a scene file: what the reference handed to triangulate_points is what read_kp2d returns
    first = triang.read_kp2d(str(SCENES / "ring8" / "poses_sapiens" / "00" / "000000.json"))
    assert first[0].shape == (133, 2) and first[2][113:].max() < 0.6 * 0.6 + 1e-12


def test_written_files_parse_back_equal(tmp_path):
    rng = np.random.default_rng(2)
    kp, depth, score = rng.standard_normal((133, 2)) * 500, rng.uniform(1, 4, size=133), rng.uniform(size=133)
    kp[5], depth[5] = -1e6, -1e6
    triang.write_kp2d(str(tmp_path / "x" / "y" / "k.json"), kp, depth)
    text = (tmp_path / "x" / "y" / "k.json").read_text()
    inst = json.loads(text)["instance_info"]
    assert len(inst) == 1 and list(inst[0]) == ["keypoints", "keypoint_depths"] and text.startswith('{\n    "instance_info": [\n        {')
    assert np.array_equal(np.array(inst[0]["keypoints"]), kp) and np.array_equal(np.array(inst[0]["keypoint_depths"]), depth)
    triang.write_kp2d(str(tmp_path / "s.json"), kp, None, score)
    assert list(json.loads((tmp_path / "s.json").read_text())["instance_info"][0]) == ["keypoints", "keypoint_scores"]
    kp3d, reproj = rng.standard_normal((133, 3)), rng.uniform(size=133)
    triang.write_kp3d(str(tmp_path / "p" / "3.json"), kp3d, reproj)
    inst = json.loads((tmp_path / "p" / "3.json").read_text())["instance_info"][0]
    assert list(inst) == ["keypoints", "keypoint_reproj"]
    assert np.array_equal(np.array(inst["keypoints"]), kp3d) and np.array_equal(np.array(inst["keypoint_reproj"]), reproj)


# -- arguments and ABI ----------------------------------------------------------------------------------------------------------------
def test_shape_checks_use_the_reference_s_texts():
    c = CASES["n3_min_views"]
    with pytest.raises(ValueError, match=r"^min_views should be at least 3, got 2\.$"):
        triang.triangulate_points(c["Ks"], c["Ts"], c["kp2d"], c["score"], min_views=2)
    with pytest.raises(ValueError, match=r"^kp2d must have shape \(n, k, 2\), got \(3, 133, 3\)$"):
        triang.triangulate_points(c["Ks"], c["Ts"], np.zeros((3, 133, 3)), c["score"])
    with pytest.raises(ValueError, match=r"^kp2d_score must have shape \(n, k\), got \(3, 132\)$"):
        triang.triangulate_points(c["Ks"], c["Ts"], c["kp2d"], c["score"][:, :132])
    with pytest.raises(ValueError, match=r"^Ks must have shape \(n, 3, 3\), got \(2, 3, 3\)$"):
        triang.triangulate_points(c["Ks"][:2], c["Ts"], c["kp2d"], c["score"])
    with pytest.raises(ValueError, match=r"^Ts must have shape \(n, 4, 4\), got \(3, 3, 4\)$"):
        triang.triangulate_points(c["Ks"], c["Ts"][:, :3], c["kp2d"], c["score"])
    with pytest.raises(ValueError, match=r"^kp2d_score must have shape \(n, k\), got \(3, 133\)$"):
        triang.triangulate_points(c["Ks"], c["Ts"], c["kp2d"][None], c["score"])  # a frame axis on one of the two only


def test_there_is_no_cpu_path(tmp_path):
    c = CASES["n3_min_views"]
    for device in ("cpu", "cuda"):  # no HIP device on this machine either way
        if device == "cuda" and torch.cuda.is_available():
            continue
        with pytest.raises(L.Dm4dError, match="HIP device"):
            triang.triangulate_points(c["Ks"], c["Ts"], c["kp2d"], c["score"], device=device)
        with pytest.raises(L.Dm4dError, match="HIP device"):
            triang.project_points(c["kp3d"], c["Ks"], c["Ts"], device=device)
        with pytest.raises(L.Dm4dError, match="HIP device"):
            triang.triangulate_skeleton(str(SCENES / "ring8" / "transforms.json"), str(SCENES / "ring8" / "poses_sapiens"),
                                        str(tmp_path / "poses_3d"), device=device)
    from diffuman4d_amd.host import ops
    t = torch.zeros(3, 3, 3, dtype=torch.float64)
    with pytest.raises(L.Dm4dError, match="HIP device"):
        ops.triangulate_points(t, t, t, t, t, 3)
    with pytest.raises(L.Dm4dError, match="HIP device"):
        ops.project_points(t, t, t)


def test_abi_entries_are_in_header_library_and_table():
    header = (ROOT / "include" / "dm4d.h").read_text()
    lib = L.load()
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert "triang_utils.py" in header and "triangulate_skeleton.py" in header
    from diffuman4d_amd import build
    assert "triang.hip" in build.SOURCES and "-ffp-contract=off" in build.EXTRA_FLAGS["triang.hip"]
