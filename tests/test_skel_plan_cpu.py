"""CPU: the numpy model of dm4d_skeleton_plan_kp3d (tests/skel_plan_model.py) against the file route, record for record -- project ->
write_kp2d -> _read_instance -> plan_draw_calls -> pack_calls -- with dropped_links and the raised errors, on random poses and on the
constructed cases of tests/skel_plan_cases.py; the per-palette tables and per-map parameters the host builds; and the host wiring
(job lists, shape grouping, error mapping, draw_skeleton(kp3d_dir=...), SpaTemDataset(skeleton_source="kp3d"), the config keys) on the
stand-ins of tests/skel_plan_standin.py."""
import json

import numpy as np
import pytest
import torch

import kp2d_scene as ks
import skel_plan_cases as sc
import skel_plan_model as model
import skel_plan_standin as standin
from diffuman4d_amd.host import capture, config, ops, skeleton, triang

CASES = sc.cases()


def model_plan(case):
    uv, depth = sc.project(case.kp3d)
    tables = skeleton.plan_tables(case.palette)
    p = skeleton.map_params(case.shapes)
    return model.plan(uv, depth, case.scores, p.scale_ratio, p.offset, p.radius, p.thickness, tables.links, tables.colors, tables.low_thr,
                      tables.high_thr, tables.thr_span), tables


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_model_equals_the_file_route(case, tmp_path):
    want = sc.file_route(case, tmp_path)
    (records, bits, dropped), tables = model_plan(case)
    err = skeleton.plan_error(bits, tables)
    if case.error is not None:
        assert isinstance(want, ValueError) and str(want) == case.error
        assert type(err) is ValueError and str(err) == case.error
        return
    assert not isinstance(want, Exception), want
    assert err is None and bits == 0
    assert dropped == want[1]
    assert records.shape == want[0].shape and np.array_equal(records, want[0]), np.argwhere(records != want[0])[:5]


def test_the_cases_reach_what_they_are_built_for(tmp_path):
    """Each constructed case exercises its branch: ties under both sorts, list order, both parities of half landings, dropped links, ..."""
    by_name = {c.name: c for c in CASES}
    plans = {name: model_plan(c)[0] for name, c in by_name.items()}
    assert plans["outside"][2] > 0 and plans["random0"][2] == 0
    assert len(plans["zero_depths"][0]) == 3 * len(sc.LINKS)                       # nothing dropped: list order
    ids = [l["link"] for l in sc.LINKS]
    recs = plans["zero_depths"][0][0::3]
    uv, _ = sc.project(by_name["zero_depths"].kp3d)
    assert [tuple(r[1:3]) for r in recs.tolist()] == [tuple(np.rint(uv[i1].astype(np.float32) * 2.0).astype(int)) for i1, _ in ids]
    half = by_name["half_landings"]
    uv, _ = sc.project(half.kp3d)
    frac = (uv[:, 0].astype(np.float32).astype(np.float64) * 2) % 1
    assert (frac == 0.5).all() and len({int(np.floor(v * 2)) % 2 for v in uv[:, 0]}) == 2
    def line_ends(name):  # the lines' end points in paint order, and in list order
        uv, _ = sc.project(by_name[name].kp3d)
        p = skeleton.map_params(by_name[name].shapes)
        xy = np.rint(uv.astype(np.float32).astype(np.float64) * p.scale_ratio + p.offset).astype(int)
        return [r[1:5] for r in plans[name][0][0::3].tolist()], [[*xy[i1], *xy[i2]] for i1, i2 in ids]
    painted, listed = line_ends("one_depth")           # every key ties: a stable sort keeps the list order
    assert painted == listed
    for name in ("equal_depths", "zero_depths_scores"):  # three key values: sorted, so not the list order, with long runs of ties
        painted, listed = line_ends(name)
        assert len(painted) > 10 and painted != listed and sorted(painted) == sorted(l for l in listed if l in painted)
    assert 0 < len(plans["threshold_scores"][0]) < 3 * len(sc.LINKS)
    assert len(plans["behind_camera"][0]) < len(plans["behind_camera_positive_uv"][0]) == 3 * len(sc.LINKS)
    assert plans["nan_dropped"][1] == 0 and plans["colourless_dropped"][1] == 0


def test_numpy_promotes_float32_times_float64_scalar_to_float64():
    """The definition's scaling step: under NumPy 2 a float32 array times an np.float64 scalar is float64 (NumPy 1.x keeps float32)."""
    assert (np.ones(2, np.float32) * np.float64(2.0)).dtype == np.float64


# -- tables and parameters ----------------------------------------------------------------------------------------------------------------
def test_plan_tables():
    t = skeleton.plan_tables(sc.PALETTE)
    L, k = len(sc.LINKS), sc.K_PTS
    assert t.links.shape == (L, ops.SKEL_LINK_FIELDS) and t.links.dtype == np.int32 and t.colors.shape == (k + L, 4) and t.n_keypoints == k
    assert [l["id"] for l in sc.LINKS[-2:]] == [65, 66] and t.links[-2:, :3].tolist() == [[5, 12, 65], [6, 11, 66]]
    assert t.colors[k + L - 1, :3].tolist() == sc.PALETTE.x_link_color and (t.colors[:, 3] == 1).all()
    for row, l in zip(t.links.tolist(), sc.LINKS):
        assert row == [*l["link"], l["id"], *([2, 2] if l["id"] < skeleton.MAJOR_LINKS else [1, 1]), 0, 0, 0]
    assert t.low_thr == float(np.float32(0.5)) and t.high_thr == float(np.float32(0.9)) and t.thr_span == float(np.float32(0.9 - 0.5))
    assert skeleton.plan_tables(t) is t
    t2 = skeleton.plan_tables(sc.with_colourless(7))
    assert t2.colors[7].tolist() == [0, 0, 0, 0] and t2.colors[:k, 3].sum() == k - 1
    data = json.loads(sc.PALETTE_PATH.read_text())
    data["links"][0]["id"] = 500
    with pytest.raises(ValueError, match="link ids must be below the number of links"):
        skeleton.plan_tables(skeleton.make_palette(data))
    data = json.loads(sc.PALETTE_PATH.read_text())
    data["links"] = [{"id": i, "link": [0, 1], "color": [1, 2, 3]} for i in range(171)]
    with pytest.raises(ValueError, match="SKEL_MAX_PRIMS"):
        skeleton.plan_tables(skeleton.make_palette(data))


@pytest.mark.parametrize("shapes", [sc.SQUARE, sc.WIDE, ((1280, 1024), (320, 256)), ((720, 1280), (1024, 1024)), ((4096, 4096), (256, 256))])
def test_map_params_are_plan_draw_calls(shapes):
    inst = {"keypoints": [[10.0, 20.0]] * sc.K_PTS}
    try:
        plan = skeleton.plan_draw_calls(inst, None, shapes, sc.PALETTE)
    except ValueError as e:
        with pytest.raises(ValueError) as got:
            skeleton.map_params(shapes)
        assert str(got.value) == str(e) and "thickness rounds to" in str(e)
        return
    p = skeleton.map_params(shapes)
    assert p.canvas_shape == plan.canvas_shape and p.out_size == plan.out_size
    line, circle = plan.calls[0], plan.calls[1]
    assert (line["thickness"], circle["radius"]) == (2 * p.thickness, 2 * p.radius)
    x = np.float64(np.float32(10.0)) * p.scale_ratio + p.offset
    assert line["p1"][0] == int(np.rint(x))


def test_read_kp3d(tmp_path):
    kp = np.arange(12, dtype=np.float64).reshape(4, 3) / 7
    triang.write_kp3d(tmp_path / "a.json", kp, np.zeros(4))
    assert np.array_equal(skeleton.read_kp3d(tmp_path / "a.json"), kp)
    (tmp_path / "b.json").write_text(json.dumps({"instance_info": [{"keypoints": [[1, 2]]}]}))
    with pytest.raises(ValueError, match=r"\(k, 3\)"):
        skeleton.read_kp3d(tmp_path / "b.json")


# -- host wiring on stand-ins ---------------------------------------------------------------------------------------------------------------
@pytest.fixture
def host_ops(monkeypatch):
    calls = standin.install(monkeypatch)
    return calls


def scene_arrays():
    good = [c for c in CASES if c.error is None and c.scores is None and c.palette is sc.PALETTE][:3]
    kp3d = np.stack([c.kp3d for c in good])
    Ks, Ts = np.stack([sc.K_FLAT, sc.K_FLAT * [[1.5], [1.5], [1.0]]]), np.stack([sc.T_FLAT, sc.T_FLAT])
    return kp3d, Ks, Ts


def test_draw_skeleton_maps_kp3d_groups_by_shape_and_keeps_job_order(host_ops):
    kp3d, Ks, Ts = scene_arrays()
    jobs = [(0, 0), (1, 1), (2, 0), (1, 0)]
    shapes = [sc.SQUARE, sc.WIDE, sc.SQUARE, sc.WIDE]
    maps, dropped = skeleton.draw_skeleton_maps_kp3d(kp3d, Ks, Ts, jobs, shapes, sc.PALETTE, device="cpu")
    assert [m.shape for m in maps] == [(256, 256, 3), (320, 255, 3), (256, 256, 3), (320, 255, 3)] and dropped.tolist() == [0, 0, 0, 0]
    (plan_call,) = host_ops["plan"]
    assert plan_call["jobs"] == [[0, 0], [2, 0], [1, 1], [1, 0]]           # grouped by shape, job order inside a group
    assert [d["n"] for d in host_ops["draw"]] == [2, 2] and [d["hw"] for d in host_ops["draw"]] == [(256, 256), (320, 255)]
    p_sq, p_wide = skeleton.map_params(sc.SQUARE), skeleton.map_params(sc.WIDE)
    assert plan_call["scale"] == [[p_sq.scale_ratio, p_sq.offset]] * 2 + [[p_wide.scale_ratio, p_wide.offset]] * 2
    assert plan_call["sizes"] == [[p_sq.radius, p_sq.thickness]] * 2 + [[p_wide.radius, p_wide.thickness]] * 2
    # every map is the one a single-job call draws, and one shape gives one array
    for i, (job, shape) in enumerate(zip(jobs, shapes)):
        one, _ = skeleton.draw_skeleton_maps_kp3d(kp3d, Ks, Ts, [job], shape, sc.PALETTE, device="cpu")
        assert one.shape == (1, *maps[i].shape) and np.array_equal(one[0], maps[i])
    assert maps[0].any()


def test_draw_skeleton_maps_kp3d_raises_for_the_first_bad_map_in_job_order(host_ops):
    by_name = {c.name: c for c in CASES}
    kp3d = np.stack([by_name["random0"].kp3d, by_name["nan_kept"].kp3d, by_name["colourless"].kp3d])
    Ks, Ts = sc.K_FLAT[None], sc.T_FLAT[None]
    palette = by_name["colourless"].palette
    jobs, shapes = [(0, 0), (2, 0), (1, 0)], [sc.WIDE, sc.SQUARE, sc.WIDE]  # grouping plans the NaN frame before the colourless one
    with pytest.raises(ValueError) as e:
        skeleton.draw_skeleton_maps_kp3d(kp3d, Ks, Ts, jobs, shapes, palette, device="cpu")
    assert str(e.value) == by_name["colourless"].error
    with pytest.raises(ValueError) as e:
        skeleton.draw_skeleton_maps_kp3d(kp3d, Ks, Ts, jobs[::-1], shapes[::-1], palette, device="cpu")
    assert str(e.value) == "a keypoint of a drawn link is not finite"
    assert len(host_ops["plan"]) == 2  # one plan launch a call


def test_draw_skeleton_maps_kp3d_argument_errors(host_ops):
    kp3d, Ks, Ts = scene_arrays()
    with pytest.raises(ValueError, match="does not matches that of keypoints"):
        skeleton.draw_skeleton_maps_kp3d(kp3d[:, :100], Ks, Ts, [(0, 0)], sc.SQUARE, sc.PALETTE, device="cpu")
    with pytest.raises(ValueError, match="thickness rounds to 0"):
        skeleton.draw_skeleton_maps_kp3d(kp3d, Ks, Ts, [(0, 0)], ((8192, 8192), (256, 256)), sc.PALETTE, device="cpu")
    with pytest.raises(ValueError, match="max\\(out_kpmap_shape\\) must lie in"):
        skeleton.draw_skeleton_maps_kp3d(kp3d, Ks, Ts, [(0, 0)], ((1024, 1024), (64, 64)), sc.PALETTE, device="cpu")
    with pytest.raises(ValueError, match="frame index outside"):
        skeleton.draw_skeleton_maps_kp3d(kp3d, Ks, Ts, [(3, 0)], sc.SQUARE, sc.PALETTE, device="cpu")
    with pytest.raises(ValueError, match="camera index outside"):
        skeleton.draw_skeleton_maps_kp3d(kp3d, Ks, Ts, [(0, 2)], sc.SQUARE, sc.PALETTE, device="cpu")
    with pytest.raises(ValueError, match="one .* pair or 2 of them"):
        skeleton.draw_skeleton_maps_kp3d(kp3d, Ks, Ts, [(0, 0), (1, 0)], [sc.SQUARE] * 3, sc.PALETTE, device="cpu")
    with pytest.raises(ValueError, match="scores must have shape"):
        skeleton.draw_skeleton_maps_kp3d(kp3d, Ks, Ts, [(0, 0)], sc.SQUARE, sc.PALETTE, scores=np.ones((1, 5), np.float32), device="cpu")


# -- draw_skeleton(kp3d_dir=...) -------------------------------------------------------------------------------------------------------------
@pytest.fixture
def kp3d_scene(tmp_path):
    """ring8's cameras at 256 x 256 with a poses_3d directory of two frames made of the flat-camera cases (any pose does: the listing,
    the labels and the skipping are what is looked at)."""
    d = ks.write_cameras_and_detections(tmp_path, (256, 256))
    good = [c for c in CASES if c.error is None and c.palette is sc.PALETTE]
    for frame, c in zip(ks.FRAMES, good):
        triang.write_kp3d(d / "poses_3d" / f"{frame}.json", c.kp3d, np.zeros(sc.K_PTS))
    return d


def test_draw_skeleton_from_kp3d_lists_and_skips(host_ops, kp3d_scene, monkeypatch):
    d = kp3d_scene
    monkeypatch.setattr(skeleton._l, "hip_device", lambda device, what: torch.device("cpu"))
    kw = dict(kp2d_dir=None, out_kpmap_dir=str(d / "skeletons"), kp2d_canvas_shape=(256, 256), out_kpmap_shape=(256, 256), image_ext=".png",
              palette=sc.PALETTE, kp3d_dir=str(d / "poses_3d"), camera_path=str(d / "transforms.json"))
    counts = skeleton.draw_skeleton(spa_labels=[1, 4, 6], **kw)
    assert counts["frames"] == 6 and counts["files"] == 6 and counts["skipped"] == 0
    assert sorted(p.relative_to(d / "skeletons").as_posix() for p in (d / "skeletons").rglob("*.png")) == [
        f"{cam}/{frame}.png" for cam in ("01", "04", "06") for frame in ks.FRAMES]
    assert host_ops["plan"][-1]["jobs"] == [[f, c] for c in range(3) for f in range(2)]  # cameras outermost, as the file route lists them
    # without labels: every camera of transforms.json and every frame of poses_3d; what exists and verifies is skipped
    (d / "skeletons" / "04" / f"{ks.FRAMES[1]}.png").write_bytes(b"broken")
    counts = skeleton.draw_skeleton(skip_exists=True, **kw)
    assert counts["frames"] == 8 * 2 - 5 and counts["skipped"] == 5 and counts["files"] == 11
    from PIL import Image
    Image.open(d / "skeletons" / "04" / f"{ks.FRAMES[1]}.png").verify()
    counts = skeleton.draw_skeleton(skip_exists=True, tem_labels=[1], **kw)
    assert counts == {"frames": 0, "skipped": 8, "files": 0, "dropped_links": 0}
    with pytest.raises(ValueError, match="camera_path"):
        skeleton.draw_skeleton(**{**kw, "camera_path": None})


# -- SpaTemDataset(skeleton_source="kp3d") -------------------------------------------------------------------------------------------------------
def test_dataset_argument_errors(kp3d_scene):
    root = kp3d_scene.parent
    kw = dict(data_dir=str(root), scene_label=ks.SCENE, height=64, width=64)
    assert capture.SKELETON_SOURCES == ("files", "kp2d", "kp3d")
    with pytest.raises(ValueError) as e:
        capture.SpaTemDataset(skeleton_source="kp4d", **kw)
    assert str(e.value) == "skeleton_source must be one of ('files', 'kp2d', 'kp3d'), got 'kp4d'"
    with pytest.raises(ValueError, match="skeleton_source='kp3d' needs palette="):
        capture.SpaTemDataset(skeleton_source="kp3d", **kw)
    with pytest.raises(ValueError, match="kp2d_canvas_shape must be"):
        capture.SpaTemDataset(skeleton_source="kp3d", palette=sc.PALETTE, kp2d_canvas_shape=(0, 5), **kw)
    ds = capture.SpaTemDataset(skeleton_source="kp3d", palette=sc.PALETTE, **kw)
    assert ds.kp3d_path_pat == "{data_dir}/{scene_label}/poses_3d/{tem_label}.json" == capture.KP3D_PATH_PAT
    ds = capture.SpaTemDataset(skeleton_source="kp3d", palette=sc.PALETTE, kp3d_path_pat="{data_dir}/x/{tem_label}.json", **kw)
    assert ds.get_file_path(ds.kp3d_path_pat, ks.SCENE, "03", "000001") == f"{root}/x/000001.json"


def test_config_keys(kp3d_scene, monkeypatch):
    """data.skeleton_source=kp3d data.kp3d_path_pat=... reach the native class, also where the reference's class imports."""
    import sys
    import types
    assert config.NATIVE_DATASET_KEYS["kp3d_path_pat"] == capture.KP3D_PATH_PAT and config.NATIVE_DATASET_KEYS["skeleton_source"] == "files"
    base = ["exp=demo_3d", f"data.data_dir={kp3d_scene.parent}", f"data.scene_label={ks.SCENE}", "data.height=64", "data.width=64"]
    cfg = config.compose(base + ["data.skeleton_source=kp3d", f"data.palette={sc.PALETTE_PATH}", "data.kp3d_path_pat='{data_dir}/p3/{tem_label}.json'"])

    class Reference:  # a reference class that imports, and does not know the keywords
        def __init__(self, data_dir, camera_path_pat=None, image_path_pat=None, fmask_path_pat=None, skeleton_path_pat=None,
                     scene_label=None, height=1024, width=1024, has_gt_target=True):
            pass
    for name in ("src", "src.data"):
        monkeypatch.setitem(sys.modules, name, types.ModuleType(name))
    mod = types.ModuleType("src.data.spatem_dataset")
    mod.SpaTemDataset = Reference
    monkeypatch.setitem(sys.modules, "src.data.spatem_dataset", mod)
    ds = config.instantiate(cfg["data"])
    assert type(ds) is capture.SpaTemDataset and ds.skeleton_source == "kp3d" and ds.kp3d_path_pat == "{data_dir}/p3/{tem_label}.json"
    # the key at its default asks for nothing new; set to anything else it selects the native class
    assert type(config.instantiate(config.compose(base + [f"data.kp3d_path_pat='{capture.KP3D_PATH_PAT}'"])["data"])) is Reference
    assert type(config.instantiate(config.compose(base + ["data.kp3d_path_pat='{data_dir}/p3/{tem_label}.json'"])["data"])) is capture.SpaTemDataset
    with pytest.raises(ValueError, match="skeleton_source='kp3d' needs palette="):
        config.instantiate(config.compose(base + ["data.skeleton_source=kp3d"])["data"])


# -- the tools ------------------------------------------------------------------------------------------------------------------------------
def _tool(name):
    import importlib.util
    from pathlib import Path
    spec = importlib.util.spec_from_file_location(f"tool_{name}", Path(__file__).resolve().parent.parent / "tools" / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_preprocess_skeleton_from_kp3d_writes_no_poses_2d(monkeypatch, tmp_path):
    mod, calls = _tool("preprocess"), []
    monkeypatch.setattr(mod, "STAGES", {name: (lambda n: lambda *a, **k: calls.append((n, a, k)) or {})(name) for name in mod.STAGES})
    d = str(tmp_path)
    assert mod.main(["--data_dir", d, "--actions", "triangulate_skeleton,draw_skeleton", "--palette", "P", "--skeleton_from", "kp3d"]) == 0
    assert calls[0] == ("triangulate_skeleton", (f"{d}/transforms.json", f"{d}/poses_sapiens", f"{d}/poses_3d"), {"out_pcd_dir": f"{d}/poses_pcd"})
    assert calls[1] == ("draw_skeleton", (None, f"{d}/skeletons"), {"palette": "P", "kp3d_dir": f"{d}/poses_3d", "camera_path": f"{d}/transforms.json"})
    with pytest.raises(ValueError, match="skeleton_from"):
        mod.run(d, ["draw_skeleton"], palette="P", skeleton_from="files")


def test_draw_skeleton_tool_arguments(monkeypatch, tmp_path, capsys):
    mod, seen = _tool("draw_skeleton"), []
    monkeypatch.setattr(skeleton, "draw_skeleton", lambda *a, **k: seen.append((a, k)) or {"frames": 0})
    assert mod.main(["--kp3d_dir", "D3", "--camera_path", "C", "--out_kpmap_dir", "O", "--palette", "P", "--spa_labels", "1,4"]) == 0
    (args, kw), = seen
    assert args == (None, "O") and kw["kp3d_dir"] == "D3" and kw["camera_path"] == "C" and kw["spa_labels"] == [1, 4] and kw["intri_scale"] is None
    for argv in (["--kp3d_dir", "D3"], ["--camera_path", "C", "--kp2d_dir", "D2"], []):
        with pytest.raises(SystemExit):
            mod.main([*argv, "--out_kpmap_dir", "O", "--palette", "P"])
    capsys.readouterr()
