"""GPU: dm4d_skeleton_plan_kp3d against the numpy model and the file route record for record; a map alone against the map in a batch;
draw_skeleton_maps_kp3d and draw_skeleton(kp3d_dir=...) byte for byte against the file route on the poses_2d files triangulate_skeleton
writes; SpaTemDataset(skeleton_source="kp3d") against skeleton_source="kp2d", samples and exceptions, with device_decode off and on."""
import json
import shutil

import numpy as np
import pytest
import torch
from PIL import Image

import kp2d_scene as ks
import skel_plan_cases as sc
import skel_plan_model as model
from diffuman4d_amd.host import capture, ops, skeleton, triang

pytestmark = pytest.mark.gpu

PALETTE = sc.PALETTE
CASES = sc.cases()
CAMS3 = ["01", "04", "06"]
FRAMES3 = ["000000", "000001", "000002"]
OUT = 64

# other GPU modules swap entries of `ops` for host models and may leave them installed (see tests/test_capture_kp2d_gpu.py): the tests
# here are about the device entries and run with the wrappers this module saw when it was imported
GENUINE = {name: getattr(ops, name) for name in ("capture_crop_resize", "skeleton_draw", "skeleton_box_mask", "skeleton_plan_kp3d",
                                                  "skeleton_draw_planned", "project_points")}
assert all(f.__module__ == ops.__name__ for f in GENUINE.values())


@pytest.fixture(autouse=True)
def genuine_ops(monkeypatch):
    for name, f in GENUINE.items():
        monkeypatch.setattr(ops, name, f)


# -- the plan kernel ----------------------------------------------------------------------------------------------------------------------
def plan_on_device(dev, kp3d, Ks, Ts, jobs, params, tables, scores=None):
    """ops.skeleton_plan_kp3d -> (records [n, 3 L, 8], counts [n], status [n, 2]) as numpy."""
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt))
    jobs_h = up(jobs, np.int32)
    scale_h = up([[p.scale_ratio, p.offset] for p in params], np.float64)
    sizes_h = up([[p.radius, p.thickness] for p in params], np.int32)
    links_h, colors_h = torch.from_numpy(tables.links), torch.from_numpy(tables.colors)
    out = ops.skeleton_plan_kp3d(up(kp3d, np.float64).to(dev), up(Ks, np.float64).to(dev), up(Ts, np.float64).to(dev), jobs_h, jobs_h.to(dev),
                                 None if scores is None else up(scores, np.float32).to(dev), scale_h, scale_h.to(dev), sizes_h, sizes_h.to(dev),
                                 links_h, links_h.to(dev), colors_h, colors_h.to(dev), tables.low_thr, tables.high_thr, tables.thr_span)
    return tuple(t.cpu().numpy() for t in out)


def device_projection(dev, kp3d, Ks, Ts):
    uv, depth = ops.project_points(*(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev) for a in (kp3d, Ks, Ts)))
    return uv.cpu().numpy(), depth.cpu().numpy()


def model_of(uv, depth, scores, p, tables):
    return model.plan(uv, depth, scores, p.scale_ratio, p.offset, p.radius, p.thickness, tables.links, tables.colors, tables.low_thr,
                      tables.high_thr, tables.thr_span)


@pytest.fixture(scope="module")
def planned_cases(hip_device):
    """Every constructed case planned on the device, the cases of one palette in one launch -> {name: (records, count, status row, the
    device's (uv, depth))}."""
    out = {}
    for palette in {id(c.palette): c.palette for c in CASES}.values():
        group = [c for c in CASES if c.palette is palette]
        kp3d = np.stack([c.kp3d for c in group])
        scores = np.stack([np.ones(sc.K_PTS, np.float32) if c.scores is None else c.scores for c in group])
        params = [skeleton.map_params(c.shapes) for c in group]
        tables = skeleton.plan_tables(palette)
        rec, cnt, st = plan_on_device(hip_device, kp3d, sc.K_FLAT[None], sc.T_FLAT[None], [(i, 0) for i in range(len(group))], params, tables, scores)
        uv, depth = device_projection(hip_device, kp3d, sc.K_FLAT[None], sc.T_FLAT[None])
        for i, c in enumerate(group):
            out[c.name] = (rec[i], int(cnt[i]), st[i].tolist(), (uv[i, 0], depth[i, 0]))
    return out


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_plan_equals_the_model_and_the_file_route(planned_cases, case, tmp_path):
    rec, count, (bits, dropped), projected = planned_cases[case.name]
    tables = skeleton.plan_tables(case.palette)
    want_rec, want_bits, want_dropped = model_of(*projected, case.scores, skeleton.map_params(case.shapes), tables)
    assert (bits, dropped) == (want_bits, want_dropped)
    assert count == len(want_rec) and np.array_equal(rec[:count], want_rec), np.argwhere(rec[:count] != want_rec)[:5]
    assert not rec[count:].any()  # the slots past the count are zero
    route = sc.file_route(case, tmp_path, projected)
    err = skeleton.plan_error(bits, tables)
    if case.error is not None:
        assert isinstance(route, ValueError) and type(err) is ValueError and str(err) == str(route) == case.error
    else:
        assert err is None and dropped == route[1] and np.array_equal(rec[:count], route[0])


# -- a scene: three frames, three cameras ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(hip_device, tmp_path_factory):
    """ring8 at 1024 x 1024 with a third frame (the first one's detections moved by a pixel and a half), triangulated from all eight
    cameras and projected into three of them: poses_3d and poses_2d as the native triangulate_skeleton writes them."""
    d = ks.write_cameras_and_detections(tmp_path_factory.mktemp("kp3d_scene"), (1024, 1024))
    for cam in ks.CAMS:
        inst = ks.instance(d, cam, "000000", "poses_sapiens")
        inst["keypoints"] = [[x + 1.5, y - 0.5] for x, y in inst["keypoints"]]
        (d / "poses_sapiens" / cam / "000002.json").write_text(json.dumps({"instance_info": [inst]}))
    triang.triangulate_skeleton(str(d / "transforms.json"), str(d / "poses_sapiens"), str(d / "poses_3d"), out_kp2d_proj_dir=str(d / "poses_2d"),
                                spa_labels_proj=[int(c) for c in CAMS3])
    rng = np.random.default_rng(8)
    for cam in CAMS3:
        for frame in FRAMES3:
            p = d / "scores" / cam / f"{frame}.json"
            p.parent.mkdir(parents=True, exist_ok=True)
            p.write_text(json.dumps({"instance_info": [{"keypoint_scores": rng.uniform(0.3, 1.0, 133).tolist()}]}))
    kp3d = np.stack([skeleton.read_kp3d(d / "poses_3d" / f"{f}.json") for f in FRAMES3])
    Ks, Ts = triang.scene_cameras(str(d / "transforms.json"), CAMS3)
    return d, kp3d, Ks, Ts


JOBS = [(f, c) for c in range(3) for f in range(3)]
SHAPES = [sc.SQUARE] * 8 + [sc.WIDE]  # one non-square map in the same call


def paths_of(d, jobs, sub="poses_2d"):
    return [str(d / sub / CAMS3[c] / f"{FRAMES3[f]}.json") for f, c in jobs]


def test_scene_plans_equal_the_model_and_the_file_route(hip_device, scene):
    d, kp3d, Ks, Ts = scene
    tables = skeleton.plan_tables(PALETTE)
    params = [skeleton.map_params(s) for s in SHAPES]
    rec, cnt, st = plan_on_device(hip_device, kp3d, Ks, Ts, JOBS, params, tables)
    uv, depth = device_projection(hip_device, kp3d, Ks, Ts)
    for i, ((f, c), shape) in enumerate(zip(JOBS, SHAPES)):
        want_rec, want_bits, want_dropped = model_of(uv[f, c], depth[f, c], None, params[i], tables)
        assert st[i].tolist() == [want_bits, want_dropped] == [0, want_dropped]
        assert cnt[i] == len(want_rec) > 0 and np.array_equal(rec[i, :cnt[i]], want_rec)
        plan = skeleton.plan_draw_calls(skeleton._read_instance(paths_of(d, [(f, c)])[0]), None, shape, PALETTE)
        assert np.array_equal(rec[i, :cnt[i]], skeleton.pack_calls(plan.calls)) and plan.dropped_links == want_dropped


def test_a_map_alone_equals_the_map_in_the_batch_and_two_runs_agree(hip_device, scene):
    d, kp3d, Ks, Ts = scene
    tables = skeleton.plan_tables(PALETTE)
    params = [skeleton.map_params(s) for s in SHAPES]
    scores = np.random.default_rng(4).uniform(0.3, 1.0, (len(JOBS), 133)).astype(np.float32)
    batch = plan_on_device(hip_device, kp3d, Ks, Ts, JOBS, params, tables, scores)
    again = plan_on_device(hip_device, kp3d, Ks, Ts, JOBS, params, tables, scores)
    assert all(np.array_equal(a, b) for a, b in zip(batch, again))
    for i in (0, 4, 8):
        alone = plan_on_device(hip_device, kp3d, Ks, Ts, JOBS[i:i + 1], params[i:i + 1], tables, scores[i:i + 1])
        assert all(np.array_equal(a[0], b[i]) for a, b in zip(alone, batch)), i  # the whole stride, the padding included
    rev = plan_on_device(hip_device, kp3d, Ks, Ts, JOBS[::-1], params[::-1], tables, scores[::-1].copy())
    assert all(np.array_equal(a[::-1], b) for a, b in zip(rev, batch))


@pytest.mark.parametrize("override", [False, True])
def test_maps_equal_the_file_route_byte_for_byte(hip_device, scene, override):
    d, kp3d, Ks, Ts = scene
    scores = None
    if override:
        scores = np.stack([skeleton._read_scores(p) for p in paths_of(d, JOBS, "scores")])
    maps, dropped = skeleton.draw_skeleton_maps_kp3d(kp3d, Ks, Ts, JOBS, SHAPES, PALETTE, scores=scores, device=hip_device)
    stats = {}
    want = skeleton.draw_skeleton_maps(paths_of(d, JOBS[:8]), paths_of(d, JOBS[:8], "scores") if override else None, *sc.SQUARE, palette=PALETTE,
                                       device=hip_device, stats=stats)
    wide = skeleton.draw_skeleton_maps(paths_of(d, JOBS[8:]), paths_of(d, JOBS[8:], "scores") if override else None, *sc.WIDE, palette=PALETTE,
                                       device=hip_device, stats=stats)
    assert [m.shape for m in maps] == [(256, 256, 3)] * 8 + [(320, 255, 3)]
    for i in range(8):
        assert np.array_equal(maps[i], want[i]), i
    assert np.array_equal(maps[8], wide[0]) and want.any()
    assert int(dropped.sum()) == stats["dropped_links"]
    # into a buffer of the caller's, on the device
    out = torch.full((8, 256, 256, 3), 7, dtype=torch.uint8, device=hip_device)
    got, _ = skeleton.draw_skeleton_maps_kp3d(kp3d, Ks, Ts, JOBS[:8], sc.SQUARE, PALETTE, scores=None if scores is None else scores[:8], out=out)
    assert got is out and np.array_equal(out.cpu().numpy(), want)


def test_draw_skeleton_from_kp3d_writes_the_files_of_the_file_route(hip_device, scene, tmp_path):
    d = scene[0]
    kw = dict(kp2d_canvas_shape=(1024, 1024), out_kpmap_shape=(256, 256), image_ext=".png", palette=PALETTE, device=hip_device)
    a = skeleton.draw_skeleton(str(d / "poses_2d"), str(tmp_path / "a"), kp2d_score_dir=str(d / "scores"), **kw)
    b = skeleton.draw_skeleton(None, str(tmp_path / "b"), kp2d_score_dir=str(d / "scores"), spa_labels=[int(c) for c in CAMS3],
                               kp3d_dir=str(d / "poses_3d"), camera_path=str(d / "transforms.json"), **kw)
    names = sorted(p.relative_to(tmp_path / "a").as_posix() for p in (tmp_path / "a").rglob("*.png"))
    assert names == [f"{c}/{f}.png" for c in CAMS3 for f in FRAMES3] == sorted(p.relative_to(tmp_path / "b").as_posix() for p in (tmp_path / "b").rglob("*.png"))
    for name in names:
        assert np.array_equal(np.asarray(Image.open(tmp_path / "a" / name)), np.asarray(Image.open(tmp_path / "b" / name))), name
    assert (a["frames"], a["files"], a["dropped_links"]) == (b["frames"], b["files"], b["dropped_links"]) == (9, 9, a["dropped_links"])


# -- the dataset ----------------------------------------------------------------------------------------------------------------------------
def reproject(d, dev) -> None:
    """poses_2d of every camera from the poses_3d files, as triangulate_skeleton writes them."""
    Ks, Ts = triang.scene_cameras(str(d / "transforms.json"), ks.CAMS)
    for frame in ks.FRAMES:
        uv, depth, _ = triang.project_points(skeleton.read_kp3d(d / "poses_3d" / f"{frame}.json"), Ks, Ts, device=dev)
        for c, cam in enumerate(ks.CAMS):
            triang.write_kp2d(d / "poses_2d" / cam / f"{frame}.json", uv[c], depth[c])


@pytest.fixture(scope="module")
def roots(hip_device, tmp_path_factory):
    """A scene of kp2d_scene's first size with poses_3d and poses_2d from the native triangulate_skeleton, and a copy of it in which frame
    000000's pose holds a NaN, camera 00's image of that frame is missing and camera 06's mask of it is empty."""
    hw = ks.SIZES[0]
    good = tmp_path_factory.mktemp("kp3d_ds")
    d = ks.write_cameras_and_detections(good, hw)
    triang.triangulate_skeleton(str(d / "transforms.json"), str(d / "poses_sapiens"), str(d / "poses_3d"), out_kp2d_proj_dir=str(d / "poses_2d"))
    ks.write_images_and_masks(d, hw)
    broken = tmp_path_factory.mktemp("kp3d_ds_broken")
    shutil.copytree(d, broken / ks.SCENE)
    b = broken / ks.SCENE
    pose = json.loads((b / "poses_3d" / "000000.json").read_text())
    pose["instance_info"][0]["keypoints"][5][0] = float("nan")
    (b / "poses_3d" / "000000.json").write_text(json.dumps(pose))
    reproject(b, hip_device)
    (b / "images" / "00" / "000000.png").unlink()
    Image.fromarray(np.zeros(hw, np.uint8)).save(b / "fmasks" / "06" / "000000.png")
    return good, broken


def dataset(root, source, **kw):
    return capture.SpaTemDataset(data_dir=str(root), scene_label=ks.SCENE, height=OUT, width=OUT, decode_threads=4, skeleton_source=source,
                                 palette=PALETTE, **{**ks.patterns(), **kw})


def same(a, b):
    assert a["domain"] == b["domain"] and a["labels"] == b["labels"] and a["hws"] == b["hws"] and a["crops"] == b["crops"]
    for k in ("pixel_values", "skeletons", "Ks", "poses", "cond_masks", "plucker_embeds"):
        assert torch.equal(a[k], b[k]), k


TASKS = {"spatial": (["01", "05", "06"], ["000000"]), "temporal": (["03"], ["000000", "000001"])}


@pytest.mark.parametrize("device_decode", [False, True])
@pytest.mark.parametrize("has_gt_target", [True, False])
@pytest.mark.parametrize("task", ["spatial", "temporal"])
def test_kp3d_sample_equals_the_kp2d_sample(roots, task, has_gt_target, device_decode):
    spa, tem = TASKS[task]
    kw = dict(has_gt_target=has_gt_target, device_decode=device_decode)
    want = dataset(roots[0], "kp2d", **kw).get_item(ks.SCENE, spa, tem, ks.INPUTS)
    got = dataset(roots[0], "kp3d", kp2d_path_pat="{data_dir}/{scene_label}/nowhere/{spa_label}/{tem_label}.json", **kw).get_item(ks.SCENE, spa, tem, ks.INPUTS)
    same(got, want)
    assert got["pixel_values"].is_cuda and got["skeletons"].max() > -1.0 and len(got["labels"]) == (3 if task == "spatial" else 4)


def raised(root, source, spa, tem, **kw):
    with pytest.raises(Exception) as e:
        dataset(root, source, **kw).get_item(ks.SCENE, spa, tem, ks.INPUTS)
    return type(e.value), str(e.value)


@pytest.mark.parametrize("device_decode", [False, True])
@pytest.mark.parametrize("spa,tem,cls", [(["00", "01", "05"], ["000000"], FileNotFoundError),   # the image is opened before the plan is made
                                         (["01", "00", "05"], ["000000"], ValueError),          # the plan's error first, the missing image after it
                                         (["06", "07"], ["000000"], ValueError),                # the plan's error before the same frame's empty mask
                                         (["03"], ["000001", "000000"], ValueError)])           # the second frame of four
def test_kp3d_raises_what_kp2d_raises(roots, spa, tem, cls, device_decode):
    want = raised(roots[1], "kp2d", spa, tem, device_decode=device_decode)
    assert raised(roots[1], "kp3d", spa, tem, device_decode=device_decode) == want and want[0] is cls
    if cls is ValueError:
        assert want[1] == "a keypoint of a drawn link is not finite"
