"""CPU: SpaTemDataset(skeleton_source="kp3d") against skeleton_source="kp2d" on the poses_2d files that the projection of the same
poses_3d gives, with every device entry replaced by its numpy stand-in (tests/skel_plan_standin.py for plan and draw, kp2d_scene and
capture_model for the rest): the sample, and the exceptions with their order."""
import json

import numpy as np
import pytest
import torch

import capture_model as cm
import kp2d_scene as ks
import skel_plan_standin as standin
import triang_model
from diffuman4d_amd.host import capture, skeleton, triang

PALETTE = skeleton.load_palette(ks.PALETTE_PATH)
HW = ks.SIZES[0]
OUT = 64


def write_poses(scene, kp3d_by_frame) -> None:
    """poses_3d/{frame}.json and, by the model's projection into every camera, poses_2d/{cam}/{frame}.json as triangulate_skeleton writes them."""
    Ks, Ts = triang.scene_cameras(str(scene / "transforms.json"), ks.CAMS)
    for frame, kp3d in kp3d_by_frame.items():
        triang.write_kp3d(scene / "poses_3d" / f"{frame}.json", kp3d, np.zeros(len(kp3d)))
        with np.errstate(all="ignore"):
            uv, depth = triang_model.project(kp3d[None], Ks, Ts)
        for c, cam in enumerate(ks.CAMS):
            triang.write_kp2d(scene / "poses_2d" / cam / f"{frame}.json", uv[0, c], depth[0, c])


def poses(rng):
    """A cloud the ring's cameras all see, a tenth of it not triangulated."""
    kp3d = rng.uniform(-0.25, 0.25, (133, 3))
    kp3d[rng.random(133) < 0.1] = -1e6
    return kp3d


@pytest.fixture(scope="module")
def scene_root(tmp_path_factory):
    root = tmp_path_factory.mktemp("kp3d_cpu")
    scene = ks.write_cameras_and_detections(root, HW)
    rng = np.random.default_rng(5)
    write_poses(scene, {frame: poses(rng) for frame in ks.FRAMES})
    ks.write_images_and_masks(scene, HW)
    return root


@pytest.fixture
def host_ops(monkeypatch):
    def crop_resize(blob, blob_host, n_frames, desc_off, tab_off, tab_len, H, W, meta=None):
        both = torch.cat([blob, blob_host])
        return cm.standin_crop_resize(both, both, n_frames, blob.numel() + desc_off, blob.numel() + tab_off, tab_len, H, W)
    monkeypatch.setattr(capture.ops, "capture_crop_resize", crop_resize)
    monkeypatch.setattr(capture.ops, "skeleton_draw", ks.standin_skeleton_draw)
    monkeypatch.setattr(capture.ops, "skeleton_box_mask", ks.standin_box_mask)
    return standin.install(monkeypatch, paint=True)


def dataset(root, source, **kw):
    return capture.SpaTemDataset(data_dir=str(root), scene_label=ks.SCENE, device="cpu", decode_threads=4, height=OUT, width=OUT,
                                 skeleton_source=source, palette=PALETTE, **{**ks.patterns(), **kw})


def same(a, b):
    assert a["domain"] == b["domain"] and a["labels"] == b["labels"] and a["hws"] == b["hws"] and a["crops"] == b["crops"]
    for k in ("pixel_values", "skeletons", "Ks", "poses", "cond_masks", "plucker_embeds"):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("has_gt_target", [True, False])
@pytest.mark.parametrize("task", ["spatial", "temporal"])
def test_kp3d_equals_kp2d(scene_root, host_ops, task, has_gt_target):
    spa, tem = ks.TASKS[task]
    want = dataset(scene_root, "kp2d", has_gt_target=has_gt_target).get_item(ks.SCENE, spa, tem, ks.INPUTS)
    got = dataset(scene_root, "kp3d", has_gt_target=has_gt_target).get_item(ks.SCENE, spa, tem, ks.INPUTS)
    same(got, want)
    assert want["skeletons"].max() > -1.0
    (call,) = host_ops["plan"]  # one plan launch a task; a temporal task names each frame's pose once per camera
    n_frames = len(want["labels"])
    assert len(call["jobs"]) == n_frames and sorted({f for f, _ in call["jobs"]}) == list(range(len(tem)))


def test_kp3d_needs_no_poses_2d_directory_and_reads_each_pose_once(scene_root, host_ops, monkeypatch):
    reads = []
    real = skeleton.read_kp3d
    monkeypatch.setattr(skeleton, "read_kp3d", lambda p: reads.append(str(p)) or real(p))
    spa, tem = ks.TASKS["temporal"]
    ds = dataset(scene_root, "kp3d", has_gt_target=False, kp2d_path_pat="{data_dir}/{scene_label}/nowhere/{spa_label}/{tem_label}.json")
    want = dataset(scene_root, "kp2d", has_gt_target=False).get_item(ks.SCENE, spa, tem, ks.INPUTS)
    same(ds.get_item(ks.SCENE, spa, tem, ks.INPUTS), want)
    assert sorted(reads) == [f"{scene_root}/{ks.SCENE}/poses_3d/{t}.json" for t in tem]  # 2 x 2 frames, two reads
    ds.get_item(ks.SCENE, spa, tem, ks.INPUTS)
    assert len(ds._scene_cams) == 1  # the cameras went up once


def test_kp3d_score_override(scene_root, host_ops):
    rng = np.random.default_rng(3)
    scene = scene_root / ks.SCENE
    for cam in ks.CAMS:
        p = scene / "scores" / cam / "000000.json"
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_text(json.dumps({"instance_info": [{"keypoint_scores": rng.uniform(0.3, 1.0, 133).tolist()}]}))
    kw = dict(kp2d_score_path_pat="{data_dir}/{scene_label}/scores/{spa_label}/{tem_label}.json", has_gt_target=False)
    want = dataset(scene_root, "kp2d", **kw).get_item(ks.SCENE, *ks.TASKS["spatial"], ks.INPUTS)
    got = dataset(scene_root, "kp3d", **kw).get_item(ks.SCENE, *ks.TASKS["spatial"], ks.INPUTS)
    same(got, want)
    assert not torch.equal(got["skeletons"], dataset(scene_root, "kp3d", has_gt_target=False).get_item(ks.SCENE, *ks.TASKS["spatial"], ks.INPUTS)["skeletons"])


# -- exceptions: class, text and the first bad frame, as "kp2d" raises them -------------------------------------------------------------------
@pytest.fixture
def broken_root(tmp_path):
    """Frame 000000 holds a NaN keypoint (every camera's plan refuses it); camera 00's image of that frame is missing; camera 06's
    mask of it is empty."""
    scene = ks.write_cameras_and_detections(tmp_path, HW)
    rng = np.random.default_rng(6)
    good, bad = poses(rng), poses(rng)
    bad[5] = (np.nan, 0.0, 0.0)
    write_poses(scene, {"000000": bad, "000001": good})
    ks.write_images_and_masks(scene, HW)
    (scene / "images" / "00" / "000000.png").unlink()
    from PIL import Image
    Image.fromarray(np.zeros(HW, np.uint8)).save(scene / "fmasks" / "06" / "000000.png")
    return tmp_path


def raised(root, source, spa, tem, **kw):
    with pytest.raises(Exception) as e:
        dataset(root, source, **kw).get_item(ks.SCENE, spa, tem, ks.INPUTS)
    return type(e.value), str(e.value)


@pytest.mark.parametrize("spa,tem", [(ks.CAMS, ["000000"]),             # the first frame's image is missing: opened before the plan is made
                                     (["01", "00"], ["000000"]),         # the plan's error at the first frame, the missing image after it
                                     (["03"], ["000001", "000000"]),     # the plan's error at the second frame of four
                                     (ks.CAMS, ["000001"])])             # no error: both routes return
def test_kp3d_raises_what_kp2d_raises(broken_root, host_ops, spa, tem):
    if tem == ["000001"]:
        same(dataset(broken_root, "kp3d").get_item(ks.SCENE, spa, tem, ks.INPUTS), dataset(broken_root, "kp2d").get_item(ks.SCENE, spa, tem, ks.INPUTS))
        return
    want = raised(broken_root, "kp2d", spa, tem)
    assert raised(broken_root, "kp3d", spa, tem) == want
    assert want[0] in (ValueError, FileNotFoundError)


def test_kp3d_plan_error_comes_before_the_same_frames_mask_error(broken_root, host_ops):
    """Camera 06, frame 000000: the NaN plan and the empty mask; "kp2d" plans before it looks at the mask."""
    want = raised(broken_root, "kp2d", ["06", "07"], ["000000"])
    assert want == (ValueError, "a keypoint of a drawn link is not finite") == raised(broken_root, "kp3d", ["06", "07"], ["000000"])


def test_kp3d_missing_pose_file(broken_root, host_ops):
    (broken_root / ks.SCENE / "poses_3d" / "000001.json").unlink()
    cls, text = raised(broken_root, "kp3d", ["03", "04"], ["000001"])
    assert cls is FileNotFoundError and "poses_3d/000001.json" in text
