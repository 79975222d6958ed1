"""CPU: the nerfstudio export (host/nerfstudio.py) and its wiring.  The camera files, the copied point cloud and the arguments that reach
``remove_background`` on a small result directory built from tests/golden/capture_scene; the refusal of a hub-style network name before
anything is written; ``inference.py``'s ``to_nerfstudio`` step with a fake runner; the runner's arguments.  The matting stage itself
runs on the device: tests/test_nerfstudio_gpu.py."""
import json
import shutil
import types
from pathlib import Path

import numpy as np
import pytest
from PIL import Image

from diffuman4d_amd.host import matting, nerfstudio

SCENE = Path(__file__).resolve().parent / "golden" / "capture_scene" / "ring8"


def make_dirs(tmp_path):
    data, res = tmp_path / "data" / "ring8", tmp_path / "res"
    data.mkdir(parents=True)
    shutil.copy(SCENE / "transforms.json", data / "transforms.json")
    (data / "sparse_pcd.ply").write_bytes(b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nend_header\n0\n")
    for cam in ("00", "03"):
        (res / "images" / cam).mkdir(parents=True)
        Image.fromarray(np.full((20, 16, 3), 200, np.uint8)).save(res / "images" / cam / "000000.jpg")
    return str(data), str(res)


def test_export_writes_cameras_and_point_cloud_and_calls_the_matting_stage(tmp_path, monkeypatch):
    data, res = make_dirs(tmp_path)
    seen = {}
    monkeypatch.setattr(nerfstudio, "remove_background", lambda **kw: seen.update(kw) or {"images": 2, "written": 2, "skipped": 0})
    model = lambda x: x[:, :1]
    out = nerfstudio.diffuman4d_to_nerfstudio(data, res, ["00", "03"], matting_model=model, device_png=True, batch_size=3)
    assert out == {"images": 2, "written": 2, "skipped": 0}
    assert seen == dict(images_dir=f"{res}/images", out_fmasks_dir=f"{res}/fmasks", out_images_alpha_dir=f"{res}/images_alpha", model_name=None,
                        image_ext=".jpg", mask_ext=".png", rotate_clockwise=0, batch_size=3, skip_exists=False, gpu_ids=None,
                        matting_model=model, device_png=True)
    src = json.loads((SCENE / "transforms.json").read_text())
    cams = json.loads(Path(res, "transforms.json").read_text())
    assert [f["file_path"] for f in cams["frames"]] == [f"images_alpha/{f['camera_label']}/000000.png" for f in src["frames"]]
    assert {k: v for k, v in cams.items() if k != "frames"} == {k: v for k, v in src.items() if k != "frames"}
    inputs = json.loads(Path(res, "transforms_input.json").read_text())
    assert [f["camera_label"] for f in inputs["frames"]] == ["00", "03"]
    assert all(f in cams["frames"] for f in inputs["frames"])
    assert Path(res, "sparse_pcd.ply").read_bytes() == Path(data, "sparse_pcd.ply").read_bytes()


def test_defaults_and_no_input_cameras(tmp_path, monkeypatch):
    data, res = make_dirs(tmp_path)
    seen = {}
    monkeypatch.setattr(nerfstudio, "remove_background", lambda **kw: seen.update(kw) or {})
    nerfstudio.diffuman4d_to_nerfstudio(data, res, matting_model_dir=str(tmp_path))  # an existing directory
    assert seen["batch_size"] == 4 and seen["device_png"] is False and seen["model_name"] == str(tmp_path) and seen["matting_model"] is None
    assert Path(res, "transforms.json").exists() and Path(res, "sparse_pcd.ply").exists()
    assert not Path(res, "transforms_input.json").exists()  # the reference raises NameError here


def test_hub_style_name_is_refused_before_anything_is_written(tmp_path):
    data, res = make_dirs(tmp_path)
    with pytest.raises(FileNotFoundError, match="never downloaded"):
        nerfstudio.diffuman4d_to_nerfstudio(data, res, ["00"], matting_model_dir="ZhengPeng7/BiRefNet")
    with pytest.raises(ValueError, match="matting"):
        nerfstudio.diffuman4d_to_nerfstudio(data, res, ["00"])
    assert sorted(p.name for p in Path(res).iterdir()) == ["images"]


def test_device_png_needs_png_masks(tmp_path):
    with pytest.raises(ValueError, match="mask_ext"):
        matting.remove_background(str(tmp_path), str(tmp_path / "m"), matting_model=lambda x: x[:, :1], mask_ext=".jpg", device_png=True)


def fake_sampler(out):
    ds = types.SimpleNamespace(data_dir="/data", scene_label="0023_06")
    return types.SimpleNamespace(dataset=ds, output_dir=out, input_spa_labels=["01", "13"], pipelines=[None])


def test_runner_passes_the_references_arguments(monkeypatch):
    from diffuman4d_amd.host import runner
    seen = {}
    monkeypatch.setattr(nerfstudio, "diffuman4d_to_nerfstudio", lambda **kw: seen.update(kw) or {"written": 0})
    assert runner.SamplingRunner(fake_sampler("/out")).to_nerfstudio(matting_model_dir="/ckpt", device_png=True) == {"written": 0}
    assert seen == dict(data_dir="/data/0023_06", result_dir="/out", input_cameras=["01", "13"], matting_model_dir="/ckpt", device_png=True)

    class Dist:
        barriers = 0

        def barrier(self, group):
            Dist.barriers += 1

    for rank, want in ((0, {"written": 0}), (1, None)):
        r = object.__new__(runner.DistributedSamplingRunner)
        r.sampler, r.dist, r.group, r.rank = fake_sampler("/out"), Dist(), None, rank
        seen.clear()
        Dist.barriers = 0
        assert r.to_nerfstudio(matting_model_dir="/ckpt") == want
        assert Dist.barriers == 2 and bool(seen) == (rank == 0)


def test_cli_to_nerfstudio_reaches_the_runner(monkeypatch, caplog, tmp_path):
    import inference
    from diffuman4d_amd.host import config as cfglib
    from diffuman4d_amd.host import runner
    calls = []

    class FakeRunner:
        def __init__(self, sampler, **kw):
            pass

        def inference(self):
            calls.append("inference")

        def to_nerfstudio(self, **kw):
            calls.append(("to_nerfstudio", kw))

    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(runner, "SamplingRunner", FakeRunner)
    monkeypatch.setattr(inference.cfglib, "instantiate", lambda node, **kw: types.SimpleNamespace(output_dir="/nowhere"))
    cfg = cfglib.compose(["exp=demo_4d_tiny", "model=diffuman4d_mi355x", "to_nerfstudio=true", f"nerfstudio.matting_model_dir={tmp_path}"])
    assert cfg["to_nerfstudio"] is True and cfg["nerfstudio"] == {"matting_model_dir": str(tmp_path)}
    inference.inference(cfg)
    assert calls == ["inference", ("to_nerfstudio", {"matting_model_dir": str(tmp_path), "device_png": False})]
    del calls[:]
    cfg = cfglib.compose(["exp=demo_4d_tiny", "model=diffuman4d_mi355x", f"nerfstudio.matting_model_dir={tmp_path}", "nerfstudio.device_png=true",
                          "nerfstudio.batch_size=2"])
    inference.inference(cfg)  # to_nerfstudio defaults to true
    assert calls == ["inference", ("to_nerfstudio", {"matting_model_dir": str(tmp_path), "device_png": True, "batch_size": 2})]
    del calls[:]
    with caplog.at_level("WARNING"):
        inference.inference(cfglib.compose(["exp=demo_4d_tiny", "model=diffuman4d_mi355x"]))
    assert calls == ["inference"]
    assert any("to_nerfstudio" in r.message and "out of scope" in r.message and "nerfstudio.matting_model_dir" in r.message
               for r in caplog.records)
