"""GPU: dm4d_capture_crop_resize_f32 against Pillow + the reference's epilogue (recomputed here on the host), the captured-scene
dataset against the reference's own results (tests/golden/capture_reference.pt), and the CLI on the golden scene."""
import hashlib
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image

import capture_model as cm
from diffuman4d_amd.host import capture

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
SCENE_DIR = GOLDEN / "capture_scene"
REF = torch.load(GOLDEN / "capture_reference.pt", weights_only=False)
SCENE = REF["scene"]
DEV = torch.device("cuda", 0)


def digest(t) -> str:
    a = t.detach().cpu().contiguous().numpy()
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


def frame(rng, h, w, crop):
    """Random planes (the worst case for rounding) with a soft mask; crop = [top, left, height, width]."""
    mask = rng.integers(0, 256, (h, w), dtype=np.uint8)
    mask[rng.random((h, w)) < 0.3] = 0
    return {"img": rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "mask": mask,
            "skel": rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "crop": list(crop) + [h, w]}


def pillow_expected(fr, H, W):
    """Pillow's crop().resize(BICUBIC) on each plane, then the reference's fp32 epilogue."""
    top, left, ch, cw = fr["crop"][:4]
    box = (left, top, left + cw, top + ch)
    rs = lambda a: np.asarray(Image.fromarray(a).crop(box).resize((W, H), Image.BICUBIC))
    return cm.epilogue(rs(fr["img"]), rs(fr["mask"]), rs(fr["skel"]))


def check(frames, H, W):
    ds = capture.SpaTemDataset.__new__(capture.SpaTemDataset)  # only the device half is exercised here
    ds.height, ds.width = H, W
    from concurrent.futures import ThreadPoolExecutor
    import threading
    ds._pool, ds._tls = ThreadPoolExecutor(4), threading.local()
    pix, skel = ds._resize_on_device(frames, DEV)
    assert pix.device == DEV and pix.shape == (len(frames), 3, H, W) and skel.shape == pix.shape
    pix, skel = pix.cpu(), skel.cpu()
    for i, fr in enumerate(frames):
        p, s = pillow_expected(fr, H, W)
        assert torch.equal(pix[i], p), f"frame {i}: pixel_values differ at {int((pix[i] != p).sum())} values"
        assert torch.equal(skel[i], s), f"frame {i}: skeletons differ at {int((skel[i] != s).sum())} values"
    assert pix.min() >= -1 and pix.max() <= 1 and skel.min() >= -1 and skel.max() <= 1


def test_kernel_equals_pillow_at_capture_size():
    rng = np.random.default_rng(0)
    # 2448 x 2048 sources, ~1400^2 crops (one past the top-left corner, one past the right edge) -> 1024^2
    check([frame(rng, 2048, 2448, (300, 500, 1400, 1401)), frame(rng, 2048, 2448, (-60, -25, 1398, 1398)),
           frame(rng, 2048, 2448, (700, 1300, 1404, 1404))], 1024, 1024)


def test_kernel_equals_pillow_upscaling():
    rng = np.random.default_rng(1)
    check([frame(rng, 300, 240, (40, -30, 200, 200)), frame(rng, 300, 240, (150, 100, 180, 181))], 512, 512)


def test_kernel_mixed_batch_in_one_launch():
    rng = np.random.default_rng(2)
    frames = [frame(rng, 200, 160, (-10, -40, 140, 140)),    # past two edges, down
              frame(rng, 333, 251, (0, 0, 96, 120)),         # height kept: Pillow skips the vertical pass
              frame(rng, 96, 128, (0, 0, 96, 128)),          # no resize at all (identity passes)
              frame(rng, 517, 389, (480, 350, 150, 150)),    # past the bottom-right corner
              frame(rng, 64, 64, (10, 10, 1, 1))]            # a 1-pixel crop
    check(frames, 96, 128)


@pytest.mark.parametrize("plucker", ["host", "cameras"])
@pytest.mark.parametrize("name", sorted(REF["queries"]))
def test_get_item_equals_the_reference(name, plucker):
    q = REF["queries"][name]
    ds = capture.SpaTemDataset(data_dir=str(SCENE_DIR), scene_label=SCENE, plucker=plucker, **q["kw"])
    s = ds.get_item(SCENE, q["spa"], q["tem"], REF["inputs"])
    assert s["pixel_values"].device == DEV and s["skeletons"].device == DEV
    assert s["labels"] == q["labels"] and s["crops"] == q["crops"] and torch.equal(s["Ks"], q["Ks"])
    for k in ("pixel_values", "skeletons"):
        assert torch.equal(s[k][:, :, ::16, ::16].cpu(), q[k + "_thumb"]), k
        assert digest(s[k]) == q[k + "_sha256"], k
        assert float(s[k].min()) >= -1.0 and float(s[k].max()) <= 1.0
    if plucker == "host":
        assert float((s["plucker_embeds"][:, :, ::16, ::16] - q["plucker_embeds_thumb"]).abs().max()) <= 1e-6
    else:
        assert s["plucker_embeds"] is None


class _HostTensors:
    """In-test stand-in: the native dataset with the host model in place of the kernel, tensors left on the host."""

    def __init__(self, ds):
        self.ds, self.scene_label = ds, ds.scene_label

    def get_item(self, *a, **k):
        real = capture.ops.capture_crop_resize
        capture.ops.capture_crop_resize = cm.standin_crop_resize
        try:
            return self.ds.get_item(*a, **k)
        finally:
            capture.ops.capture_crop_resize = real

    def nearest_input_camera(self, *a):
        return self.ds.nearest_input_camera(*a)


def _run(tmp_path, ckpt, tag, device_results, standin):
    from diffuman4d_amd.host import config as cfglib
    from diffuman4d_amd.host.results import check_sampling_results
    from diffuman4d_amd.host.runner import SamplingRunner
    ov = ["exp=demo_4d_tiny", "model=diffuman4d_mi355x", f"data.data_dir={SCENE_DIR}", f"data.scene_label={SCENE}",
          f"model.model_dir={ckpt}", "model.gpu_ids=[0]", "data.height=64", "data.width=64", f"result_dir={tmp_path / tag}",
          "sampler.spa_label_range=[0,8,1]", "sampler.tem_label_range=[0,3,1]", "sampler.input_spa_labels=[1,5]",
          "sampler.window_size=2", "sampler.sliding_stride=1", f"sampler.device_results={str(device_results).lower()}"]
    cfg = cfglib.compose(ov)
    pipelines = cfglib.instantiate(cfg["model"])
    ds = cfglib.instantiate(cfg["data"])
    assert type(ds) is capture.SpaTemDataset  # resolved without the reference checkout
    if standin:
        ds.device = "cpu"
        ds = _HostTensors(ds)
    sampler = cfglib.instantiate(cfg["sampler"], dataset=ds, pipelines=pipelines)
    torch.manual_seed(1234)  # the initial noise comes from the device generator: one GPU stream keeps the draws in task order
    SamplingRunner(sampler, prefetch_depth=0 if standin else 2, writers=2, gpu_streams=1,
                   writer_processes=2 if device_results else 0).inference()
    assert all(sampler.timestep_indices[c][f] == 2 // 1 * 3 for c in sampler.target_spa_labels for f in sampler.tem_labels)
    assert check_sampling_results(sampler.spa_labels, sampler.tem_labels, sampler.output_dir)
    return torch.stack([sampler.latents[c][f].float().cpu() for c in sampler.target_spa_labels for f in sampler.tem_labels])


def test_cli_on_the_golden_scene(tmp_path):
    from test_e2e_gpu import _tiny_cfgs
    from diffuman4d_amd.host.weights import write_synthetic_checkpoint
    ucfg, vcfg = _tiny_cfgs()
    ckpt = write_synthetic_checkpoint(tmp_path / "ckpt", ucfg, vcfg, seed=3)
    ref = _run(tmp_path, ckpt, "standin", False, standin=True)
    assert bool(torch.isfinite(ref).all())
    for device_results in (False, True):
        lat = _run(tmp_path, ckpt, f"native_{device_results}", device_results, standin=False)
        assert torch.equal(lat, ref), f"device_results={device_results}: latents differ from the host-tensor run"
