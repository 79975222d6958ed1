"""CPU: the evaluator's test-side model checks itself; evaluate_results, the runners' evaluate() and the CLI switch run with the model in
place of the kernel wrapper (the stand-in pattern of test_capture_gpu.py::_HostTensors); without it a host tensor is refused."""
import json
import math
import os
import types
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F
from PIL import Image

import eval_model as em
from diffuman4d_amd.host import lib as L, metrics

SCENE = Path(__file__).resolve().parent / "golden" / "capture_scene" / "ring8"
CAMS, FRAMES = ["00", "03", "06"], ["000000", "000001", "000002"]


# -- the model's self-checks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_model_identical_images(dtype):
    a = torch.rand(3, 40, 50, generator=torch.Generator().manual_seed(0))
    psnr, ssim, box = em.evaluate(a, a, canvas_size=50, crop_with_fmask=False, dtype=dtype)
    assert psnr == float("inf") and ssim == pytest.approx(1.0, abs=1e-6 if dtype == torch.float32 else 1e-12) and box == (0, 0, 50, 40)


@pytest.mark.parametrize("a,d", [(0.3, 0.2), (0.0, 1.0), (0.9, 0.05)])
def test_model_constant_images(a, d):
    c1 = 1e-4
    p, t = torch.full((3, 30, 34), a, dtype=torch.float64), torch.full((3, 30, 34), a + d, dtype=torch.float64)
    _, ssim, _ = em.evaluate(p, t, canvas_size=34, crop_with_fmask=False, dtype=torch.float64)
    # constant images have no variance: the structure term is c2 / c2 and the luminance term is left.  In floating point each of the
    # three E[xy] - mu_x mu_y is a rounding residue of 121-term sums of values <= 1, at most 121 * 2^-53 each; four of them against
    # c2 = 9e-4 move the ratio by at most 4 * 121 * 2^-53 / 9e-4 = 6e-11
    assert ssim == pytest.approx((2 * a * (a + d) + c1) / (a * a + (a + d) ** 2 + c1), abs=6e-11)
    assert em.evaluate(p, t, canvas_size=34, crop_with_fmask=False)[0] == pytest.approx(10 * math.log10(1 / d ** 2), abs=1e-9)


@pytest.mark.parametrize("w,h,size", [(2448, 2048, (1024, 1224)), (200, 160, (1024, 1280)), (1000, 750, (1024, 1365))])
def test_model_nearest_resize_sizes_and_indices(w, h, size):
    assert metrics.resized_size(h, w, 1024) == size
    for n_in, n_out in ((h, size[0]), (w, size[1])):
        ramp = torch.arange(n_in, dtype=torch.float32)[None, None, None]
        assert F.interpolate(ramp, size=(1, n_out), mode="nearest")[0, 0, 0].long().tolist() == em.nearest_index(n_out, n_in)
    assert em.nearest_index(37, 37) == list(range(37)) and em.nearest_index(74, 37) == [d >> 1 for d in range(74)]


def test_resize_compares_the_canvas_with_the_width_only():
    assert metrics.resized_size(800, 1024, 1024) == (800, 1024)    # the width is the canvas: nothing is resized, although h < w
    assert metrics.resized_size(1024, 800, 1024) == (1310, 1024)   # the short edge becomes the canvas
    assert metrics.resized_size(1024, 2048, 1024) == (1024, 2048)  # resized to its own size


# -- evaluate_results over a directory, the model as the kernel wrapper -----------------------------------------------------------------
def make_results(root: Path, cams=CAMS, frames=FRAMES) -> str:
    """A result directory for the golden scene: every target view = the captured one shifted by a pixel, as JPEG quality 90."""
    for cam in cams:
        (root / "images" / cam).mkdir(parents=True)
        for fr in frames:
            gt = np.asarray(Image.open(SCENE / "images" / cam / f"{fr}.webp"))
            Image.fromarray(np.roll(gt, 1, axis=1)).save(root / "images" / cam / f"{fr}.jpg", quality=90)
    return str(root)


@pytest.fixture
def standin(monkeypatch):
    monkeypatch.setattr(metrics.ops, "eval_psnr_ssim", em.standin_eval_psnr_ssim)


def _evaluate(out, **kw):
    args = dict(pred_images_dir=f"{out}/images", gt_images_dir=str(SCENE / "images"), fmasks_dir=str(SCENE / "fmasks"), pred_image_ext=".jpg",
                gt_image_ext=".webp", fmask_ext=".png", background_color="white", gpu_ids=["cpu"])
    args.update(kw)
    return metrics.evaluate_results(**args)


def test_evaluate_results_schema_order_and_means(tmp_path, standin, caplog):
    out = make_results(tmp_path / "res")
    path = tmp_path / "res" / "sub" / "metrics.json"
    with caplog.at_level("INFO"):
        m = _evaluate(out, out_metrics_path=str(path), batch_size=4)  # spa / tem labels from the directory listings
    assert sum("LPIPS is not built" in r.message for r in caplog.records) == 1
    assert json.loads(path.read_text()) == m and path.read_text().startswith("{\n    \"mean\"")
    assert list(m) == ["mean", "values"] and list(m["mean"]) == ["psnr", "ssim", "lpips"]
    assert [v["key"] for v in m["values"]] == [f"{c}/{f}" for c in CAMS for f in FRAMES]
    for v in m["values"]:
        assert list(v) == ["key", "psnr", "ssim", "lpips"] and v["lpips"] is None
        cam, fr = v["key"].split("/")
        fm = np.asarray(Image.open(SCENE / "fmasks" / cam / f"{fr}.png"))
        p, s, _ = em.evaluate(np.asarray(Image.open(f"{out}/images/{v['key']}.jpg")), np.asarray(Image.open(SCENE / "images" / cam / f"{fr}.webp")),
                              fm, fm, 1024, True, "white", torch.float32)
        assert (v["psnr"], v["ssim"]) == (p, s) and 15 < p < 60 and 0.3 < s < 1
    assert m["mean"]["lpips"] is None
    for k in ("psnr", "ssim"):
        assert m["mean"][k] == round(torch.tensor([v[k] for v in m["values"]]).mean().item(), 3) == round(m["mean"][k], 3)
    # explicit labels in the caller's order; two workers over keys[i::2]; the same values
    m2 = _evaluate(out, spa_labels=["03", "00"], tem_labels=["000002", "000001"], gpu_ids=["cpu", "cpu"], batch_size=1)
    assert [v["key"] for v in m2["values"]] == ["00/000001", "00/000002", "03/000001", "03/000002"]
    by_key = {v["key"]: v for v in m["values"]}
    assert all(v == by_key[v["key"]] for v in m2["values"])


def test_lpips_callable_fills_the_values(tmp_path, standin):
    out = make_results(tmp_path / "res", ["00"], ["000001"])
    m = _evaluate(out, lpips=lambda gt, pred: (gt - pred).abs().mean())
    assert m["values"][0]["lpips"] == pytest.approx(m["mean"]["lpips"], abs=1e-3) and m["mean"]["lpips"] > 0


def test_the_references_error_texts(tmp_path, standin):
    ev = metrics.ImageEvaluator("cpu")
    img, small = torch.rand(3, 40, 48), torch.rand(3, 40, 40)
    mask = torch.zeros(1, 40, 48)
    mask[0, 10:30, 10:30] = 1
    with pytest.raises(ValueError, match="The GT and predicted images should have the same shape."):
        ev(img, small, mask, mask, canvas_size=48)
    with pytest.raises(ValueError, match=r"shape mismatch: torch.Size\(\[3, 40, 48\]\) != torch.Size\(\[1, 40, 40\]\)"):
        ev(img, img, small[:1], None, canvas_size=48)
    with pytest.raises(ValueError, match=r"shape mismatch: torch.Size\(\[3, 40, 48\]\) != torch.Size\(\[1, 20, 48\]\)"):
        ev(img, img, mask, mask[:, :20], canvas_size=48)
    with pytest.raises(ValueError, match="Invalid background color: blue"):
        ev(img, img, mask, mask, canvas_size=48, background_color="blue")
    with pytest.raises(ValueError, match="Either pred_fmask or gt_fmask should be provided to crop with fmask."):
        ev(img, img, canvas_size=48)
    tiny = torch.zeros(1, 40, 48)
    tiny[0, 20, 20] = 1  # a 17 x 17 box: 289 >= 0.02 * 3 * 40 * 48 = 115.2 passes
    big_img, big_tiny = torch.rand(3, 200, 240), torch.zeros(1, 200, 240)
    big_tiny[0, 100, 100] = 1  # 17 x 17 = 289 < 0.02 * 3 * 200 * 240 = 2880
    with pytest.raises(ValueError, match="The cropped region is too small. Please check your data."):
        ev(big_img, big_img, big_tiny, big_tiny, canvas_size=240)
    with pytest.raises(ValueError, match="The cropped region is too small. Please check your data."):
        ev(big_img, big_img, torch.zeros(1, 200, 240), None, canvas_size=240)  # an empty mask
    assert ev(img, img, tiny, tiny, canvas_size=48)[0] == float("inf")
    with pytest.raises(ValueError, match="The GT image should be normalized."):
        ev(img, img * 2, canvas_size=48, crop_with_fmask=False)
    with pytest.raises(ValueError, match="The predicted image should be normalized."):
        ev(img - 0.5, img, canvas_size=48, crop_with_fmask=False)
    with pytest.raises(ValueError, match="too small for the 11 x 11 SSIM window"):
        ev(img[:, :10], img[:, :10], canvas_size=48, crop_with_fmask=False)
    # a file whose mode would need a conversion
    Image.fromarray(np.zeros((40, 48, 3), np.uint8)).save(tmp_path / "rgb_mask.png")
    with pytest.raises(ValueError, match="image mode 'RGB', expected 'L'"):
        ev(img, img, str(tmp_path / "rgb_mask.png"), None, canvas_size=48)


def test_there_is_no_cpu_path():
    a = torch.rand(3, 32, 32)
    with pytest.raises(L.Dm4dError, match="HIP device"):
        metrics.ImageEvaluator("cpu")(a, a, canvas_size=32, crop_with_fmask=False)


# -- wiring -------------------------------------------------------------------------------------------------------------------------
def fake_sampler(out: str):
    ds = types.SimpleNamespace(data_dir=str(SCENE.parent), scene_label=SCENE.name)
    return types.SimpleNamespace(dataset=ds, output_dir=out, target_spa_labels=CAMS, tem_labels=FRAMES[:2], pipelines=[None])


def test_runner_evaluate_passes_the_references_arguments(tmp_path, standin, monkeypatch):
    from diffuman4d_amd.host import runner
    out = make_results(tmp_path / "res")
    seen = {}
    real = metrics.evaluate_results
    monkeypatch.setattr(metrics, "evaluate_results", lambda **kw: seen.update(kw) or real(**kw))
    m = runner.SamplingRunner(fake_sampler(out)).evaluate(gpu_ids=["cpu"])
    scene = f"{SCENE.parent}/{SCENE.name}"
    assert seen == dict(pred_images_dir=f"{out}/images", gt_images_dir=f"{scene}/images", fmasks_dir=f"{scene}/fmasks", pred_image_ext=".jpg",
                        gt_image_ext=".webp", fmask_ext=".png", spa_labels=CAMS, tem_labels=FRAMES[:2],
                        out_metrics_path=f"{out}/metrics.json", crop_with_fmask=True, background_color="white", gpu_ids=["cpu"])
    assert json.loads(Path(out, "metrics.json").read_text()) == m and len(m["values"]) == 6


def test_cli_evaluating_reaches_the_runner(monkeypatch, caplog):
    import inference
    from diffuman4d_amd.host import runner
    calls = []

    class FakeRunner:
        def __init__(self, sampler, **kw):
            calls.append("init")

        def inference(self):
            calls.append("inference")

        def evaluate(self):
            calls.append("evaluate")
            return {"mean": {"psnr": 1.0, "ssim": 1.0, "lpips": None}, "values": []}

    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(runner, "SamplingRunner", FakeRunner)
    monkeypatch.setattr(inference.cfglib, "instantiate", lambda node, **kw: types.SimpleNamespace(output_dir="/nowhere"))
    cfg = {"data": {"_target_": "d"}, "model": {"_target_": "m"}, "sampler": {"_target_": "s"}, "sampling": True}
    inference.inference(dict(cfg, evaluating=False, to_nerfstudio=False))
    assert calls == ["init", "inference"]
    del calls[:]
    with caplog.at_level("WARNING"):
        inference.inference(dict(cfg, evaluating=True, to_nerfstudio=True))
    assert calls == ["init", "inference", "evaluate"]
    assert any("to_nerfstudio" in r.message and "out of scope" in r.message for r in caplog.records)  # still not built: still said


def _eval_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from diffuman4d_amd.host import runner
        metrics.ops.eval_psnr_ssim = em.standin_eval_psnr_ssim
        seen = []
        real = metrics.evaluate_keys
        metrics.evaluate_keys = lambda keys, device, **kw: seen.extend(keys) or real(keys, device, **kw)
        m = runner.DistributedSamplingRunner(fake_sampler(out)).evaluate()
        assert (m is not None) == (rank == 0)
        Path(out, f"keys{rank}.json").write_text(json.dumps(seen))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_distributed_evaluate_equals_one_process(tmp_path, standin):
    from diffuman4d_amd.host import runner
    one, two = make_results(tmp_path / "one"), make_results(tmp_path / "two")
    runner.SamplingRunner(fake_sampler(one)).evaluate(gpu_ids=["cpu"])
    mp.spawn(_eval_worker, args=(2, 29500 + (os.getpid() % 2000) + 7, two), nprocs=2, join=True)
    assert Path(two, "metrics.json").read_text() == Path(one, "metrics.json").read_text()
    keys = [f"{c}/{f}" for c in CAMS for f in FRAMES[:2]]
    assert [json.loads(Path(two, f"keys{r}.json").read_text()) for r in range(2)] == [keys[0::2], keys[1::2]]


# -- ABI: descriptor errors before the device is touched ----------------------------------------------------------------------------------
def test_eval_entry_rejects_bad_descriptors():
    lib = L.load()
    f = lib.dm4d_eval_psnr_ssim_f64
    last = lambda: lib.dm4d_last_error().decode()
    P, h, w = 0x10000, 32, 48  # P: a non-null "device" address that is never read -- every call below fails its host-side check first
    blob_bytes = h * w * 7
    good = [0, h * w * 3, h * w * 6, -1, h, w, h, w, metrics.ops.EVAL_CROP_MASKS | (1 << metrics.ops.EVAL_BG_SHIFT), 0, 0, w, h, 0, 0, 0]

    def call(desc=None, blob=P, n=1, ws_bytes=1 << 20, dbg=None, dbg_h=0, dbg_w=0, **fields):
        d = list(good)
        for k, v in fields.items():
            d[int(k[1:])] = v
        d = np.array([d], np.int64)
        return f(None, blob, blob_bytes, d.ctypes.data, P, n, P, ws_bytes, P, P, dbg, dbg_h, dbg_w)

    assert call(blob=None) == -1 and "null pointer" in last()
    assert call(n=0) == -1 and "batch" in last()
    assert call(blob=P + 4) == -1 and "aligned" in last()
    for fields, text in [(dict(f1=h * w * 5), "image lies outside"), (dict(f0=-4), "image lies outside"), (dict(f2=h * w * 6 + 1), "mask lies outside"),
                         (dict(f4=0), "bad source or resized size"), (dict(f5=-w), "bad source or resized size"), (dict(f4=2 * h), "image lies outside"),
                         (dict(f6=0), "bad source or resized size"), (dict(f7=1 << 20), "bad source or resized size"),
                         (dict(f8=3 << metrics.ops.EVAL_BG_SHIFT), "bad flags"), (dict(f8=1 << 8), "bad flags"), (dict(f2=-1), "without a mask"),
                         (dict(f8=metrics.ops.EVAL_IMAGE_F32, f0=2, f4=4, f5=4, f6=4, f7=4, f11=4, f12=4), "misaligned"),
                         (dict(f8=0, f11=w + 1), "crop box"), (dict(f8=0, f9=10, f11=10), "crop box"), (dict(f8=0, f10=-1), "crop box")]:
        assert call(**fields) == -1 and text in last(), (fields, last())
    assert call(ws_bytes=64) == -1 and "workspace too small" in last()
    assert call(dbg=P, dbg_h=h - 1, dbg_w=w) == -1 and "debug planes" in last()
    assert lib.dm4d_eval_ws_bytes(1, h, w) == 16 + 2 * 2 * 6 * 8 and lib.dm4d_eval_ws_bytes(0, h, w) == 0
