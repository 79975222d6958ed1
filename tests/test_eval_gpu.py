"""GPU: dm4d_eval_psnr_ssim_f64 and the evaluator built on it against the test-side model (tests/eval_model.py): bounding boxes and
composites exactly, PSNR / SSIM within the float32 model's own distance from the float64 model, reproducibility, descriptor checks,
and the CLI with evaluating=true on the golden scene.

The PSNR / SSIM bound is not a constant: the test measures the float32 model's distance from the float64 model on its own case set and
allows the native results twice that (a different summation order produces rounding error of the same size).  It prints both maxima."""
import io
import json
import math
import os
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image

import eval_model as em
from diffuman4d_amd.host import lib as L, metrics, ops

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
SCENE_DIR = GOLDEN / "capture_scene"
SCENE = "ring8"
DEV = torch.device("cuda", 0)


def _jpeg(a: np.ndarray, quality: int = 90) -> np.ndarray:
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, format="JPEG", quality=quality)
    return np.asarray(Image.open(io.BytesIO(buf.getvalue())))


def _ring8(cam: str, canvas: int, bg: str = "white"):
    gt = np.asarray(Image.open(SCENE_DIR / SCENE / "images" / cam / "000001.webp"))
    mask = np.asarray(Image.open(SCENE_DIR / SCENE / "fmasks" / cam / "000001.png"))
    pred = _jpeg(np.roll(gt, 1, axis=1))  # the ground truth shifted by one pixel, through JPEG quality 90
    return dict(pred=pred, gt=gt, pred_fmask=mask, gt_fmask=mask, canvas_size=canvas, crop_with_fmask=True, background_color=bg)


def _soft_mask(rng, h, w):
    m = rng.integers(0, 256, (h, w), dtype=np.uint8)
    m[rng.random((h, w)) < 0.3] = 0
    return m


def _noisy(rng, a, amp=24):
    return np.clip(a.astype(np.int32) + rng.integers(-amp, amp + 1, a.shape), 0, 255).astype(np.uint8)


def case_set():
    """(name, evaluator keywords).  Arrays stand for decoded files (uint8 HWC), tensors for the API path (fp32 CHW)."""
    rng = np.random.default_rng(7)
    cases = [(f"ring8_{cam}_canvas{c}", _ring8(cam, c)) for cam in ("00", "03") for c in (1024, 100, 160)]
    cases += [(f"ring8_00_{bg}", _ring8("00", 100, bg)) for bg in ("black", "grey")]
    # random images at capture size with a soft mask (the worst case for rounding)
    gt = rng.integers(0, 256, (2048, 2448, 3), dtype=np.uint8)
    m = _soft_mask(rng, 2048, 2448)
    cases.append(("random_2448x2048", dict(pred=_noisy(rng, gt), gt=gt, pred_fmask=m, gt_fmask=m, canvas_size=1024,
                                           crop_with_fmask=True, background_color="white")))
    # a mask touching two image edges (the top-left corner), two different masks
    gt = rng.integers(0, 256, (200, 160, 3), dtype=np.uint8)
    m1, m2 = np.zeros((200, 160), np.uint8), np.zeros((200, 160), np.uint8)
    m1[:120, :100], m2[10:150, :80] = 255, 200
    cases.append(("mask_on_two_edges", dict(pred=_noisy(rng, gt), gt=gt, pred_fmask=m1, gt_fmask=m2, canvas_size=100,
                                            crop_with_fmask=True, background_color="white")))
    # the smallest crops the SSIM window fits into: 11 x 11 and 12 x 400 (fp32 tensors, nothing cropped, canvas == width)
    for h, w in ((11, 11), (12, 400)):
        a = torch.from_numpy(rng.random((3, h, w), dtype=np.float32))
        b = (a + torch.from_numpy(rng.normal(0, 0.05, (3, h, w)).astype(np.float32))).clamp(0, 1)
        cases.append((f"crop_{h}x{w}", dict(pred=b, gt=a, canvas_size=w, crop_with_fmask=False)))
    # fp32 tensors with fp32 masks, up-scaled by 2 (90 x 70 -> 180 x 140)
    a = torch.from_numpy(rng.random((3, 90, 70), dtype=np.float32))
    b = (a + torch.from_numpy(rng.normal(0, 0.1, (3, 90, 70)).astype(np.float32))).clamp(0, 1)
    fm = torch.zeros(1, 90, 70)
    fm[0, 20:70, 15:60] = torch.from_numpy(rng.random((50, 45), dtype=np.float32))
    cases.append(("fp32_tensors", dict(pred=b, gt=a, pred_fmask=fm, gt_fmask=fm, canvas_size=140, crop_with_fmask=True,
                                       background_color="grey")))
    # no mask, nothing cropped, up-scaled (300 x 240 -> 1280 x 1024)
    gt = rng.integers(0, 256, (300, 240, 3), dtype=np.uint8)
    cases.append(("no_mask", dict(pred=_noisy(rng, gt, 8), gt=gt, canvas_size=1024, crop_with_fmask=False)))
    # one mask only, black background
    gt = rng.integers(0, 256, (150, 210, 3), dtype=np.uint8)
    m = np.zeros((150, 210), np.uint8)
    m[30:120, 50:170] = rng.integers(1, 256, (90, 120), dtype=np.uint8)
    cases.append(("gt_mask_only_black", dict(pred=_noisy(rng, gt), gt=gt, gt_fmask=m, canvas_size=128, crop_with_fmask=True,
                                             background_color="black")))
    return cases


def _native(cases, debug=False):
    ev = metrics.ImageEvaluator(DEV)
    items = [ev._prepare(**kw) for _, kw in cases]
    out, boxes, dbg = ev._run(items, debug=debug)
    return out, boxes, (None if dbg is None else dbg.cpu())


def test_boxes_and_composites_equal_the_model():
    cases = case_set()
    out, boxes, dbg = _native(cases, debug=True)
    for i, (name, kw) in enumerate(cases):
        p, g, box = em.composites(dtype=torch.float32, **kw)
        assert tuple(int(v) for v in boxes[i]) == tuple(box), f"{name}: box {boxes[i].tolist()} != {box}"
        l, t, r, b = box
        assert torch.equal(dbg[i, 0, :, : b - t, : r - l], p), f"{name}: predicted composite differs"
        assert torch.equal(dbg[i, 1, :, : b - t, : r - l], g), f"{name}: ground-truth composite differs"
        assert float(out[i, 2]) == float(p.min()) and float(out[i, 3]) == float(p.max()), name
        assert float(out[i, 4]) == float(g.min()) and float(out[i, 5]) == float(g.max()), name


def test_psnr_and_ssim_within_the_float32_models_own_error(tmp_path):
    cases = case_set()
    out, _, _ = _native(cases)
    rows, model_err, native_err = [], [0.0, 0.0], [0.0, 0.0]
    for i, (name, kw) in enumerate(cases):
        p64, s64, _ = em.evaluate(dtype=torch.float64, **kw)
        p32, s32, _ = em.evaluate(dtype=torch.float32, **kw)
        pn, sn = float(out[i, 0]), float(out[i, 1])
        assert math.isfinite(pn) and math.isfinite(sn), name
        e = (abs(p32 - p64), abs(s32 - s64), abs(pn - p64), abs(sn - s64))
        rows.append(f"{name:24s} psnr {p64:10.6f} dB  ssim {s64:.8f}   fp32 model: {e[0]:.2e} dB {e[1]:.2e}   native: {e[2]:.2e} dB {e[3]:.2e}")
        model_err = [max(model_err[0], e[0]), max(model_err[1], e[1])]
        native_err = [max(native_err[0], e[2]), max(native_err[1], e[3])]
    rows.append(f"largest |fp32 model - fp64 model|: psnr {model_err[0]:.3e} dB, ssim {model_err[1]:.3e}")
    rows.append(f"largest |native - fp64 model|:     psnr {native_err[0]:.3e} dB, ssim {native_err[1]:.3e}   (bound: 2 x the line above)")
    report = "\n".join(rows)
    print("\n" + report)
    (tmp_path / "eval_parity.log").write_text(report + "\n")
    if os.environ.get("DM4D_EVAL_PARITY_LOG"):
        Path(os.environ["DM4D_EVAL_PARITY_LOG"]).write_text(report + "\n")
    assert native_err[0] <= 2 * model_err[0], f"psnr: native {native_err[0]:.3e} dB > 2 x {model_err[0]:.3e} dB"
    assert native_err[1] <= 2 * model_err[1], f"ssim: native {native_err[1]:.3e} > 2 x {model_err[1]:.3e}"


def test_identical_images_give_inf_and_one():
    kw = _ring8("00", 100)
    kw["pred"] = kw["gt"]
    psnr, ssim, lp = metrics.ImageEvaluator(DEV)(**kw)
    assert psnr == float("inf") and ssim == pytest.approx(1.0, abs=1e-12) and lp is None


def test_a_pair_does_not_depend_on_its_batch_or_the_run():
    cases = case_set()
    pick = [c for c in cases if c[0] in ("ring8_00_canvas1024", "mask_on_two_edges", "crop_11x11", "crop_12x400", "no_mask",
                                         "ring8_03_canvas100", "gt_mask_only_black")]
    assert len(pick) == 7
    batch, _, _ = _native(pick)
    again, _, _ = _native(pick)
    assert batch.numpy().tobytes() == again.numpy().tobytes()
    for i, c in enumerate(pick):
        alone, _, _ = _native([c])
        assert alone[0].numpy().tobytes() == batch[i].numpy().tobytes(), f"{c[0]}: alone != in a batch of 7"
    rev, _, _ = _native(pick[::-1])
    assert rev.flip(0).numpy().tobytes() == batch.numpy().tobytes()


def test_lpips_callable_receives_the_cropped_composites():
    kw = _ring8("00", 100)
    p, g, _ = em.composites(dtype=torch.float32, **kw)
    seen = {}

    def fake_lpips(gt, pred):
        seen["gt"], seen["pred"] = gt.cpu(), pred.cpu()
        return torch.tensor(0.25)
    ev = metrics.ImageEvaluator(DEV, lpips=fake_lpips)
    _, _, lp = ev(**kw)
    assert lp == 0.25 and torch.equal(seen["gt"][0], g) and torch.equal(seen["pred"][0], p)


def test_bad_descriptors_are_refused_before_any_launch():
    """Host-side checks only: every call below must come back with an error code from the descriptor validation."""
    h, w = 32, 48
    blob = torch.zeros(h * w * 3 * 2 + h * w, dtype=torch.uint8, device=DEV)
    good = [0, h * w * 3, h * w * 6, -1, h, w, h, w, ops.EVAL_CROP_MASKS | (1 << ops.EVAL_BG_SHIFT), 0, 0, w, h, 0, 0, 0]
    out, boxes = ops.eval_psnr_ssim(blob, torch.tensor([good], dtype=torch.int64))
    assert tuple(boxes[0].tolist()) == (0, 0, 0, 0) and math.isnan(float(out[0, 0]))  # an all-zero mask: the empty box, no fault

    def bad(**changes):
        d = list(good)
        for k, v in changes.items():
            d[int(k[1:])] = v
        return torch.tensor([d], dtype=torch.int64)

    for name, desc in [("image outside the blob", bad(f1=h * w * 5)), ("negative offset", bad(f0=-4)),
                       ("mask outside the blob", bad(f2=h * w * 6 + 1)), ("zero height", bad(f4=0)), ("negative width", bad(f5=-w)),
                       ("source larger than the blob", bad(f4=h * 2)), ("zero resized size", bad(f6=0)),
                       ("oversized resized size", bad(f7=1 << 20)), ("bad background", bad(f8=3 << ops.EVAL_BG_SHIFT)),
                       ("unknown flag", bad(f8=1 << 8)), ("crop by masks without a mask", bad(f2=-1)),
                       ("misaligned fp32 image", bad(f8=ops.EVAL_IMAGE_F32, f0=2, f9=0, f10=0, f11=4, f12=4, f4=4, f5=4, f6=4, f7=4)),
                       ("box leaves the image", bad(f8=0, f11=w + 1)), ("empty box", bad(f8=0, f9=10, f11=10)),
                       ("negative box", bad(f8=0, f10=-1))]:
        with pytest.raises(L.Dm4dError, match="eval_psnr_ssim"):
            ops.eval_psnr_ssim(blob, desc)
    with pytest.raises(L.Dm4dError, match="HIP device"):
        ops.eval_psnr_ssim(blob.cpu(), torch.tensor([good], dtype=torch.int64))
    torch.cuda.synchronize()


def test_cli_with_evaluating_on_the_golden_scene(tmp_path):
    import inference
    from test_e2e_gpu import _tiny_cfgs
    from diffuman4d_amd.host.weights import write_synthetic_checkpoint
    ucfg, vcfg = _tiny_cfgs()
    ckpt = write_synthetic_checkpoint(tmp_path / "ckpt", ucfg, vcfg, seed=3)
    result_dir = tmp_path / "res"
    inference.main(["exp=demo_4d_tiny", "model=diffuman4d_mi355x", f"data.data_dir={SCENE_DIR}", f"data.scene_label={SCENE}",
                    f"model.model_dir={ckpt}", "model.gpu_ids=[0]", "data.height=64", "data.width=64", f"result_dir={result_dir}",
                    "sampler.spa_label_range=[0,8,1]", "sampler.tem_label_range=[0,3,1]", "sampler.input_spa_labels=[1,5]",
                    "sampler.window_size=2", "sampler.sliding_stride=1", "evaluating=true", "to_nerfstudio=false"])
    found = list(result_dir.rglob("metrics.json"))
    assert len(found) == 1
    m = json.loads(found[0].read_text())
    out_dir = found[0].parent
    targets = [f"{c:02d}" for c in range(8) if c not in (1, 5)]
    keys = [f"{c}/{f:06d}" for c in targets for f in range(3)]
    assert [v["key"] for v in m["values"]] == keys and set(m["mean"]) == {"psnr", "ssim", "lpips"} and m["mean"]["lpips"] is None
    # the bound of test_psnr_and_ssim_within_the_float32_models_own_error, on this test's own pairs
    model_err, native_err = [0.0, 0.0], [0.0, 0.0]
    for v in m["values"]:
        assert math.isfinite(v["psnr"]) and math.isfinite(v["ssim"]) and v["lpips"] is None
        kw = dict(pred=np.asarray(Image.open(out_dir / "images" / f"{v['key']}.jpg")),
                  gt=np.asarray(Image.open(SCENE_DIR / SCENE / "images" / f"{v['key']}.webp")), canvas_size=1024, crop_with_fmask=True,
                  background_color="white")
        kw["pred_fmask"] = kw["gt_fmask"] = np.asarray(Image.open(SCENE_DIR / SCENE / "fmasks" / f"{v['key']}.png"))
        p64, s64, _ = em.evaluate(dtype=torch.float64, **kw)
        p32, s32, _ = em.evaluate(dtype=torch.float32, **kw)
        model_err = [max(model_err[0], abs(p32 - p64)), max(model_err[1], abs(s32 - s64))]
        native_err = [max(native_err[0], abs(v["psnr"] - p64)), max(native_err[1], abs(v["ssim"] - s64))]
    print(f"\ncli: fp32 model {model_err}, native {native_err}")
    assert native_err[0] <= 2 * model_err[0] and native_err[1] <= 2 * model_err[1]
    mean = lambda k: round(torch.tensor([v[k] for v in m["values"]]).mean().item(), 3)
    assert m["mean"]["psnr"] == mean("psnr") and m["mean"]["ssim"] == mean("ssim")
