"""GPU: LpipsVGG (host/lpips.py, csrc/lpips.hip, the MFMA convolution with three-term bf16 products) against the test-side float64 model
(tests/lpips_model.py) with generated full-width weights: the value and the five feature maps, exact zeros / symmetry / reproducibility,
the evaluator and the CLI with LPIPS switched on, and a 1024 x 1024 pair (the reference's canvas; the largest tensors of the path).

Bounds.  Value: |native - fp64 model| <= 5e-5 -- a tenth of the half-unit of the third decimal metrics.json keeps, so the native error
cannot move a rounded mean except at a tie (the fp32 model is within 2e-7 of the fp64 model on these pairs; a CPU emulation of the
three-term rounding within 1.1e-6).  Feature maps: rel-L2 <= 1e-3, the project's north_star bound.

Shapes are the smallest at which each part can still go wrong: 16 x 16 (the last tap is one pixel), 17 x 31 (odd at every pooling, ragged
tiles), 40 x 56, 100 x 64, 96 x 128 (several distance workgroups per tap)."""
import json
import math
import os
from pathlib import Path

import pytest
import torch

import eval_model as em
import lpips_model as lm
from diffuman4d_amd.host import lpips, metrics

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SHAPES = [(16, 16), (17, 31), (40, 56), (100, 64), (96, 128)]
AMPS = [0.02, 0.08, 0.3, 1.0]
VALUE_BOUND = 5e-5
TAP_BOUND = 1e-3


@pytest.fixture(scope="module")
def weights():
    return lm.random_weights(seed=0)


@pytest.fixture(scope="module")
def weight_files(weights, tmp_path_factory):
    return lm.write_checkpoints(tmp_path_factory.mktemp("lpips_weights"), weights)


@pytest.fixture(scope="module")
def lp(weight_files):
    return lpips.LpipsVGG(DEV, *weight_files)


def _dev(t):
    return t.to(DEV)[None]


@pytest.fixture(scope="module")
def parity(lp, weights):
    """Every (shape, amp) pair once: the fp64 model, the native value and feature maps -> rows of (name, model value, |value error|,
    largest feature-map rel-L2)."""
    rows = []
    for h, w in SHAPES:
        for k, amp in enumerate(AMPS):
            a, b = lm.pair(h, w, amp, seed=1000 * h + w + k)
            ref, ref_taps = lm.lpips(a, b, weights, torch.float64)
            val = lp(_dev(a), _dev(b))
            errs = []
            for n, m in zip(lp.taps(_dev(a), _dev(b)), ref_taps):
                assert n.shape == (2,) + tuple(m.shape[2:]) + (m.shape[1],) and n.dtype == torch.float32
                n = n.cpu().double().clamp_min(0).permute(0, 3, 1, 2)
                errs.append(((n - m).norm() / m.norm()).item())
            rows.append((f"{h}x{w}_amp{amp}", ref, abs(val - ref), max(errs), val))
    return rows


def _report(rows):
    lines = [f"{name:18s} lpips {ref:.8f}   native: |value - fp64 model| {ve:.2e}   feature maps rel-L2 <= {te:.2e}" for name, ref, ve, te, _ in rows]
    lines.append(f"largest |native - fp64 model|: {max(r[2] for r in rows):.3e}   (bound {VALUE_BOUND:g})")
    lines.append(f"largest feature-map rel-L2:    {max(r[3] for r in rows):.3e}   (bound {TAP_BOUND:g})")
    return "\n".join(lines)


def test_value_within_a_tenth_of_the_rounding_unit(parity):
    report = _report(parity)
    print("\n" + report)
    if os.environ.get("DM4D_LPIPS_PARITY_LOG"):
        Path(os.environ["DM4D_LPIPS_PARITY_LOG"]).write_text(report + "\n")
    for name, ref, ve, _, val in parity:
        assert math.isfinite(val) and 0.005 <= ref <= 2.0, (name, ref, val)  # the pairs span the range real results have (0.011 .. 1.7)
        assert ve <= VALUE_BOUND, f"{name}: |native - fp64 model| = {ve:.3e} > {VALUE_BOUND:g}"


def test_feature_maps_within_the_north_star_bound(parity):
    print("\n" + _report(parity))
    for name, _, _, te, _ in parity:
        assert te <= TAP_BOUND, f"{name}: feature-map rel-L2 {te:.3e} > {TAP_BOUND:g}"


def test_identical_images_symmetry_and_reruns(lp):
    for h, w in SHAPES:
        a, b = lm.pair(h, w, 0.3, seed=h * w)
        a, b = _dev(a), _dev(b)
        assert lp(a, a) == 0.0 and lp(b, b.clone()) == 0.0
        v = lp(a, b)
        assert v > 0 and lp(b, a) == v and lp(a, b) == v
        d = lp.distances(a, b)
        assert len(d) == 6 and all(x > 0 for x in d[:5]) and d[5] == v == (((d[0] + d[1]) + d[2]) + d[3]) + d[4]


def test_a_pair_does_not_depend_on_its_batch_or_the_run(lp):
    ev = metrics.ImageEvaluator(DEV, lpips=lp)
    pairs, alone = [], []
    for h, w in [(17, 31), (96, 128), (16, 16), (40, 56), (100, 64)]:
        a, b = lm.pair(h, w, 0.08, seed=h + w)
        pairs.append(dict(pred=b, gt=a, canvas_size=w, crop_with_fmask=False))
        alone.append(lp(_dev(a), _dev(b)))  # nothing is composited, resized or cropped: the evaluator hands over the images themselves
    batch = ev.evaluate_batch(pairs)
    assert [r[2] for r in batch] == alone
    assert ev.evaluate_batch(pairs) == batch and ev.evaluate_batch(pairs[::-1]) == batch[::-1]
    for kw, r in zip(pairs, batch):
        assert ev(**kw) == r and metrics.ImageEvaluator(DEV)(**kw) == r[:2] + (None,)  # PSNR / SSIM are what they are without LPIPS


def test_through_the_evaluator_on_the_golden_pair(lp, weights):
    from test_eval_gpu import _ring8
    kw = _ring8("00", 100)
    p, g, _ = em.composites(dtype=torch.float32, **kw)
    ref, _ = lm.lpips(g, p, weights, torch.float64)
    psnr, ssim, val = metrics.ImageEvaluator(DEV, lpips=lp)(**kw)
    print(f"\nring8 canvas 100: crop {tuple(p.shape[1:])}, lpips {ref:.8f}, |native - fp64 model| {abs(val - ref):.2e}")
    assert (psnr, ssim) == metrics.ImageEvaluator(DEV)(**kw)[:2]
    assert abs(val - ref) <= VALUE_BOUND


def test_too_small_crops(lp):
    a, b = lm.pair(12, 400, 0.05, seed=5)
    kw = dict(pred=b, gt=a, canvas_size=400, crop_with_fmask=False)
    with pytest.raises(ValueError, match=r"The cropped region is too small for the five VGG stages of LPIPS: 12 x 400\."):
        metrics.ImageEvaluator(DEV, lpips=lp)(**kw)
    psnr, ssim, val = metrics.ImageEvaluator(DEV)(**kw)
    assert math.isfinite(psnr) and 0 < ssim < 1 and val is None
    a, b = lm.pair(16, 15, 0.05, seed=6)
    with pytest.raises(ValueError, match=r"too small for the five VGG stages of LPIPS: 16 x 15\."):
        lp(_dev(a), _dev(b))


def test_too_large_crops_are_refused_by_name(lp):
    """The convolution entry takes tensors below 2^31 elements: 2 h w 192 operand values.  Above that LpipsVGG raises its own error
    before anything is launched."""
    assert lpips.MAX_PIXELS == 5592405
    big = torch.zeros(1, 3, 2366, 2364, device=DEV)  # 5 593 224 pixels
    with pytest.raises(ValueError, match=r"too large for LPIPS: 2366 x 2364 = 5593224 pixels, at most 5592405"):
        lp(big, big)


def test_1024_pair_at_the_references_canvas(lp):
    """The reference's canvas: the 64-channel stages hold 2 x 1024^2 x 192 operand values (0.8 GB), the largest tensors of the path, and
    the distance kernels run 4096 workgroups per tap.  No CPU model at this size: finite, positive, exact zero, symmetry and reruns.
    This does NOT exercise the 64-bit index paths: no offset passes 2^31 at this size (that takes an edge near 2364, the largest the
    convolution entry accepts, and 4 GiB operands -- too large for a quick test); it checks that the far end of large planes is read."""
    a, b = lm.pair(1024, 1024, 0.08, seed=9)
    a, b = _dev(a), _dev(b)
    v = lp(a, b)
    assert math.isfinite(v) and 0.01 < v < 1.5
    assert lp(a, a) == 0.0
    assert lp(b, a) == v and lp(a, b) == v
    # the far end of the planes is really read: one changed pixel in the last row moves the value
    b2 = b.clone()
    b2[0, :, 1023, 1023] = 1.0 - b2[0, :, 1023, 1023]
    assert lp(a, b2) != v


def test_cli_with_lpips_on_the_golden_scene(tmp_path, lp, weight_files):
    import inference
    from test_e2e_gpu import _tiny_cfgs
    from test_eval_gpu import SCENE, SCENE_DIR
    from diffuman4d_amd.host.weights import write_synthetic_checkpoint
    ucfg, vcfg = _tiny_cfgs()
    ckpt = write_synthetic_checkpoint(tmp_path / "ckpt", ucfg, vcfg, seed=3)
    result_dir = tmp_path / "res"
    inference.main(["exp=demo_4d_tiny", "model=diffuman4d_mi355x", f"data.data_dir={SCENE_DIR}", f"data.scene_label={SCENE}",
                    f"model.model_dir={ckpt}", "model.gpu_ids=[0]", "data.height=64", "data.width=64", f"result_dir={result_dir}",
                    "sampler.spa_label_range=[0,8,1]", "sampler.tem_label_range=[0,3,1]", "sampler.input_spa_labels=[1,5]",
                    "sampler.window_size=2", "sampler.sliding_stride=1", "evaluating=true", "to_nerfstudio=false",
                    f"evaluation.lpips_vgg16={weight_files[0]}", f"evaluation.lpips_lin={weight_files[1]}"])
    found = list(result_dir.rglob("metrics.json"))
    assert len(found) == 1
    m = json.loads(found[0].read_text())
    out_dir = found[0].parent
    targets = [f"{c:02d}" for c in range(8) if c not in (1, 5)]
    keys = [f"{c}/{f:06d}" for c in targets for f in range(3)]
    assert [v["key"] for v in m["values"]] == keys
    pairs = []
    for key in keys:
        fmask = str(SCENE_DIR / SCENE / "fmasks" / f"{key}.png")
        pairs.append(dict(pred=str(out_dir / "images" / f"{key}.jpg"), gt=str(SCENE_DIR / SCENE / "images" / f"{key}.webp"), pred_fmask=fmask,
                          gt_fmask=fmask, canvas_size=1024, crop_with_fmask=True, background_color="white"))
    own = metrics.ImageEvaluator(DEV, lpips=lp).evaluate_batch(pairs)
    for v, r in zip(m["values"], own):
        assert isinstance(v["lpips"], float) and math.isfinite(v["lpips"]) and v["lpips"] >= 0
        assert (v["psnr"], v["ssim"], v["lpips"]) == r
    assert m["mean"]["lpips"] == round(torch.tensor([v["lpips"] for v in m["values"]]).mean().item(), 3)


def test_eval_bench_lpips_report(weight_files):
    """tools/eval_bench.py --lpips: the report of time per pair without and with LPIPS, on two small pairs."""
    import importlib.util
    import types
    spec = importlib.util.spec_from_file_location("eval_bench", Path(__file__).resolve().parent.parent / "tools" / "eval_bench.py")
    eb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(eb)
    pairs = []
    for h, w in [(40, 56), (17, 31)]:
        a, b = lm.pair(h, w, 0.08, seed=h)
        pairs.append(dict(pred=b, gt=a, canvas_size=w, crop_with_fmask=False))
    r = eb.lpips_report(DEV, pairs, types.SimpleNamespace(lpips=list(weight_files), reps=1, threads=2, canvas=56))
    assert r["lpips_pairs"] == 2 and r["crop_of_pair_0"] == [40, 56] and r["lpips_of_pair_0"] > 0
    assert set(r) == {"lpips_pairs", "canvas", "crop_of_pair_0", "psnr_ssim_only_ms_per_pair", "with_lpips_ms_per_pair",
                      "lpips_call_span_ms_per_pair", "lpips_of_pair_0"}
    for k in ("psnr_ssim_only_ms_per_pair", "with_lpips_ms_per_pair", "lpips_call_span_ms_per_pair"):  # figures, not an ordering: no timing assertion
        assert math.isfinite(r[k]) and r[k] > 0, (k, r[k])


def test_a_callable_of_the_users_runs_on_the_evaluators_stream():
    """ImageEvaluator(lpips=callable): the callable gets (gt[None], pred[None]) fp32 on the device, with the evaluator's stream current
    (the one the composites were made on), and its result is the third value."""
    seen = []

    def user_lpips(gt, pred):
        seen.append((torch.cuda.current_stream(DEV), gt.shape, pred.shape, gt.dtype, gt.device))
        return (gt - pred).abs().mean().item()

    a, b = lm.pair(17, 31, 0.08, seed=3)
    ev = metrics.ImageEvaluator(DEV, lpips=user_lpips)
    _, _, val = ev(pred=b, gt=a, canvas_size=31, crop_with_fmask=False)
    assert abs(val - (a - b).abs().mean().item()) < 1e-6  # two fp32 means of 1581 values below 1, summed in different orders
    assert seen == [(ev._stream(), (1, 3, 17, 31), (1, 3, 17, 31), torch.float32, DEV)]
