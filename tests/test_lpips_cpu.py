"""CPU: the LPIPS weight loader and packer, the refusal of host tensors, `lpips_weights` through evaluate_results (the float32 evaluator
model of test_eval_cpu.py as the kernel wrapper, a stub in place of LpipsVGG), the CLI keys, and the new entries' argument checks."""
import json
import threading
import types
from pathlib import Path

import pytest
import torch

import eval_model as em
import lpips_model as lm
import test_eval_cpu as tec
from diffuman4d_amd.host import lib as L, lpips, metrics, ops


@pytest.fixture(scope="module")
def weights():
    return lm.random_weights(seed=1)


# -- loader -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["pth", "safetensors"])
def test_loader_reads_both_formats_and_ignores_the_classifier(tmp_path, weights, fmt):
    vgg, lin = lm.write_checkpoints(tmp_path, weights, fmt)
    w = lpips.load_lpips_weights(vgg, lin)
    shapes = lpips.conv_shapes()
    assert [i for i, _, _ in shapes] == [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28]
    assert [(ci, co) for _, ci, co in shapes] == [(3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512),
                                                  (512, 512), (512, 512), (512, 512), (512, 512), (512, 512)]
    assert len(w["conv"]) == 13 and len(w["lin"]) == 5 and set(w) == {"conv", "lin"}
    for (i, _, _), (wt, b) in zip(shapes, w["conv"]):
        assert torch.equal(wt, weights[f"features.{i}.weight"]) and torch.equal(b, weights[f"features.{i}.bias"])
    for l, t in enumerate(w["lin"]):
        assert t.shape == (lm.WIDTHS[l],) and torch.equal(t, weights[f"lin{l}.model.1.weight"].reshape(-1))


def test_loader_errors(tmp_path, weights):
    vgg, lin = lm.write_checkpoints(tmp_path / "good", weights)
    with pytest.raises(FileNotFoundError, match="absent.pth"):
        lpips.load_lpips_weights(str(tmp_path / "absent.pth"), lin)
    with pytest.raises(FileNotFoundError, match="nolin.safetensors"):
        lpips.load_lpips_weights(vgg, str(tmp_path / "nolin.safetensors"))
    bad = dict(weights)
    del bad["features.17.bias"]
    v2, l2 = lm.write_checkpoints(tmp_path / "nokey", bad)
    with pytest.raises(KeyError, match=r"features\.17\.bias.*vgg16-397923af\.pth"):
        lpips.load_lpips_weights(v2, l2)
    bad = dict(weights)
    del bad["lin3.model.1.weight"]
    v3, l3 = lm.write_checkpoints(tmp_path / "nolin", bad)
    with pytest.raises(KeyError, match=r"lin3\.model\.1\.weight.*vgg\.pth"):
        lpips.load_lpips_weights(v3, l3)
    bad = dict(weights)
    bad["features.5.weight"] = torch.zeros(128, 64, 3, 2)
    v4, l4 = lm.write_checkpoints(tmp_path / "shape", bad)
    with pytest.raises(ValueError, match=r"features\.5\.weight.*\(128, 64, 3, 2\).*\(128, 64, 3, 3\)"):
        lpips.load_lpips_weights(v4, l4)
    bad = dict(weights)
    bad["lin0.model.1.weight"] = torch.zeros(1, 32, 1, 1)
    v5, l5 = lm.write_checkpoints(tmp_path / "linshape", bad)
    with pytest.raises(ValueError, match=r"lin0\.model\.1\.weight.*\(1, 32, 1, 1\).*\(1, 64, 1, 1\)"):
        lpips.load_lpips_weights(v5, l5)


# -- weight packing -----------------------------------------------------------------------------------------------------------------
def test_packed_weights_layout_and_reconstruction(weights):
    for key, cols in (("features.0.weight", ops.LPIPS_IN_COLS), ("features.2.weight", 0), ("features.10.weight", 0)):
        w = weights[key]
        cout, cin = w.shape[:2]
        p = lpips.pack_conv_weight(w, cols)
        width = cols or 3 * cin
        assert p.dtype == torch.bfloat16 and p.shape == (cout, 9 * width)
        p = p.reshape(cout, 3, 3, width).float()  # (ky, kx, column)
        tap = w.permute(0, 2, 3, 1)               # (ky, kx, ci)
        hi, hi2, lo, rest = p[..., :cin], p[..., cin: 2 * cin], p[..., 2 * cin: 3 * cin], p[..., 3 * cin:]
        assert torch.equal(hi, tap.to(torch.bfloat16).float()) and torch.equal(hi2, hi)
        assert torch.equal(lo, (tap - hi).to(torch.bfloat16).float()) and not rest.any()
        # bf16 keeps 8 significant bits: |w - hi| <= 2^-9 |w|, and the same again for lo against that residue
        assert ((hi + lo - tap).abs() <= 2.0 ** -16 * tap.abs()).all()
        assert (hi + lo - tap).abs().max() > 0  # ... and the two terms are not the whole fp32 value: the bound is not vacuous


# -- no CPU path ----------------------------------------------------------------------------------------------------------------------
def test_there_is_no_cpu_path(tmp_path):
    with pytest.raises(L.Dm4dError, match="HIP device"):
        lpips.LpipsVGG("cpu", str(tmp_path / "never_read.pth"), str(tmp_path / "never_read2.pth"))
    a = torch.rand(3, 16, 16)
    with pytest.raises(L.Dm4dError, match="HIP device"):
        ops.lpips_input(a, a)
    with pytest.raises(L.Dm4dError, match="HIP device"):
        ops.lpips_relu_pool(torch.zeros(2, 4, 4, 64), pool=True)
    with pytest.raises(L.Dm4dError, match="HIP device"):
        ops.lpips_tap_distance(torch.zeros(2, 4, 4, 64), torch.zeros(64), 0, torch.zeros(5, dtype=torch.float64), torch.zeros(16, dtype=torch.uint8))


# -- evaluate_results ---------------------------------------------------------------------------------------------------------------
@pytest.fixture
def standin(monkeypatch):
    monkeypatch.setattr(metrics.ops, "eval_psnr_ssim", em.standin_eval_psnr_ssim)


def test_lpips_and_lpips_weights_together_are_refused(tmp_path, standin):
    out = tec.make_results(tmp_path / "res", ["00"], ["000001"])
    with pytest.raises(ValueError, match="either lpips= .* or lpips_weights="):
        tec._evaluate(out, lpips=lambda gt, pred: 0.0, lpips_weights=("a.pth", "b.pth"))
    with pytest.raises(ValueError, match="either lpips= .* or lpips_weights="):
        metrics.evaluate_keys(["00/000001"], "cpu", f"{out}/images", str(tec.SCENE / "images"), lpips=lambda gt, pred: 0.0,
                              lpips_weights=("a.pth", "b.pth"))


def test_lpips_weights_reach_every_worker_and_fill_the_metrics(tmp_path, standin, monkeypatch, caplog):
    made = []

    class StubLpips:
        def __init__(self, device, vgg16_path, lin_path):
            made.append((str(device), vgg16_path, lin_path, threading.current_thread().name))

        def __call__(self, gt, pred):
            assert gt.shape == pred.shape and gt.shape[:2] == (1, 3)
            return (gt - pred).abs().mean()

    monkeypatch.setattr(lpips, "LpipsVGG", StubLpips)
    out = tec.make_results(tmp_path / "res", tec.CAMS[:2], tec.FRAMES)
    path = tmp_path / "res" / "metrics.json"
    with caplog.at_level("INFO"):
        m = tec._evaluate(out, out_metrics_path=str(path), gpu_ids=["cpu", "cpu", "cpu"], batch_size=2, lpips_weights=("v.pth", "l.pth"))
    assert not any("LPIPS is not built" in r.message for r in caplog.records)
    assert len(made) == 3 and {x[:3] for x in made} == {("cpu", "v.pth", "l.pth")} and len({x[3] for x in made}) == 3  # one per worker thread
    assert json.loads(path.read_text()) == m and len(m["values"]) == 6
    for v in m["values"]:
        assert isinstance(v["lpips"], float) and 0 < v["lpips"] < 1
    assert m["mean"]["lpips"] == round(torch.tensor([v["lpips"] for v in m["values"]]).mean().item(), 3)
    assert '"lpips": null' not in path.read_text()


# -- CLI ------------------------------------------------------------------------------------------------------------------------------
def _run_cli(monkeypatch, evaluation):
    import inference
    from diffuman4d_amd.host import runner
    calls = []

    class FakeRunner:
        def __init__(self, sampler, **kw):
            pass

        def inference(self):
            calls.append(("inference", (), {}))

        def evaluate(self, *args, **kw):
            calls.append(("evaluate", args, kw))
            return {"mean": {"psnr": 1.0, "ssim": 1.0, "lpips": 0.5}, "values": []}

    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(runner, "SamplingRunner", FakeRunner)
    monkeypatch.setattr(inference.cfglib, "instantiate", lambda node, **kw: types.SimpleNamespace(output_dir="/nowhere"))
    cfg = {"data": {"_target_": "d"}, "model": {"_target_": "m"}, "sampler": {"_target_": "s"}, "sampling": False, "evaluating": True}
    if evaluation is not None:
        cfg["evaluation"] = evaluation
    inference.inference(cfg)
    return calls


def test_cli_passes_both_paths_as_lpips_weights(monkeypatch):
    assert _run_cli(monkeypatch, {"lpips_vgg16": "/w/vgg16.pth", "lpips_lin": "/w/vgg.pth"}) == \
        [("evaluate", (), {"lpips_weights": ("/w/vgg16.pth", "/w/vgg.pth")})]


def test_cli_without_the_keys_calls_evaluate_without_arguments(monkeypatch):
    assert _run_cli(monkeypatch, None) == [("evaluate", (), {})]
    assert _run_cli(monkeypatch, {}) == [("evaluate", (), {})]


@pytest.mark.parametrize("given,missing", [("lpips_vgg16", "lpips_lin"), ("lpips_lin", "lpips_vgg16")])
def test_cli_refuses_one_key_alone(monkeypatch, given, missing):
    with pytest.raises(ValueError, match=rf"evaluation\.{missing} is missing"):
        _run_cli(monkeypatch, {given: "/w/file.pth"})


def test_the_dotted_overrides_compose_into_the_evaluation_node():
    from diffuman4d_amd.host import config
    cfg = config.compose(["exp=demo_4d_tiny", "evaluation.lpips_vgg16=/w/vgg16-397923af.pth", "evaluation.lpips_lin=/w/vgg.pth"])
    assert cfg["evaluation"] == {"lpips_vgg16": "/w/vgg16-397923af.pth", "lpips_lin": "/w/vgg.pth"}


# -- ABI: argument errors before the device is touched --------------------------------------------------------------------------------
def test_lpips_entries_reject_bad_arguments():
    lib = L.load()
    last = lambda: lib.dm4d_last_error().decode()
    P = 0x10000  # a non-null "device" address that is never read: every call below fails its host-side check first
    assert lib.dm4d_lpips_input_split(None, None, P, 256, 16, 16, 16, P) == -1 and "null pointer" in last()
    assert lib.dm4d_lpips_input_split(None, P, P, 256, 16, 0, 16, P) == -1 and "bad image size" in last()
    assert lib.dm4d_lpips_input_split(None, P, P, 256, 8, 16, 16, P) == -1 and "overlap" in last()
    assert lib.dm4d_lpips_input_split(None, P, P, 100, 16, 16, 16, P) == -1 and "overlap" in last()
    assert lib.dm4d_lpips_input_split(None, P, P, 256, 16, 16, 16, P + 2) == -1 and "aligned" in last()
    assert lib.dm4d_lpips_relu_pool_split(None, P, None, 2, 4, 4, 64, 1) == -1 and "null pointer" in last()
    assert lib.dm4d_lpips_relu_pool_split(None, P, P, 2, 4, 4, 60, 1) == -1 and "multiple of 8" in last()
    assert lib.dm4d_lpips_relu_pool_split(None, P, P, 2, 1, 4, 64, 1) == -1 and "pooling" in last()
    assert lib.dm4d_lpips_relu_pool_split(None, P + 4, P, 2, 4, 4, 64, 0) == -1 and "aligned" in last()
    f = lib.dm4d_lpips_tap_distance_f64
    assert f(None, P, None, 4, 4, 64, 0, P, 1 << 10, P) == -1 and "null pointer" in last()
    assert f(None, P, P, 0, 4, 64, 0, P, 1 << 10, P) == -1 and "bad tap size" in last()
    assert f(None, P, P, 4, 4, 96, 0, P, 1 << 10, P) == -1 and "VGG-16 width" in last()
    assert f(None, P, P, 4, 4, 64, 5, P, 1 << 10, P) == -1 and "tap outside" in last()
    assert f(None, P, P, 4, 4, 64, 0, P + 8, 1 << 10, P) == -1 and "aligned" in last()
    assert f(None, P, P, 64, 64, 64, 0, P, 64, P) == -1 and "workspace too small" in last()
    assert lib.dm4d_lpips_ws_bytes(64, 64) == 16 * 8 and lib.dm4d_lpips_ws_bytes(17, 31) == 3 * 8 and lib.dm4d_lpips_ws_bytes(0, 5) == 0
