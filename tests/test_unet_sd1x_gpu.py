"""GPU: the UNet at the SD-1.x attention layout (attention_head_dim = 8 heads at every level, i.e. head dimensions 40 / 80 / 160 over
320 / 640 / 1280 channels; reference unet_multiview_condition.py:184, :222-228) through the real model classes.

The small geometry below is (320, 640, 640, 640) channels with (8, 8, 4, 4) heads: head dimensions 40, 80 and 160 at a size the CPU
oracle handles in seconds.  It keeps production channel counts (320 / 640) rather than (160, 320, 320, 320) so that every non-attention
kernel sees a width the SD-2.1 path already runs."""
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

SMALL = dict(block_out_channels=(320, 640, 640, 640), attention_head_dim=(8, 8, 4, 4))


@pytest.fixture()
def sd1x_small(monkeypatch):
    import modelcheck as mc
    real = mc.make_unet
    monkeypatch.setattr(mc, "make_unet", lambda seed=0, **kw: real(seed, **dict(kw, **SMALL)))
    return mc


@pytest.mark.parametrize("precision", ["fast", "fp16", "parity"])
def test_frame_shard_is_bitwise_at_the_sd1x_layout(hip_device, sd1x_small, precision):
    """modelcheck.case_unet_frame_shard at the SD-1.x head dimensions: every rank's slice of the UNet output equals the unsharded output
    bitwise, and what it contributes to each K | V all-gather equals the unsharded slice."""
    worst, _ = sd1x_small.case_unet_frame_shard(P=4, num_frames=8, h=16, w=8, tem=True, precision=precision)
    assert worst == 0.0, worst


@pytest.mark.parametrize("precision", ["fast", "fp16", "parity"])
def test_unet_call_at_the_sd1x_layout(hip_device, sd1x_small, precision):
    """One UNet call (4 frames, CFG batch 2, 16 x 8 latent) against the fp32 oracle: parity 1e-4, fp16 FP16_BOUNDS["unet_out"], fast
    YARD_FACTOR x the bf16-oracle yardstick."""
    mc = sd1x_small
    err, yard = mc.case_unet(num_frames=4, cfg_batch=2, h=16, w=8, precision=precision)
    e = err["unet_out"]
    bound = {"parity": 1e-4, "fp16": mc.FP16_BOUNDS["unet_out"]}.get(precision, mc.YARD_FACTOR * yard["unet_out"])
    assert e <= bound, (precision, e, bound)


def test_sliding_task_fp16_at_the_sd1x_layout(hip_device, sd1x_small):
    """One whole sliding task (VAE encode -> window sweep -> VAE decode) in the fp16 precision at the small SD-1.x geometry against the
    oracle pipeline: decoded RGB within 1e-3, latents within FP16_BOUNDS["latents"]."""
    mc = sd1x_small
    err, _ = mc.case_pipeline(precision="fp16")
    assert "bookkeeping" not in err
    assert err["images"] <= 1e-3 and err["latents"] <= mc.FP16_BOUNDS["latents"], err


def test_cli_path_on_an_sd1x_checkpoint(tmp_path):
    """config.compose -> load_pipelines (unet/config.json with the int `"attention_head_dim": 8`, as diffusers writes it for SD-1.x) ->
    sampler -> runner: the grid is fully denoised and every cell is written."""
    from diffuman4d_amd.host import config as cfglib
    from diffuman4d_amd.host.results import check_sampling_results
    from diffuman4d_amd.host.runner import SamplingRunner
    from diffuman4d_amd.host.unet import UNetConfig
    from diffuman4d_amd.host.vae import VAEConfig
    from diffuman4d_amd.host.weights import write_synthetic_checkpoint
    ucfg = UNetConfig(block_out_channels=(320, 640, 640, 640), attention_head_dim=8)  # head dimensions 40 / 80 / 80
    ckpt = write_synthetic_checkpoint(tmp_path / "ckpt", ucfg, VAEConfig(block_out_channels=(32, 32, 64, 64), norm_num_groups=8), seed=3)
    ov = ["exp=demo_4d_tiny", "model=diffuman4d_mi355x", "data=synthetic", f"model.model_dir={ckpt}", "model.gpu_ids=[0]",
          "data.height=64", "data.width=64", "data.num_cameras=8", f"result_dir={tmp_path / 'results'}",
          "sampler.spa_label_range=[0,8,1]", "sampler.tem_label_range=[0,4,1]", "sampler.input_spa_labels=[1,5]",
          "sampler.window_size=4", "sampler.sliding_stride=2"]
    cfg = cfglib.compose(ov)
    pipelines = cfglib.instantiate(cfg["model"])
    assert pipelines[0].unet.config.attention_head_dim == 8
    sampler = cfglib.instantiate(cfg["sampler"], dataset=cfglib.instantiate(cfg["data"]), pipelines=pipelines)
    SamplingRunner(sampler, prefetch_depth=2, writers=2).inference()
    steps = 4 // 2 * 3
    assert all(sampler.timestep_indices[c][f] == steps for c in sampler.target_spa_labels for f in sampler.tem_labels)
    assert check_sampling_results(sampler.spa_labels, sampler.tem_labels, sampler.output_dir)
    lat = torch.stack([sampler.latents[c][f].float() for c in sampler.target_spa_labels for f in sampler.tem_labels])
    assert bool(torch.isfinite(lat).all())


@pytest.mark.parametrize("precision", ["fast", "fp16", "parity"])
def test_judged_window_call_at_the_sd1x_layout(hip_device, precision):
    """One spatial window call at the judged shape (72 x 40 latents, F = 16, CFG batch 32) with widths (320, 640, 1280, 1280) and 8 heads,
    against the fp32 oracle output recorded in tests/golden/sd1x_72x40.pt (tests/golden/make_golden_sd1x.py) on the positive CFG half:
    fast <= YARD_FACTOR x the bf16-oracle yardstick, fp16 <= FP16_BOUNDS["unet_out"], parity <= 1e-4."""
    import modelcheck as mc
    from diffuman4d_amd.host import ops
    from diffuman4d_amd.host.unet import UNetMultiviewConditionModel
    from diffuman4d_amd.host.weights import random_state_dict, unet_param_shapes
    sys.path.insert(0, str(mc.GOLDEN))
    import make_golden_sd1x as mk1
    import make_golden_sd21 as mk
    g = torch.load(mc.GOLDEN / "sd1x_72x40.pt")["unet_f16_spatial"]
    cfg = mk1.host_config()
    sd = random_state_dict(unet_param_shapes(cfg), mk1.UNET_SEED, "cpu")
    mc._check_fixture_inputs("UNet weights", float(sum(v.float().abs().sum() for v in sd.values())), g["weights_checksum"])
    x, t = mk.unet_inputs(g["num_frames"], g["n_cond"], g["seed"])
    mc._check_fixture_inputs("UNet input", float(x.float().abs().sum()), g["x_checksum"])
    assert torch.equal(t, g["t"])
    hm = UNetMultiviewConditionModel(cfg, sd, "cuda", precision)
    del sd
    out = ops.nhwc_to_nchw(hm(mc.unet_sample(hm, x), t.float().cuda(), domains=[g["domain"]] * 2, num_frames=g["num_frames"]))
    r0, r1 = g["rows"]
    e = mc.rel_l2(out[r0:r1], g["out_f32"])
    bound = {"parity": 1e-4, "fp16": mc.FP16_BOUNDS["unet_out"]}.get(precision, mc.YARD_FACTOR * g["yard_bf16"])
    print(f"    [sd1x 72x40 F=16 {precision}] unet_out rel_l2={e:.3e} (oracle-bf16 {g['yard_bf16']:.3e}, bound {bound:.3e})", flush=True)
    del hm
    torch.cuda.empty_cache()
    assert e <= bound, (precision, e, bound)
