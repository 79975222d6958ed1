#!/usr/bin/env python
"""Golden vector for the SD-1.x attention layout at the JUDGED shape: the CPU oracle (oracle/unet.py, fp32) with widths (320, 640, 1280, 1280)
and `attention_head_dim = 8` (8 heads at every level, head dimensions 40 / 80 / 160 -- the reference's own constructor default,
unet_multiview_condition.py:184, :222-228), one spatial window call on 72 x 40 latents: F = 16 frames (4 conditioning + 12 targets), CFG
batch 32.

    python tests/golden/make_golden_sd1x.py          (~5 min on 8 cores)

writes tests/golden/sd1x_72x40.pt: unet_f16_spatial = the fp32 oracle output of the POSITIVE CFG half (rows 16..31, stored fp32: the
whole output would exceed the size limit of a committed file), the rel-L2 of the oracle run in bf16 against it on the same rows (the
yardstick), input and weight checksums.  Weights are not stored: both sides rebuild them with random_state_dict(shapes, seed, "cpu")
(make_golden_sd21.py's convention); tests/test_unet_sd1x_gpu.py checks the checksums first.
"""
from __future__ import annotations

import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(Path(__file__).resolve().parent))
OUT = Path(__file__).resolve().parent / "sd1x_72x40.pt"

BF = torch.bfloat16
UNET_SEED = 0
HEADS = 8


def host_config():
    from diffuman4d_amd.host.unet import UNetConfig
    return UNetConfig(attention_head_dim=HEADS)


def build_unet():
    from dataclasses import asdict

    from diffuman4d_amd.host.weights import random_state_dict, unet_param_shapes
    from oracle.unet import UNetConfig, UNetMultiviewConditionModel
    hc = host_config()
    cfg = UNetConfig(**{k: v for k, v in asdict(hc).items() if k in UNetConfig.__dataclass_fields__})
    sd = random_state_dict(unet_param_shapes(hc), UNET_SEED, "cpu")
    m = UNetMultiviewConditionModel(cfg).eval()
    res = m.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return m, float(sum(v.float().abs().sum() for v in sd.values()))


def main():
    import make_golden_sd21 as mk
    num_frames, n_cond, domain, seed = 16, 4, "spatial", 7
    m, wchk = build_unet()
    x, t = mk.unet_inputs(num_frames, n_cond, seed)
    half = slice(num_frames, 2 * num_frames)  # the positive CFG half
    with torch.no_grad():
        t0 = time.time()
        ref = m(x.float(), t, domains=[domain] * 2, num_frames=num_frames)
        t_fp32 = time.time() - t0
        m.to(BF)
        t0 = time.time()
        ref_bf = m(x, t, domains=[domain] * 2, num_frames=num_frames).float()
        t_bf = time.time() - t0
    blob = {"unet_f16_spatial": dict(out_f32=ref[half].clone(), rows=(half.start, half.stop), yard_bf16=mk.rel_l2(ref_bf[half], ref[half]),
                                     num_frames=num_frames, n_cond=n_cond, domain=domain, seed=seed, t=t, heads=HEADS,
                                     x_checksum=float(x.float().abs().sum()), weights_checksum=wchk, oracle_seconds=(t_fp32, t_bf),
                                     threads=torch.get_num_threads(), size=(mk.LAT_H, mk.LAT_W))}
    torch.save(blob, OUT)
    print(f"unet_f16_spatial: fp32 {t_fp32:.1f}s bf16 {t_bf:.1f}s yardstick {blob['unet_f16_spatial']['yard_bf16']:.3e} -> {OUT} "
          f"({OUT.stat().st_size} bytes)", flush=True)


if __name__ == "__main__":
    main()
