"""CPU: head dimensions 40 / 80 / 160 (the SD-1.x UNet layout, attention_head_dim = 8 heads at every level) -- the C ABI surface of
attention_hd.hip and its argument checks, the dispatch of host/ops.py by head dimension, and a UNet at that layout wired through the
REAL host classes with tests/cpu_standin_ops.py standing in for the kernel wrappers (the kernels themselves: tests/test_attention_hd_gpu.py)."""
import copy
import json
import math
import re
import subprocess
import sys
from dataclasses import asdict
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
NEW = ("dm4d_attention_hd_qscaled_kv_bf16", "dm4d_attention_hd_qscaled_kv_f16", "dm4d_attention_hd_split_bf16")
P = 0x10000  # a non-null, 16-byte aligned "device pointer" (never dereferenced: every call below fails its argument check)
ERR_ARG = -1


@pytest.fixture(scope="module")
def lib():
    from diffuman4d_amd.host import lib as L
    return L.load()


def last(lib):
    return lib.dm4d_last_error().decode()


def test_new_entries_are_declared_exported_and_bound(lib):
    from diffuman4d_amd.host import lib as L
    text = (ROOT / "include" / "dm4d.h").read_text()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(L.lib_path())], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (dm4d_\w+)", nm))
    for name in NEW:
        assert re.search(rf"\bint\s+{name}\s*\(", text), name
        assert name in exported, name
        assert name in L.SIGNATURES, name
    assert len(L.SIGNATURES[NEW[0]][1]) == 14 and len(L.SIGNATURES[NEW[2]][1]) == 19


@pytest.mark.parametrize("fn", NEW[:2])
def test_qscaled_entries_refuse_bad_arguments(lib, fn):
    a = getattr(lib, fn)
    # Q, K, V, O, ldq, ldk, ldv, ldo, batch, heads, head_dim, Lq, Lk
    for d in (32, 41, 64):
        assert a(None, P, P, P, P, 960, 960, 960, 320, 1, 8, d, 64, 64) == ERR_ARG
        assert f"head_dim {d}" in last(lib) and "own entry points" in last(lib)
    assert a(None, None, P, P, P, 960, 960, 960, 320, 1, 8, 40, 64, 64) == ERR_ARG
    assert "null pointer" in last(lib)
    assert a(None, P, P, P, P, 960, 960, 960, 320, 1, 8, 40, 0, 64) == ERR_ARG
    assert "empty shape" in last(lib)
    assert a(None, P, P, P, P, 312, 960, 960, 320, 1, 8, 40, 64, 64) == ERR_ARG  # below heads * head_dim
    assert ">= heads * head_dim" in last(lib)
    assert a(None, P, P, P, P, 964, 960, 960, 320, 1, 8, 40, 64, 64) == ERR_ARG
    assert "multiples of 8" in last(lib)
    assert a(None, P, P, P, P, 960, 960, 960, 320, 1 << 30, 8, 40, 1 << 20, 64) == ERR_ARG
    assert "grid too large" in last(lib)


def test_split_entry_refuses_bad_arguments(lib):
    a = lib.dm4d_attention_hd_split_bf16
    # Q, K, V, O, ldq, ldk, ldv, ldo, q_lo, k_lo, v_lo, o_lo, batch, heads, Lq, Lk, scale, head_dim
    args = [None, P, P, P, P, 1920, 1920, 1920, 640, 960, 960, 960, 320, 1, 8, 64, 64, 40 ** -0.5]
    for d in (32, 41, 64):
        assert a(*args, d) == ERR_ARG
        assert f"head_dim {d}" in last(lib)
    assert a(*(args[:3] + [None] + args[4:]), 80) == ERR_ARG
    assert "null pointer" in last(lib)
    assert a(*(args[:5] + [100] + args[6:]), 40) == ERR_ARG
    assert ">= heads * head_dim" in last(lib)
    assert a(*(args[:9] + [964] + args[10:]), 40) == ERR_ARG
    assert "plane offsets" in last(lib)


class _Recorder:
    """Stands in for the loaded libdm4d.so: records (entry name, arguments) and returns DM4D_OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


@pytest.fixture()
def recorder(monkeypatch):
    from diffuman4d_amd.host import lib as L
    from diffuman4d_amd.host import ops
    rec = _Recorder()
    monkeypatch.setattr(L, "load", lambda: rec)
    monkeypatch.setattr(ops, "_req", lambda t, name, dtype=ops.BF16: t)
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    return rec


@pytest.mark.parametrize("d", [64, 40, 80, 160])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_ops_attention_dispatches_by_head_dimension(recorder, d, dt):
    from diffuman4d_amd.host import ops
    heads, batch, seq = 8, 2, 24
    C = heads * d
    qkv = torch.zeros(batch * seq, 3 * C, dtype=dt)
    out = ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], batch, heads, seq, q_scaled=True)
    assert out.shape == (batch * seq, C)
    (name, args), = recorder.calls
    if d == 64:
        assert name == ("dm4d_attention_qscaled_kv_f16" if dt == torch.float16 else "dm4d_attention_qscaled_kv_bf16")
        assert args[5:] == (3 * C, 3 * C, 3 * C, C, batch, heads, seq, seq)
    else:
        assert name == ("dm4d_attention_hd_qscaled_kv_f16" if dt == torch.float16 else "dm4d_attention_hd_qscaled_kv_bf16")
        assert args[5:] == (3 * C, 3 * C, 3 * C, C, batch, heads, d, seq, seq)


@pytest.mark.parametrize("d", [64, 80])
def test_ops_attention_split_dispatches_by_head_dimension(recorder, d):
    from diffuman4d_amd.host import ops
    heads, batch, seq = 8, 1, 16
    C = heads * d
    ops.attention_split(torch.zeros(batch * seq, 6 * C, dtype=torch.bfloat16), batch, heads, seq)
    q = torch.zeros(batch * seq, 2 * C, dtype=torch.bfloat16)
    kv = torch.zeros(batch * 4 * seq, 4 * C, dtype=torch.bfloat16)
    ops.attention_split(None, batch, heads, seq, 0.3, q=q, kv=kv, kv_seq=4 * seq)
    (n1, a1), (n2, a2) = recorder.calls
    want = "dm4d_attention_split_bf16" if d == 64 else "dm4d_attention_hd_split_bf16"
    assert n1 == n2 == want
    assert math.isclose(a1[17], d ** -0.5, rel_tol=1e-12) and a2[17] == 0.3  # default scale d^-0.5
    assert a1[9:12] == (3 * C, 3 * C, 3 * C) and a2[9:12] == (C, 2 * C, 2 * C)
    if d != 64:
        assert a1[18] == d and a2[18] == d


def test_ops_attention_refuses_other_head_dimensions(recorder):
    from diffuman4d_amd.host import lib as L
    from diffuman4d_amd.host import ops
    x = torch.zeros(16, 8 * 32, dtype=torch.bfloat16)
    with pytest.raises(L.Dm4dError, match="supported head dimensions are 64, 40, 80, 160"):
        ops.attention(x, x, x, 1, 8, 16, q_scaled=True)
    y = torch.zeros(16, 8 * 40, dtype=torch.bfloat16)
    with pytest.raises(L.Dm4dError, match="pre-scaled Q"):
        ops.attention(y, y, y, 1, 8, 16)
    assert recorder.calls == []


# ---- a UNet at the SD-1.x layout, host side, on the CPU stand-in -------------------------------------------------------------------
def _attention_any_d(q, k, v, batch, heads, seq, scale=None, out=None, kv_seq=None, q_scaled=False):
    """cpu_standin_ops.attention for any head dimension (the stand-in's own is written for 64)."""
    import cpu_standin_ops as so
    kv_seq = kv_seq or seq
    d = q.shape[1] // heads
    hv = lambda t, L: t.double().reshape(batch, L, heads, d).transpose(1, 2)  # noqa: E731
    s = hv(q, seq) @ hv(k, kv_seq).transpose(-1, -2)
    p = torch.softmax(s * (math.log(2.0) if q_scaled else (d ** -0.5 if scale is None else scale)), dim=-1)
    assert q.dtype == k.dtype == v.dtype and (q.dtype == so.BF or q_scaled)
    o = p @ hv(v, kv_seq)
    return o.transpose(1, 2).reshape(batch * seq, heads * d).to(q.dtype)


def _attention_split_any_d(qkv, batch, heads, seq, scale=None, *, q=None, kv=None, kv_seq=None):
    import cpu_standin_ops as so
    if qkv is not None:
        C = qkv.shape[1] // 6
        val = qkv[:, :3 * C].double() + qkv[:, 3 * C:].double()
        qv, kval, vval, kv_seq = val[:, :C], val[:, C:2 * C], val[:, 2 * C:], seq
    else:
        C = q.shape[1] // 2
        kv_seq = kv_seq or seq
        qv = q[:, :C].double() + q[:, C:].double()
        kval, vval = kv[:, :C].double() + kv[:, 2 * C:3 * C].double(), kv[:, C:2 * C].double() + kv[:, 3 * C:].double()
    d = C // heads
    hv = lambda t, L: t.reshape(batch, L, heads, d).transpose(1, 2)  # noqa: E731
    o = torch.softmax(hv(qv, seq) @ hv(kval, kv_seq).transpose(-1, -2) * (d ** -0.5 if scale is None else scale), dim=-1) @ hv(vval, kv_seq)
    return so._out(o.transpose(1, 2).reshape(batch * seq, C).float(), split=True)


def _install_standin_any_d():
    """cpu_standin_ops.install() with the attention wrappers replaced by the head-dimension-generic ones above.  Set directly (not through
    monkeypatch): cpu_standin_ops.uninstall() restores the real wrappers it saved at install, and nothing is left behind afterwards."""
    import cpu_standin_ops as fake_ops
    from diffuman4d_amd.host import ops
    fake_ops.install()
    ops.attention, ops.attention_split = _attention_any_d, _attention_split_any_d
    return fake_ops


SD1X = dict(block_out_channels=(320, 640, 1280, 1280), attention_head_dim=8)


def _sd1x_wiring_check():
    """Body of test_sd1x_unet_constructs_and_is_wired; run in a child process (see the test)."""
    import modelcheck as mc
    from diffuman4d_amd.host import ops
    from diffuman4d_amd.host.unet import UNetConfig, UNetMultiviewConditionModel
    cfg, om = mc.make_unet(0, **SD1X)
    g = torch.Generator().manual_seed(1)
    F = 4
    x = torch.randn(F, cfg.in_channels, 16, 8, generator=g).to(torch.bfloat16)
    t = torch.randint(0, 1000, (F,), generator=g)
    with torch.no_grad():
        ref = om(x.float(), t, domains=["spatial"], num_frames=F)
        yard = mc.rel_l2(copy.deepcopy(om).to(torch.bfloat16)(x, t, domains=["spatial"], num_frames=F).float(), ref)
    assert math.isfinite(yard), yard
    fake_ops = _install_standin_any_d()
    try:
        for precision in ("parity", "fp16", "fast"):
            hm = UNetMultiviewConditionModel(UNetConfig.from_dict(asdict(cfg)), om.state_dict(), "cpu", precision)
            if precision == "fast":
                got = sorted({(t_.pob.shape[0] // t_.blocks[0].heads, t_.blocks[0].heads) for t_ in _transformers(hm)})
                assert got == [(40, 8), (80, 8), (160, 8)], got
            if hm.wide:
                xd = ops.split(x.float().permute(0, 2, 3, 1).contiguous(), cpad=hm.IN_PAD, h16=hm.h16)
            else:
                xd = ops.nchw_to_nhwc(x, hm.IN_PAD)
            e = mc.rel_l2(ops.nhwc_to_nchw(hm(xd, t.float(), domains=["spatial"], num_frames=F)), ref)
            bound = {"parity": 1e-4, "fp16": mc.FP16_BOUNDS["unet_out"]}.get(precision, mc.YARD_FACTOR * yard)
            print(f"{precision}: unet_out rel-L2 {e:.3e} (bound {bound:.3e}, bf16-oracle yardstick {yard:.3e})", flush=True)
            assert e <= bound, (precision, e, bound)
            del hm
    finally:
        fake_ops.uninstall()


def _in_child(fn: str, *args: str):
    """Run this module's function `fn(*args)` in a fresh interpreter.  The tests that build models on the CPU (gigabytes of weights, the CPU
    math libraries' caches and allocator state) run there, so that nothing of theirs stays in the test process for the tests that follow."""
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [
        "-c", "import sys; sys.path[:0] = sys.argv[1:3]; import test_attention_hd_cpu as t; getattr(t, sys.argv[3])(*sys.argv[4:])",
        str(ROOT), str(ROOT / "tests"), fn, *args]
    r = subprocess.run(cmd, cwd=str(ROOT), capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, f"{fn}: child exited {r.returncode}\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
    return r.stdout


def test_sd1x_unet_constructs_and_is_wired():
    """(320, 640, 1280, 1280) channels, 8 heads everywhere (head dimensions 40 / 80 / 160), a 16 x 8 latent, 4 frames: the three
    precisions against the fp32 oracle with the bounds the project uses for a UNet call (parity 1e-4, fp16 FP16_BOUNDS["unet_out"],
    fast YARD_FACTOR x the bf16-oracle yardstick).  modelcheck.case_unet's arithmetic, on CPU tensors, in a child process."""
    out = _in_child("_sd1x_wiring_check")
    assert out.count("unet_out rel-L2") == 3, out


def _transformers(hm):
    from diffuman4d_amd.host.unet import _Transformer
    seen, out = set(), []

    def walk(o, depth=0):
        if id(o) in seen or depth > 4:
            return
        seen.add(id(o))
        if isinstance(o, _Transformer):
            out.append(o)
            return
        items = o if isinstance(o, (list, tuple)) else (vars(o).values() if hasattr(o, "__dict__") else ())
        for v in items:
            if isinstance(v, (list, tuple)) or (hasattr(v, "__dict__") and type(v).__module__.startswith("diffuman4d_amd")):
                walk(v, depth + 1)
    walk(hm)
    return out


def test_other_head_dimensions_still_refused_at_load():
    import modelcheck as mc
    from diffuman4d_amd.host.unet import UNetConfig, UNetMultiviewConditionModel
    cfg, om = mc.make_unet(0, block_out_channels=(96, 192, 192, 192), attention_head_dim=1)  # head dimension 96
    with pytest.raises(NotImplementedError, match=r"^unet/config.json: block_out_channels / attention_head_dim give a head dimension of "
                                                  r"96 at .*40, 64, 80, 160"):
        UNetMultiviewConditionModel(UNetConfig.from_dict(asdict(cfg)), om.state_dict(), "cpu")


def test_int_attention_head_dim_flows_through_config_shapes_and_checkpoint(tmp_path):
    """diffusers writes `"attention_head_dim": 8` (an int) for SD-1.x: UNetConfig.from_dict / heads(i), unet_param_shapes,
    write_synthetic_checkpoint, and load_pipelines' config path (Diffuman4DPipeline.from_pretrained -> UNet config.json)."""
    from diffuman4d_amd.host.unet import UNetConfig
    from diffuman4d_amd.host.weights import unet_param_shapes
    cfg = UNetConfig.from_dict(json.loads(json.dumps(dict(asdict(UNetConfig()), attention_head_dim=8))))
    assert cfg.attention_head_dim == 8 and [cfg.heads(i) for i in range(4)] == [8, 8, 8, 8]
    shapes = unet_param_shapes(cfg)
    assert shapes["down_blocks.0.attentions.0.transformer_blocks.0.attn1.to_q.weight"] == (320, 320)
    assert shapes["mid_block.attentions.0.transformer_blocks.0.attn1.to_k.weight"] == (1280, 1280)
    out = _in_child("_sd1x_checkpoint_load_check", str(tmp_path / "ckpt"))
    assert "head dimensions [40, 80, 160]" in out, out


def _sd1x_checkpoint_load_check(path: str):
    """Body of the checkpoint part of the test above (write_synthetic_checkpoint -> load_pipelines); run in a child process."""
    import diffuman4d_amd.host.pipeline as hp
    from diffuman4d_amd.host import ops
    from diffuman4d_amd.host.loader import load_pipelines
    from diffuman4d_amd.host.unet import UNetConfig
    from diffuman4d_amd.host.vae import VAEConfig
    from diffuman4d_amd.host.weights import write_synthetic_checkpoint
    small = UNetConfig(block_out_channels=(80, 160, 320, 320), attention_head_dim=2, norm_num_groups=16)  # head dimensions 40 / 80 / 160
    ckpt = write_synthetic_checkpoint(path, small, VAEConfig(block_out_channels=(32, 32, 64, 64), norm_num_groups=8))
    written = json.loads((Path(ckpt) / "unet" / "config.json").read_text())
    assert written["attention_head_dim"] == 2 and written["block_out_channels"] == [80, 160, 320, 320]
    wrappers = (ops.attention, ops.attention_split)
    real = hp.Diffuman4DPipeline.from_pretrained.__func__
    hp.Diffuman4DPipeline.from_pretrained = classmethod(lambda cls, d, torch_dtype=torch.bfloat16, device="cuda", precision="fast":
                                                        real(cls, d, torch_dtype, "cpu", precision))
    fake_ops = _install_standin_any_d()
    try:
        pipe, = load_pipelines(model_dir=ckpt, torch_dtype="bf16", gpu_ids=[0], precision="parity")
    finally:
        fake_ops.uninstall()
    assert (ops.attention, ops.attention_split) == wrappers  # the real wrappers are back
    assert pipe.unet.config.attention_head_dim == 2
    dims = sorted({t.pob.shape[0] // t.blocks[0].heads for t in _transformers(pipe.unet)})
    assert dims == [40, 80, 160], dims
    print("head dimensions", dims, flush=True)
