"""GPU: the per-sweep prefix cache of Diffuman4DPipeline.window_call is a memoisation -- every row the UNet returns and the latents
after the calls are bit for bit what the single path (prefix_cache off = DM4D_PREFIX_CACHE=0) gives.

Sweep: 5 conditioning rows and 3 target rows per task, 4 consecutive window calls of 2 conditioning + 3 target frames in which one
conditioning frame slides per call ([c0 c1 | t], [c1 c2 | t], ...): call 0 computes everything, calls 1-3 copy one conditioning frame
from the cache and compute the other.  Two stacked tasks (copies = 2), CFG 2.  Latent 24 x 8 = 192 tokens: the 10 frames x 2 halves of
a full batch and the 8 x 2 of a compact one both end in ragged 256-row tiles at level 0."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H, W, N_COND, N_TGT, CALLS, COPIES = 24, 8, 5, 3, 4, 2
N = N_COND + N_TGT


def sliding_plan():
    from diffuman4d_amd.host.schedule import SweepPlan
    tgt = np.arange(N_COND, N)
    windows = [np.concatenate([[i, i + 1], tgt]) for i in range(CALLS)]
    is_cond = [np.array([True, True] + [False] * N_TGT) for _ in range(CALLS)]
    tix = [np.array([0, 0] + [i] * N_TGT, dtype=np.int64) for i in range(CALLS)]
    final = np.array([0] * N_COND + [CALLS] * N_TGT)
    return SweepPlan(num_inference_steps=CALLS, windows=windows, is_cond=is_cond, timestep_index=tix, final_timestep_indices=final,
                     target_indices=tgt, input_indices=np.arange(N_COND))


_MODELS = {}


def model(kind: str, precision: str, **cfg_kw):
    """One UNet per (geometry, precision, config) for the module."""
    key = (kind, precision, tuple(sorted(cfg_kw.items())))
    if key not in _MODELS:
        from diffuman4d_amd.host.unet import UNetConfig, UNetMultiviewConditionModel
        from diffuman4d_amd.host.weights import random_state_dict, unet_param_shapes
        if kind == "tiny":  # the geometry of the modelcheck cases (oracle UNetConfig.tiny)
            cfg = UNetConfig(block_out_channels=(64, 128, 128, 128), attention_head_dim=(1, 2, 2, 2), **cfg_kw)
        else:  # SD-2.1 widths on the two levels the head runs through (C = 320: l0_head_kernel, ff_proj_fused_kernel; C = 640)
            cfg = UNetConfig(block_out_channels=(320, 640, 640, 640), attention_head_dim=(5, 10, 10, 10), **cfg_kw)
        sd = random_state_dict(unet_param_shapes(cfg), 5, "cuda")
        _MODELS[key] = UNetMultiviewConditionModel(cfg, sd, "cuda", precision)
    return _MODELS[key]


def pipeline(unet, cache: bool):
    from diffuman4d_amd.host.pipeline import Diffuman4DPipeline
    from diffuman4d_amd.host.scheduler import DDIMScheduler
    pipe = Diffuman4DPipeline(None, unet, DDIMScheduler(), "cuda")
    pipe.prefix_cache = cache
    return pipe


def task_tensors(dtype, seed=3):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda c, s=1.0: (torch.randn(COPIES * N, H * W, c, generator=g, device="cuda") * s).to(torch.bfloat16).to(dtype)  # noqa: E731
    mask = torch.tensor([0.0] * N_COND + [1.0] * N_TGT, device="cuda").repeat(COPIES)[:, None, None].expand(-1, H * W, 1).to(dtype).contiguous()
    return dict(pv=rnd(4), pl=rnd(6, 0.5), sk=rnd(4), cm=mask, lat=rnd(4))


def sweep(pipe, t, monkeypatch, calls=range(CALLS), write_pv_before=None, tb=None, cfg=2.0):
    """Runs the window calls; returns (the UNet's result of every call, the latents after them, the tables)."""
    from diffuman4d_amd.host import ops
    eps = []
    real = ops.cfg_ddim_step
    monkeypatch.setattr(ops, "cfg_ddim_step", lambda lat, noise_pred, *a, **k: (eps.append(noise_pred.clone()), real(lat, noise_pred, *a, **k))[1])
    tb = tb or pipe.upload_plan(sliding_plan(), cfg, copies=COPIES, rows_per_task=N)
    lat = t["lat"].clone()
    for i in calls:
        if write_pv_before == i:
            t["pv"][2].mul_(0.5)  # conditioning row 2 = a frame of calls 1 and 2
        pipe.window_call(lat, t["pv"], t["pl"], t["sk"], t["cm"], tb, i, H, W, ["spatial"] * tb["cfg"], cfg, tb["cfg"] == 2, False)
    torch.cuda.synchronize()
    monkeypatch.setattr(ops, "cfg_ddim_step", real)
    return eps, lat, tb


def assert_same(a, b):
    (ea, la, _), (eb, lb, _) = a, b
    assert len(ea) == len(eb)
    for i, (x, y) in enumerate(zip(ea, eb)):
        assert x.shape == y.shape and torch.equal(x, y), f"call {i}: the UNet's result differs"
    assert torch.equal(la, lb) and bool(torch.isfinite(la.float()).all())


@pytest.mark.parametrize("kind,precision", [("tiny", "fast"), ("tiny", "fp16"), ("tiny", "parity"), ("sd21", "fast")])
def test_cached_sweep_equals_the_single_path(kind, precision, monkeypatch):
    unet = model(kind, precision)
    dtype = torch.float32 if unet.wide else torch.bfloat16
    ref = sweep(pipeline(unet, False), task_tensors(dtype), monkeypatch)
    got = sweep(pipeline(unet, True), task_tensors(dtype), monkeypatch)
    assert_same(got, ref)
    book = got[2]["prefix"]["book"]
    assert len(book.filled) == COPIES * N_COND and not torch.equal(got[1], task_tensors(dtype)["lat"])
    # partial hits: calls 1-3 ran the head on one conditioning + three target frames per task, call 0 on all five
    assert [sorted(len(k[1]) for k in book._memo if k[0] == i) for i in range(CALLS)] == [[COPIES * 5]] + [[COPIES * (N_TGT + 1)]] * (CALLS - 1)


@pytest.mark.parametrize("kind", ["tiny", "sd21"])
def test_groupnorm_statistics_are_chunked_as_in_the_full_batch(kind, monkeypatch):
    """GroupNorm sums a sample's statistics over ceil(2048 / batch) chunks of its pixels (at most one per 16 pixels), so a compact run
    must plan them for the full batch.  48 x 32 latents (96 chunks at most) and four stacked tasks: 52 chunks at the full batch of 40,
    64 at a compact batch of 32 planned on its own -- the sizes above are too small to tell."""
    import sys
    me = sys.modules[__name__]
    monkeypatch.setattr(me, "H", 48), monkeypatch.setattr(me, "W", 32), monkeypatch.setattr(me, "COPIES", 4)
    unet = model(kind, "fast")
    ref = sweep(pipeline(unet, False), task_tensors(torch.bfloat16), monkeypatch)
    got = sweep(pipeline(unet, True), task_tensors(torch.bfloat16), monkeypatch)
    assert_same(got, ref)


def test_wrapped_around_calls_hit_the_cache_with_pruning_and_without_cfg(monkeypatch):
    """A second pass over the same calls (bench.py's call index wraps) copies every conditioning frame; prune_cond_rows and cfg = 1."""
    unet = model("tiny", "fast")
    for prune, cfg in ((True, 2.0), (False, 1.0)):
        outs = []
        for cache in (False, True):
            pipe = pipeline(unet, cache)
            pipe.prune_cond_rows = prune
            outs.append(sweep(pipe, task_tensors(torch.bfloat16), monkeypatch, calls=list(range(CALLS)) * 2, cfg=cfg))
        assert_same(outs[1], outs[0])


def test_in_place_write_to_a_task_tensor_drops_the_cache(monkeypatch):
    unet = model("tiny", "fast")
    ref = sweep(pipeline(unet, False), task_tensors(torch.bfloat16), monkeypatch, write_pv_before=2)
    got = sweep(pipeline(unet, True), task_tensors(torch.bfloat16), monkeypatch, write_pv_before=2)
    assert_same(got, ref)
    stale = sweep(pipeline(unet, False), task_tensors(torch.bfloat16), monkeypatch)
    assert not torch.equal(stale[0][2], ref[0][2])  # the write does change call 2


class OneRankShard:
    """What window_call and the 3-D transformers ask of parallel.FrameShard, for a group of one rank (no process group)."""
    world = 1

    def local_frames(self, n):
        return slice(0, n)

    def gather_kv_start(self, kv):
        return kv

    def gather_kv_finish(self, pending):
        return pending

    def gather_rows(self, rows):
        return rows


def launches(pipe, monkeypatch, shard=None):
    """(family, rows) of every launch of calls 0 and 1, and the tables."""
    from diffuman4d_amd.host import ops
    monkeypatch.setattr(ops, "PROFILE", [])
    copies = 1 if shard is not None else COPIES
    t = {k: v[:copies * N] for k, v in task_tensors(torch.bfloat16).items()}
    tb = pipe.upload_plan(sliding_plan(), 2.0, shard, copies=copies, rows_per_task=N if copies > 1 else 0)
    lat = t["lat"].clone()
    counts = []
    for i in (0, 1):
        before = len(ops.PROFILE)
        pipe.window_call(lat, t["pv"], t["pl"], t["sk"], t["cm"], tb, i, H, W, ["spatial"] * 2, 2.0, True, False, shard)
        counts.append([(f, r) for f, _, _, _, _, r in ops.PROFILE[before:]])
    torch.cuda.synchronize()
    return counts, tb


def test_models_and_calls_outside_the_scope_take_the_single_path(monkeypatch):
    """ops.PROFILE launch lists: with the cache, call 1 moves rows and runs smaller head launches; an enable_tem_embeds model and a byte
    cap below one sweep's cache launch exactly what the switch-off path launches."""
    unet = model("tiny", "fast")
    off, _ = launches(pipeline(unet, False), monkeypatch)
    on, tb = launches(pipeline(unet, True), monkeypatch)
    assert "prefix" in tb and any(f == "rows_move" for f, _ in on[1]) and not any(f == "rows_move" for f, _ in off[1])
    assert [x for x in on[1] if x[0] != "rows_move"] != off[1] and len([x for x in on[1] if x[0] != "rows_move"]) == len(off[1])
    capped = pipeline(unet, True)
    capped.prefix_cache_max_bytes = 1 << 20
    got, tb = launches(capped, monkeypatch)
    assert got[1] == off[1] and not tb["prefix"]["chunks"]
    tem = model("tiny", "fast", enable_tem_embeds=True)
    off_t, _ = launches(pipeline(tem, False), monkeypatch)
    on_t, tb = launches(pipeline(tem, True), monkeypatch)
    assert on_t == off_t and "prefix" not in tb
    off_s, _ = launches(pipeline(unet, False), monkeypatch, shard=OneRankShard())
    on_s, tb = launches(pipeline(unet, True), monkeypatch, shard=OneRankShard())
    assert on_s == off_s and "prefix" not in tb and all(f != "rows_move" for c in on_s for f, _ in c)
