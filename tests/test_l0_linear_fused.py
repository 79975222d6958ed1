"""proj_in + norm1 + QKV projection of a level-0 transformer (C = 320) in one launch (ops.proj_in_ln_qkv, l0_head_kernel).

GPU: the fused launch against the three launches it replaces and against fp64 recomputation from the tensors the device was given
(oracle/replay.py, the per-launch bound of the opreplay_* cases).  Contract: h is gemm(n, Wpi, bias) bit for bit; qkv differs from
gemm(layernorm(h), Wqkv) only through the order of norm1's fp32 row sums (rel-L2 <= 1.5e-3, the bound tests/opcheck.py sets for
ff_proj_fused_*; measured on MI355X: no element differs on any of these cases); a row's result does not depend on the tile it falls in
or on M.
CPU: the ABI surface, and which launches _Transformer issues with the switch on and off."""
import math
import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
BF = torch.bfloat16
C, HID = 320, 1280
REPLAY_TOL = 5e-4   # tests/modelcheck.py: every fast-precision launch against fp64 on the device's own tensors
BETWEEN_TOL = 1.5e-3  # tests/opcheck.py ff_proj_fused_*: one-launch form against the launches it replaces


def _rnd(shape, g, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).to(BF)


def _rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


class _Switch:
    """ops.<name> = value for the duration of a with block."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        from diffuman4d_amd.host import ops
        self.old = {k: getattr(ops, k) for k in self.kw}
        for k, v in self.kw.items():
            setattr(ops, k, v)

    def __exit__(self, *exc):
        from diffuman4d_amd.host import ops
        for k, v in self.old.items():
            setattr(ops, k, v)
        return False


def _traced(fn):
    """fn() with the operator trace and the launch profile on: (result, trace entries, number of launches)."""
    from diffuman4d_amd.host import ops
    with _Switch(TRACE=[], PROFILE=[]):
        out = fn()
        torch.cuda.synchronize()
        return out, list(ops.TRACE), len(ops.PROFILE)


# ------------------------------------------------------------------------------------------------ head

def _head_inputs(M, seed=0, bias=True, strided=False):
    g = torch.Generator().manual_seed(seed)
    d = "cuda"
    n = _rnd((M, C), g)
    wpi, wqkv = _rnd((C, C), g, 1.0 / math.sqrt(C)), _rnd((3 * C, C), g, 1.0 / math.sqrt(C))
    bpi = _rnd((C,), g, 0.5) if bias else None
    gam, bet = (1.0 + 0.1 * torch.randn(C, generator=g)).to(BF), (0.1 * torch.randn(C, generator=g)).to(BF)
    nd = n.to(d)
    if strided:  # a column view of a wider tensor
        wide = torch.full((M, C + 16), 7.0, dtype=BF, device=d)
        wide[:, 8:8 + C] = nd
        nd = wide[:, 8:8 + C]
    return dict(n=nd, wpi=wpi.to(d), bpi=None if bpi is None else bpi.to(d), ln=(gam.to(d), bet.to(d), 1e-5), wqkv=wqkv.to(d))


def _run_head(inp, qkv=None):
    from diffuman4d_amd.host import ops
    return ops.proj_in_ln_qkv(inp["n"], inp["wpi"], inp["bpi"], inp["ln"], inp["wqkv"], qkv=qkv)


def _check_head(inp, qkv_view=None, qkv_view3=None):
    from oracle import replay
    with _Switch(L0_HEAD_FUSED=True):
        (h, qkv), trace, launches = _traced(lambda: _run_head(inp, qkv_view))
    assert launches == 1, f"the head took {launches} launches: the fused kernel was not used"
    assert [t[0] for t in trace] == ["gemm", "layernorm", "gemm"]
    with _Switch(L0_HEAD_FUSED=False):
        (h3, qkv3), _, launches3 = _traced(lambda: _run_head(inp, qkv_view3))
    assert launches3 == 3
    assert torch.equal(h, h3), f"h differs from gemm(n, Wpi, bias): max abs {float((h.float() - h3.float()).abs().max()):.3e}"
    errs = {"h": replay.replay_gemm(trace[0][1], trace[0][2]), "n1": replay.replay_layernorm(trace[1][1], trace[1][2]),
            "qkv": replay.replay_gemm(trace[2][1], trace[2][2])}
    assert trace[0][2] is h and trace[2][2] is qkv
    between = _rel_l2(qkv, qkv3)
    flips = float((qkv != qkv3).float().mean())
    print(f"head M={h.shape[0]}: fp64 replay {errs}; qkv against the three-launch form: rel-L2 {between:.3e}, {100 * flips:.3f} % of the elements differ")
    for k, e in errs.items():
        assert e <= REPLAY_TOL, f"{k} against fp64: rel-L2 {e:.3e} > {REPLAY_TOL:.0e}"
    assert between <= BETWEEN_TOL, f"qkv against gemm(layernorm(h), Wqkv): rel-L2 {between:.3e}"
    return h, trace[1][2], qkv


@pytest.mark.gpu
@pytest.mark.parametrize("M,bias,seed", [(128, True, 0), (129, True, 1), (300, True, 2), (257, False, 3)])
def test_head_matches_the_three_launches(M, bias, seed):
    _check_head(_head_inputs(M, seed, bias))


@pytest.mark.gpu
def test_head_on_strided_views_leaves_the_other_columns_alone():
    M = 384
    inp = _head_inputs(M, 4, strided=True)
    wide = torch.full((M, 3 * C + 16), 5.0, dtype=BF, device="cuda")
    wide3 = wide.clone()
    _, _, qkv = _check_head(inp, wide[:, 8:8 + 3 * C], wide3[:, 8:8 + 3 * C])
    assert qkv.data_ptr() == wide[:, 8:].data_ptr()
    assert bool((wide[:, :8] == 5.0).all()) and bool((wide[:, 8 + 3 * C:] == 5.0).all()), "columns outside the qkv view were written"


@pytest.mark.gpu
def test_head_rows_do_not_depend_on_their_tile_or_on_M():
    inp = _head_inputs(300, 2)
    first = dict(inp, n=inp["n"][:128])
    with _Switch(L0_HEAD_FUSED=True):
        (h, qkv), trace, _ = _traced(lambda: _run_head(inp))
        (h1, qkv1), trace1, _ = _traced(lambda: _run_head(first))
    assert torch.equal(h[:128], h1) and torch.equal(qkv[:128], qkv1) and torch.equal(trace[1][2][:128], trace1[1][2])


@pytest.mark.gpu
def test_head_falls_back_to_the_separate_launches_for_a_view_it_cannot_take():
    """Every view dm4d_gemm_bf16 accepts has 8-element-aligned strides, hence 16-byte-aligned rows: what such a call can miss of the fused
    launch's guards is the contiguous weight.  A proj_in weight with a row stride of 328 takes gemm, layernorm, gemm -- the same h bits."""
    inp = _head_inputs(257, 5)
    wv = torch.zeros((C, C + 8), dtype=BF, device="cuda")
    wv[:, :C] = inp["wpi"]
    with _Switch(L0_HEAD_FUSED=True):
        (h, qkv), _, launches = _traced(lambda: _run_head(dict(inp, wpi=wv[:, :C])))
        (hf, qkvf), _, launches_f = _traced(lambda: _run_head(inp))
    assert launches == 3 and launches_f == 1
    assert torch.equal(h, hf)
    assert _rel_l2(qkvf, qkv) <= BETWEEN_TOL


# ------------------------------------------------------------------------------------------------ CPU

def test_abi_and_the_launches_a_level0_transformer_issues(monkeypatch):
    """The export is declared in dm4d.h and bound in host/lib.py; _Transformer at C = 320 issues proj_in, norm1, QKV, attention, block tail,
    proj_out with the switch off (today's sequence) and head, attention, block tail, proj_out with it on.  The kernel wrappers are
    tests/cpu_standin_ops.py; the raw head launch is a counted stand-in that restates the three launches it replaces."""
    import cpu_standin_ops as so
    from diffuman4d_amd.host import lib as L, ops, unet

    header = (ROOT / "include" / "dm4d.h").read_text()
    for sym in ("dm4d_proj_in_ln_qkv_fused_bf16", "dm4d_l0_linear_fused_supported"):
        assert re.search(r"\bint\s+" + sym + r"\s*\(", header), f"{sym} is not declared in include/dm4d.h"
        assert sym in L.SIGNATURES, f"{sym} is not bound in diffuman4d_amd/host/lib.py"
    assert L.load().dm4d_l0_linear_fused_supported(320) == 1 and L.load().dm4d_l0_linear_fused_supported(640) == 0

    calls = []

    def counted(name, fn):
        def w(*a, **k):
            calls.append(name)
            return fn(*a, **k)
        return w

    class FF(so.FeedForward):
        def after_attention(self, a, wo, bo, x, ln):
            calls.append("tail")  # one launch: the stand-in's parts inside it are not counted
            return super().after_attention(a, wo, bo, x, ln)

    def head_launch(n, wpi, bpi, ln, wqkv, h, qkv, n1):
        calls.append("head")
        h.copy_(so.gemm(n, wpi, bias=bpi))
        qkv.copy_(so.gemm(so.layernorm(h, ln[0], ln[1], ln[2]), wqkv))

    heads, groups, frames, hw = 5, 32, 2, (4, 3)
    g = torch.Generator().manual_seed(0)
    pfx = "t."
    sd = {pfx + "norm.weight": torch.ones(C), pfx + "norm.bias": torch.zeros(C),
          pfx + "proj_in.weight": _rnd((C, C), g, C ** -0.5), pfx + "proj_in.bias": _rnd((C,), g, 0.1),
          pfx + "proj_out.weight": _rnd((C, C), g, C ** -0.5), pfx + "proj_out.bias": _rnd((C,), g, 0.1)}
    b = pfx + "transformer_blocks.0."
    for nm in ("norm1", "norm3"):
        sd[b + nm + ".weight"], sd[b + nm + ".bias"] = torch.ones(C), torch.zeros(C)
    for nm in ("to_q", "to_k", "to_v", "to_out.0"):
        sd[b + f"attn1.{nm}.weight"] = _rnd((C, C), g, C ** -0.5)
    sd[b + "attn1.to_out.0.bias"] = _rnd((C,), g, 0.1)
    sd[b + "ff.net.0.proj.weight"], sd[b + "ff.net.0.proj.bias"] = _rnd((2 * 64, C), g, C ** -0.5), _rnd((2 * 64,), g, 0.1)
    sd[b + "ff.net.2.weight"], sd[b + "ff.net.2.bias"] = _rnd((C, 64), g, 64 ** -0.5), _rnd((C,), g, 0.1)

    so.install()
    try:
        # set directly, not through monkeypatch: uninstall() below restores the real wrappers it saved at install
        ops.FeedForward = FF
        for name in ("gemm", "layernorm", "attention"):
            setattr(ops, name, counted(name, getattr(so, name)))
        monkeypatch.setattr(ops, "_on_device", lambda t: True)
        monkeypatch.setattr(ops, "_launch_l0_head", head_launch)
        W = unet._Weights(sd, torch.device("cpu"), False, False, BF)
        tr = unet._Transformer(W, pfx, heads, groups)
        x = _rnd((frames, hw[0], hw[1], C), g)
        today = ["gemm", "layernorm", "gemm", "attention", "tail", "gemm"]
        outs = {}
        for head_on, want in ((False, today), (True, ["head", "attention", "tail", "gemm"])):
            monkeypatch.setattr(ops, "L0_HEAD_FUSED", head_on)
            calls.clear()
            outs[head_on] = tr(x, frames)
            assert calls == want, (head_on, calls)
        # the stand-ins restate the same arithmetic: the wiring hands every launch the same tensors
        assert outs[True].shape == x.shape and torch.equal(outs[True], outs[False])
    finally:
        so.uninstall()
