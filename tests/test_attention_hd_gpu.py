"""GPU: the head-dimension 40 / 80 / 160 attention kernels (attention_hd.hip) against an fp64 softmax attention on the same numbers, in
the three operand forms (bf16 and fp16 with a pre-scaled Q, two-term bf16 "split" for the parity precision).  Bounds are the ones
tests/opcheck.py applies to the head-dimension 64 kernel of the same precision (TOL, TOL_H16_ATTN, TOL_PAR_ATTN)."""
import pytest
import torch

import opcheck as oc

pytestmark = pytest.mark.gpu
BF, F16 = torch.bfloat16, torch.float16
HEADS = 8
BOUND = {"bf16": oc.TOL, "f16": oc.TOL_H16_ATTN, "split": oc.TOL_PAR_ATTN}
LN2 = 0.6931471805599453


def _operands(mode, d, batch, Lq, Lk, seed, spike=False, ramp=False):
    """Q [batch*Lq, C] and K | V [batch*Lk, 2C] on the CPU as fp64 VALUES plus what the kernel is given: Q / K / V as column slices of one
    [M, 3C] tensor when Lq == Lk (the fused QKV output), else Q alone and K | V of one [M, 2C] tensor (the frame-shard gather).
    split: each value is hi + lo of two bf16 planes.  bf16 / f16: Q carries d^-0.5 log2 e."""
    from diffuman4d_amd.host import ops
    g = torch.Generator().manual_seed(seed)
    C = HEADS * d
    q = torch.randn(batch * Lq, C, generator=g)
    kv = torch.randn(batch * Lk, 2 * C, generator=g)
    kk = kv[:, :C].view(batch, Lk, C)
    if spike or ramp:  # a direction every query shares, so that chosen keys score high in every row
        u = torch.randn(C, generator=g)
        q += u
    if spike:  # one late key dominates every row
        kk[:, Lk - 3] += 3.0 * u
    if ramp:  # keys far above anything in the first tile, late in the sequence, and scores that keep growing with the key index
        kk[:, min(100, Lk - 1)] *= 16.0
        kk[:, max(Lk - 70, 0)] *= 12.0
        kk += torch.linspace(0, 3, Lk).view(1, Lk, 1) * u
    if mode != "split":
        dt = F16 if mode == "f16" else BF
        qd = (q * (d ** -0.5 * ops.LOG2E)).to(dt)
        kvd = kv.to(dt)
        return dict(q=qd.double(), kv=kvd.double(), scale=LN2), [qd, kvd]
    planes = []
    vals = []
    for x in (q, kv):
        hi = x.to(BF)
        lo = (x - hi.float()).to(BF)
        planes.append((hi, lo))
        vals.append(hi.double() + lo.double())
    return dict(q=vals[0], kv=vals[1], scale=d ** -0.5), planes


def _reference(val, batch, d, Lq, Lk, rows=None):
    C = HEADS * d
    q = val["q"].view(batch, Lq, HEADS, d).transpose(1, 2)
    k = val["kv"][:, :C].reshape(batch, Lk, HEADS, d).transpose(1, 2)
    v = val["kv"][:, C:].reshape(batch, Lk, HEADS, d).transpose(1, 2)
    if rows is not None:
        q = q[:, :, rows]
    o = torch.softmax(q @ k.transpose(-1, -2) * val["scale"], dim=-1) @ v
    return o.transpose(1, 2).reshape(batch, -1, C)


def _launch(mode, d, batch, Lq, Lk, dev, pad_o=0):
    """Run the kernel on the device tensors `dev`; O lives in a wider tensor (row stride C + 2 pad_o) prefilled with a sentinel, at
    column offset pad_o.  Returns (O view, the whole O tensor)."""
    from diffuman4d_amd.host import lib as L
    from diffuman4d_amd.host import ops
    C = HEADS * d
    lib = L.load()
    st = torch.cuda.current_stream().cuda_stream
    fused = Lq == Lk
    if mode != "split":
        qd, kvd = (t.cuda() for t in dev)
        if fused:  # [M, 3C] = [q | k | v]
            buf = torch.cat([qd, kvd], dim=1)
            q, k, v = buf[:, :C], buf[:, C:2 * C], buf[:, 2 * C:]
        else:
            q, k, v = qd, kvd[:, :C], kvd[:, C:]
        full = torch.full((batch * Lq, C + 2 * pad_o), -512.0, dtype=qd.dtype, device="cuda")
        out = full[:, pad_o:pad_o + C]
        ops.attention(q, k, v, batch, HEADS, Lq, out=out, kv_seq=Lk, q_scaled=True)
        return out, full
    (qh, ql), (kh, kl) = dev
    if fused:  # gemm(split_out=True) planes of a fused QKV: [q_hi | k_hi | v_hi | q_lo | k_lo | v_lo]
        buf = torch.cat([qh, kh, ql, kl], dim=1).cuda()
        qp, kp, vp, ld = buf.data_ptr(), buf.data_ptr() + 2 * C, buf.data_ptr() + 4 * C, buf.stride(0)
        ldq = ldk = ldv = ld
        q_lo = k_lo = v_lo = 3 * C
        keep = buf
    else:  # q [q_hi | q_lo], kv [k_hi | v_hi | k_lo | v_lo]
        qb, kvb = torch.cat([qh, ql], dim=1).cuda(), torch.cat([kh, kl], dim=1).cuda()
        qp, kp, vp = qb.data_ptr(), kvb.data_ptr(), kvb.data_ptr() + 2 * C
        ldq, ldk, ldv = qb.stride(0), kvb.stride(0), kvb.stride(0)
        q_lo, k_lo, v_lo = C, 2 * C, 2 * C
        keep = (qb, kvb)
    full = torch.full((batch * Lq, 2 * C + 2 * pad_o), -512.0, dtype=BF, device="cuda")
    out = full[:, pad_o:pad_o + 2 * C]
    rc = lib.dm4d_attention_hd_split_bf16(st, qp, kp, vp, out.data_ptr(), ldq, ldk, ldv, out.stride(0), q_lo, k_lo, v_lo, C, batch, HEADS,
                                          Lq, Lk, d ** -0.5, d)
    L.check(rc, "dm4d_attention_hd_split_bf16")
    del keep
    return out, full


def _value(mode, out):
    return oc._join(out) if mode == "split" else out.double().cpu()


MODES = ["bf16", "f16", "split"]
# (d, batch, Lq, Lk): the judged window calls' token counts (F = 16 / 24 at 72 x 40; 3-D attention sees F x HW tokens per sequence:
# 11 520 / 17 280 at 320 channels, 2 880 / 4 320 at 640, 720 / 1 080 at 1 280), ragged lengths, and Lk = 4 Lq
JUDGED = [(40, 1, 11520, 11520), (40, 1, 17280, 17280), (80, 1, 2880, 2880), (80, 1, 4320, 4320), (160, 2, 720, 720), (160, 2, 1080, 1080)]
RAGGED = [(d, 1, L, L) for d in (40, 80, 160) for L in (1080, 721, 65, 1)] + [(d, 2, 300, 1200) for d in (40, 80, 160)]


def _check(mode, d, batch, Lq, Lk, seed=0, spike=False, ramp=False, pad_o=0):
    val, dev = _operands(mode, d, batch, Lq, Lk, seed, spike, ramp)
    out, full = _launch(mode, d, batch, Lq, Lk, dev, pad_o)
    torch.cuda.synchronize()
    rows = None
    if Lq > 1024:  # the fp64 reference on a sample of query rows (all keys): first and last tiles, and a spread
        rows = torch.unique(torch.cat([torch.arange(300), torch.arange(Lq - 300, Lq), torch.randperm(Lq, generator=torch.Generator().manual_seed(1))[:300]]))
    ref = _reference(val, batch, d, Lq, Lk, rows)
    got = _value(mode, out).view(batch, Lq, -1)
    if rows is not None:
        got = got[:, rows]
    e = oc.rel_l2(got, ref)
    assert torch.isfinite(got).all()
    assert e <= BOUND[mode], f"{mode} d={d} batch={batch} Lq={Lq} Lk={Lk} spike={spike} ramp={ramp}: rel-L2 {e:.3e} > {BOUND[mode]:.0e}"
    if pad_o:
        f = full.float()
        assert (f[:, :pad_o] == -512.0).all() and (f[:, full.shape[1] - pad_o:] == -512.0).all(), "O store left its columns"
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", JUDGED, ids=lambda s: "d%d_b%d_L%d" % s[:3])
def test_judged_token_counts(hip_device, mode, shape):
    _check(mode, *shape)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", RAGGED, ids=lambda s: "d%d_b%d_Lq%d_Lk%d" % s)
def test_ragged_and_longer_keys(hip_device, mode, shape):
    _check(mode, *shape, pad_o=8)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d", [40, 80, 160])
@pytest.mark.parametrize("kind", ["spike", "ramp"])
def test_spike_and_ramp_rows(hip_device, mode, d, kind):
    _check(mode, d, 2, 777, 777, seed=3, spike=kind == "spike", ramp=kind == "ramp")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d", [40, 80, 160])
def test_repeatable_and_shard_invariant(hip_device, mode, d):
    """Two launches are bitwise equal, and each of 3 ranks' 360 queries (not a multiple of a workgroup's 256 rows) against all 1 080 keys
    equals the same rows of the unsharded run bitwise."""
    batch, L, parts = 2, 1080, 3
    val, dev = _operands(mode, d, batch, L, L, 5)
    a, _ = _launch(mode, d, batch, L, L, dev)
    b, _ = _launch(mode, d, batch, L, L, dev)
    assert torch.equal(a, b)
    ls = L // parts
    C = HEADS * d
    full = a.view(batch, L, -1)
    for r in range(parts):
        sl = slice(r * ls, (r + 1) * ls)
        if mode == "split":
            (qh, ql), kvp = dev
            sub = [(qh.view(batch, L, C)[:, sl].reshape(batch * ls, C), ql.view(batch, L, C)[:, sl].reshape(batch * ls, C)), kvp]
        else:
            sub = [dev[0].view(batch, L, C)[:, sl].reshape(batch * ls, C), dev[1]]
        o, _ = _launch(mode, d, batch, ls, L, sub)
        assert torch.equal(o.view(batch, ls, -1), full[:, sl]), f"rank {r} of {parts}"
