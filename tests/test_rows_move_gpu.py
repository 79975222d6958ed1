"""GPU: ops.rows_move (dm4d_rows_move) against index_select / index_copy_, and ops.pack_model_input with a row subset against the rows
of the full result."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


def job(n_src, n_dst, row_elems, src_idx, dst_idx, dtype=torch.bfloat16, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    src = torch.randn(n_src, row_elems, generator=g, device="cuda").to(dtype)
    dst = torch.randn(n_dst, row_elems, generator=g, device="cuda").to(dtype)
    want = dst.clone()
    if len(src_idx):
        want.index_copy_(0, torch.tensor(dst_idx, device="cuda"), src.index_select(0, torch.tensor(src_idx, device="cuda")))
    return (src, dst, i32(src_idx), i32(dst_idx)), want


def run(jobs):
    from diffuman4d_amd.host import ops
    ops.rows_move([j for j, _ in jobs])
    torch.cuda.synchronize()
    for k, ((_, dst, _, _), want) in enumerate(jobs):
        assert torch.equal(dst, want), f"job {k}"


def test_one_row_of_16_bytes():
    run([job(1, 1, 8, [0], [0])])


def test_three_rows_of_640_bytes_permuted():
    run([job(5, 4, 320, [4, 0, 2], [1, 3, 0])])


def test_five_jobs_with_different_row_sizes_and_an_empty_one():
    # 16 B, 640 B, an empty job, fp32 rows of 16 400 B (past one 16 KB workgroup step, ragged), 3 x 1 843 200 B (a level-0 row at 72 x 40)
    run([job(3, 3, 8, [2, 1], [0, 2], seed=1), job(6, 7, 320, [5, 1, 3, 0], [6, 0, 2, 4], seed=2), job(2, 2, 64, [], [], seed=3),
         job(4, 3, 4100, [3, 0], [2, 1], dtype=torch.float32, seed=4), job(3, 5, 2880 * 320, [2, 0, 1], [4, 1, 3], seed=5)])


def test_a_source_row_used_twice_and_sixteen_jobs():
    from diffuman4d_amd.host import lib as L, ops
    run([job(3, 4, 320, [1, 1, 2], [0, 3, 1])])
    run([job(4, 4, 40 * (k + 1), [k % 4, 3], [0, 1 + k % 3], seed=k) for k in range(16)])
    with pytest.raises(L.Dm4dError, match="jobs"):
        ops.rows_move([job(1, 1, 8, [0], [0])[0]] * 17)
    with pytest.raises(L.Dm4dError, match="differ in size"):
        ops.rows_move([(torch.zeros(2, 8, device="cuda"), torch.zeros(2, 16, device="cuda"), i32([0]), i32([0]))])


@pytest.mark.parametrize("wide,h16", [(False, False), (True, False), (True, True)])
def test_pack_for_a_row_subset_writes_those_rows_and_aliases_every_cond_frame(wide, h16):
    from diffuman4d_amd.host import ops
    F, N, HW, cpad = 5, 9, 37, 32
    dt = torch.float32 if wide else torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(7)
    rnd = lambda c: torch.randn(N, HW, c, generator=g, device="cuda").to(torch.bfloat16).to(dt)  # noqa: E731
    lat, pv, pl, sk, m = rnd(4), rnd(4), rnd(6), rnd(4), rnd(1)
    widx, cond = i32([7, 2, 0, 5, 3]), i32([1, 1, 0, 0, 0])
    lat_full = lat.clone()
    full = ops.pack_model_input(lat_full, pv, pl, sk, m, cond, cpad, True, frame_idx=widx, h16=h16)
    out_row = [-1, 1, 2, -1, 0]  # frames 4, 1, 2 -> compact rows 0, 1, 2; frame 0 (conditioning) and frame 3 are left out
    lat_sub = lat.clone()
    sub = ops.pack_model_input(lat_sub, pv, pl, sk, m, cond, cpad, True, frame_idx=widx, h16=h16, out_row=i32(out_row), rows=3)
    torch.cuda.synchronize()
    assert sub.shape == (6,) + tuple(full.shape[1:]) and sub.dtype == full.dtype
    for f, r in enumerate(out_row):
        if r >= 0:
            assert torch.equal(sub[r], full[f]) and torch.equal(sub[3 + r], full[F + f])
    assert torch.equal(lat_sub, lat_full) and torch.equal(lat_sub[7], pv[7]) and not torch.equal(lat[7], pv[7])
