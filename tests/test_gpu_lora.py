"""sp_lora_shrink / sp_lora_expand on the GPU against tests/lora_oracle.py (the operation's statement in fp64 on the
same stored 16-bit inputs), under the derived error model stated there - no element may fall outside it.

Shapes: T in {1, 7, 17, 33} (one row, a partial block, a block boundary, blocks with a tail; blocks are 4 rows),
K in {64, 200, 4096} (one k-round, K not divisible by the thread groups, the real width), r in {8, 16, 64},
S in {1, 2, 3}, n in {8, 24, 1024}, 3 slots, both dtypes, padded x / y / tmp strides, y and tmp at a column offset."""
import pytest
import torch

from tests import lora_oracle as lo

pytestmark = pytest.mark.gpu

SLOTS = 3
DT = {"bf16": torch.bfloat16, "f16": torch.float16}


def pattern(name, T):
    if name == "one":
        v = [1] * T
    elif name == "none":
        v = [-1] * T
    elif name == "sorted":
        v = sorted([-1, 0, 1, 2] * (T // 4 + 1))[:T]
    elif name == "interleaved":
        v = [(2, -1, 0, 1, 1, 0, 2)[i % 7] for i in range(T)]
    elif name == "straddle":          # a run of adapter 1 over rows 3 .. 8: across the 4-row block boundaries
        v = [0 if i < 3 else 1 if i < 9 else 2 for i in range(T)]
    elif name == "out_of_range":      # one index == num_slots: skipped like -1
        v = [(0, 1, 2)[i % 3] for i in range(T)]
        v[T // 2] = SLOTS
    else:
        raise ValueError(name)
    return torch.tensor(v, dtype=torch.int32)


class Problem:
    """inputs on the device in padded buffers; y and tmp are column views at an offset"""

    def __init__(self, T, K, r, S, n, pat, dtype, seed=0):
        g = torch.Generator().manual_seed(1000 * seed + T + K + r + S + n)
        self.T, self.K, self.r, self.S, self.n, self.dtype = T, K, r, S, n, dtype
        self.scale = 2.0
        R, N = S * r, S * n
        self.idx = pattern(pat, T).cuda()
        xb = torch.randn(T, K + 8, generator=g).to(dtype).cuda()
        self.x = xb[:, :K]
        self.A = (torch.randn(SLOTS, K, R, generator=g) * 0.1).to(dtype).cuda()
        self.B = (torch.randn(SLOTS, r, N, generator=g) * 0.1).to(dtype).cuda()
        self.ybuf = torch.randn(T, N + 24, generator=g).to(dtype).cuda()
        self.y = self.ybuf[:, 8:8 + N]
        self.tbuf = torch.full((T, R + 12), 123.25, dtype=torch.float32).cuda()
        self.tmp = self.tbuf[:, 4:4 + R]


def bits(t):
    return t.contiguous().view(torch.int16) if t.element_size() == 2 else t.contiguous().view(torch.int32)


def run_and_check(p: Problem):
    from scratchpad_amd import _native
    y_old, ybuf_old, tbuf_old = p.y.clone(), p.ybuf.clone(), p.tbuf.clone()
    before = dict(_native.LORA_CALLS)
    out = _native.lora_shrink(p.x, p.A, p.idx, p.scale, out=p.tmp)
    assert out.data_ptr() == p.tmp.data_ptr()
    _native.lora_expand(p.y, p.tmp, p.B, p.idx, p.S)
    torch.cuda.synchronize()
    assert _native.LORA_CALLS["shrink"] == before["shrink"] + 1 and _native.LORA_CALLS["expand"] == before["expand"] + 1
    live = lo.live_rows(p.idx, SLOTS)
    tmp64, tab = lo.shrink(p.x, p.A, p.idx.cpu(), p.scale)
    y64, yab = lo.expand(y_old, tmp64, tab, p.B, p.idx.cpu(), p.S)
    got_t, got_y = p.tmp.cpu().double(), p.y.cpu().double()
    # tmp alone
    err_t = (got_t - tmp64).abs()[live]
    bnd_t = lo.tmp_bound(tab, p.K)[live]
    worst_t = float((err_t / bnd_t.clamp_min(1e-300)).max()) if err_t.numel() else 0.0
    # y of the stacked operation
    err_y = (got_y - y64).abs()[live]
    bnd_y = lo.y_bound(y64, yab, p.K, p.r, p.dtype)[live]
    worst_y = float((err_y / bnd_y).max()) if err_y.numel() else 0.0
    print(f"[lora] T {p.T} K {p.K} r {p.r} S {p.S} n {p.n} {p.dtype}: max err/bound tmp {worst_t:.3f} y {worst_y:.3f}")
    assert bool((err_t <= bnd_t).all()), f"tmp: {int((err_t > bnd_t).sum())} elements outside the error model"
    assert bool((err_y <= bnd_y).all()), f"y: {int((err_y > bnd_y).sum())} elements outside the error model"
    # skipped rows (-1 or out of range): bit-identical y and tmp; everything outside the written columns too
    dead = ~live
    assert torch.equal(bits(p.y.cpu())[dead], bits(y_old.cpu())[dead])
    assert torch.equal(bits(p.tmp.cpu())[dead], bits(tbuf_old[:, 4:4 + p.S * p.r].cpu())[dead])
    N, R = p.S * p.n, p.S * p.r
    for lo_c, hi_c in ((0, 8), (8 + N, N + 24)):
        assert torch.equal(bits(p.ybuf[:, lo_c:hi_c].cpu()), bits(ybuf_old[:, lo_c:hi_c].cpu())), "y padding touched"
    for lo_c, hi_c in ((0, 4), (4 + R, R + 12)):
        assert torch.equal(bits(p.tbuf[:, lo_c:hi_c].cpu()), bits(tbuf_old[:, lo_c:hi_c].cpu())), "tmp padding touched"
    return p


# every value of every dimension, and every index pattern, at least once; the full product would say nothing more
CASES = [
    (1, 64, 8, 1, 8, "one"),
    (7, 200, 16, 2, 24, "sorted"),
    (17, 4096, 16, 3, 24, "straddle"),
    (33, 4096, 16, 1, 1024, "interleaved"),
    (33, 200, 64, 3, 24, "out_of_range"),
    (17, 64, 64, 2, 1024, "interleaved"),
    (33, 64, 8, 3, 8, "straddle"),
    (7, 4096, 64, 1, 8, "none"),
    (17, 200, 8, 2, 24, "one"),
    (33, 4096, 16, 2, 1024, "sorted"),
]


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "T{}-K{}-r{}-S{}-n{}-{}".format(*c))
def test_shrink_then_expand_within_the_error_model(case, dt):
    run_and_check(Problem(*case, DT[dt]))


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_expand_alone_from_given_tmp(dt):
    """expand on an fp32 tmp that is GIVEN (no shrink): the error model with tmp exact, i.e. K = 0"""
    from scratchpad_amd import _native
    p = Problem(17, 64, 16, 2, 24, "interleaved", DT[dt], seed=3)
    g = torch.Generator().manual_seed(5)
    p.tmp.copy_(torch.randn(p.T, p.S * p.r, generator=g))
    y_old = p.y.clone()
    _native.lora_expand(p.y, p.tmp, p.B, p.idx, p.S)
    torch.cuda.synchronize()
    live = lo.live_rows(p.idx, SLOTS)
    t64 = p.tmp.cpu().double()
    y64, yab = lo.expand(y_old, t64, t64.abs(), p.B, p.idx.cpu(), p.S)
    err = (p.y.cpu().double() - y64).abs()
    assert bool((err <= lo.y_bound(y64, yab, 0, p.r, p.dtype))[live].all())
    assert torch.equal(bits(p.y.cpu())[~live], bits(y_old.cpu())[~live])


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_batch_invariance_row_alone_equals_row_in_batch(dt):
    """each row of the T = 33 interleaved case run alone (T = 1): the same bits as in the batch"""
    from scratchpad_amd import _native
    p = Problem(33, 4096, 16, 3, 24, "interleaved", DT[dt], seed=7)
    y_old = p.y.clone()
    _native.lora_shrink(p.x, p.A, p.idx, p.scale, out=p.tmp)
    _native.lora_expand(p.y, p.tmp, p.B, p.idx, p.S)
    for t in range(p.T):
        x1 = p.x[t:t + 1].clone()
        y1 = y_old[t:t + 1].clone()
        i1 = p.idx[t:t + 1].clone()
        t1 = torch.full((1, p.S * p.r), 123.25, dtype=torch.float32, device="cuda")
        _native.lora_shrink(x1, p.A, i1, p.scale, out=t1)
        _native.lora_expand(y1, t1, p.B, i1, p.S)
        assert torch.equal(bits(t1.cpu()), bits(p.tmp[t:t + 1].cpu())), f"row {t}: tmp bits differ"
        assert torch.equal(bits(y1.cpu()), bits(p.y[t:t + 1].cpu())), f"row {t}: y bits differ"


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_qkv_one_shrink_two_expands_equals_the_stacked_operation(dt):
    """[q|k|v]-shaped y: one shrink (R = 3 r), expand of q (S = 1) and of kv (S = 2, tmp offset by r) against the
    oracle of the stacked operation with B = [B_q | B_kv]"""
    from scratchpad_amd import _native
    dtype = DT[dt]
    g = torch.Generator().manual_seed(11)
    T, K, r, nq, nkv = 17, 200, 16, 48, 24
    idx = pattern("interleaved", T).cuda()
    x = torch.randn(T, K, generator=g).to(dtype).cuda()
    A = (torch.randn(SLOTS, K, 3 * r, generator=g) * 0.1).to(dtype).cuda()
    Bq = (torch.randn(SLOTS, r, nq, generator=g) * 0.1).to(dtype).cuda()
    Bkv = (torch.randn(SLOTS, r, 2 * nkv, generator=g) * 0.1).to(dtype).cuda()
    y = torch.randn(T, nq + 2 * nkv, generator=g).to(dtype).cuda()
    y_old = y.clone()
    tmp = _native.lora_shrink(x, A, idx, 0.5)
    _native.lora_expand(y[:, :nq], tmp[:, :r], Bq, idx, 1)
    _native.lora_expand(y[:, nq:], tmp[:, r:], Bkv, idx, 2)
    torch.cuda.synchronize()
    live = lo.live_rows(idx, SLOTS)
    t64, tab = lo.shrink(x, A, idx.cpu(), 0.5)
    yq, yqa = lo.expand(y_old[:, :nq], t64[:, :r], tab[:, :r], Bq, idx.cpu(), 1)
    ykv, ykva = lo.expand(y_old[:, nq:], t64[:, r:], tab[:, r:], Bkv, idx.cpu(), 2)
    y64, yab = torch.cat((yq, ykv), 1), torch.cat((yqa, ykva), 1)
    err = (y.cpu().double() - y64).abs()
    assert bool((err <= lo.y_bound(y64, yab, K, r, dtype))[live].all())
    assert torch.equal(bits(y.cpu())[~live], bits(y_old.cpu())[~live])
