"""sp_embedding_pool on the device: the norm step bit for bit against sp_fused_add_rmsnorm / sp_rmsnorm
over all rows, the L2 step inside the oracle's interval and bit-equal wherever that interval is a point
(tests/embedding_oracle.py; the share of other elements is asserted below 5 % for the 16-bit types here, on the rows
the kernel normalises, and rehearsed on the host in tests/test_embedding_oracle.py on the same seeded inputs with the
statement's norm step in the kernel's place), read-only inputs, batch invariance, the range check, and the rows of the reference's own Pooler.

Shapes: hidden 7 and 100 (element path), 4096 (16-byte path), 4104 (16-byte path with a ragged last iteration), 12288
(beyond the registers of the 16-byte path: the element path at a large width); 1, 3 and 70 sequences; ragged lengths
that contain 1; int32 and int64 lengths; row strides with spare elements."""
import pytest
import torch

from tests import embedding_cases as cases
from tests import embedding_oracle as eo

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
EPS = 1e-5


def strided(t, spare, dev):
    """t [R, H] on the device as a view with `spare` unused elements behind every row"""
    buf = torch.full((t.shape[0], t.shape[1] + spare), 7.0, dtype=t.dtype, device=dev)
    buf[:, : t.shape[1]] = t.to(dev)
    return buf[:, : t.shape[1]]


def make(H, B, dtype, spare, idx64, dev="cuda"):
    x, res, w, lens = cases.pool_inputs(H, B, dtype)
    x, res, w = strided(x, spare, dev), strided(res, spare, dev), w.to(dev)
    lens_t = torch.tensor(lens, dtype=torch.int64 if idx64 else torch.int32, device=dev)
    rows = (torch.cumsum(lens_t.long(), 0) - 1)
    return x, res, w, lens_t, rows


def check_l2(got, n):
    """got = the kernel's normalised rows of n (both on the device, n in its dtype)"""
    lo, hi = eo.l2_interval(n.cpu())
    got = got.cpu()
    ok = eo.inside(got, lo, hi)
    assert bool(ok.all()), f"{int((~ok).sum())} elements outside the oracle's interval"
    point = eo.is_point(lo, hi)
    assert bool(eo.same_bits(got, lo)[point].all()), "bit-equal wherever the interval is a point"
    return float((~point).float().mean())


@pytest.mark.parametrize("B", [1, 3, 70])
@pytest.mark.parametrize("H", [7, 100, 4096, 4104, 12288])
@pytest.mark.parametrize("dtype", DTYPES)
def test_norm_step_bit_for_bit_and_l2_step_inside_the_interval(dtype, H, B):
    from scratchpad_amd import _native
    idx64 = (H + B) % 2 == 0
    spare = 8 if H % 8 == 0 else 3
    x, res, w, lens, rows = make(H, B, dtype, spare, idx64)
    x0, r0 = x.clone(), res.clone()
    # the parent's path: the norm over ALL rows (in place on copies), then the gather
    xa, ra = strided(x.cpu(), spare, "cuda"), strided(res.cpu(), spare, "cuda")
    _native.fused_add_rmsnorm(xa, ra, w, EPS)
    want_fused = xa[rows]
    want_plain = _native.rmsnorm(x, w, EPS)[rows]
    got_fused = _native.embedding_pool(x, lens, normalize=False, residual=res, weight=w, eps=EPS)
    got_plain = _native.embedding_pool(x, lens, normalize=False, weight=w, eps=EPS)
    got_gather = _native.embedding_pool(x, lens, normalize=False)
    assert got_fused.dtype == dtype and got_fused.shape == (B, H)
    assert torch.equal(got_fused, want_fused), "fused-add form differs from sp_fused_add_rmsnorm over all rows"
    assert torch.equal(got_plain, want_plain), "plain form differs from sp_rmsnorm over all rows"
    assert torch.equal(got_gather, x[rows])
    share = max(check_l2(_native.embedding_pool(x, lens, True, residual=res, weight=w, eps=EPS), want_fused),
                check_l2(_native.embedding_pool(x, lens, True, weight=w, eps=EPS), want_plain),
                check_l2(_native.embedding_pool(x, lens, True), x[rows]))
    print(f"{dtype} H={H} B={B}: largest non-point share {share:.4f}")
    # fp32 is exempt: the last bit of the fp32 sum already moves every fp32 quotient, so no bound that allows more than
    # one summation order leaves a point interval; fp32 is held to the few-ulp interval that check_l2 asserted above
    if dtype != torch.float32:
        assert share < 0.05
    assert torch.equal(x, x0) and torch.equal(res, r0), "x and residual are read only"
    assert bool((x.as_strided((x.shape[0], spare), (H + spare, 1), H) == 7).all()), "the spare elements are untouched"


@pytest.mark.parametrize("dtype", DTYPES)
def test_strides_that_break_the_16_byte_path(dtype):
    """H = 4096 with 3 spare elements per row: the all-rows norm takes its element path, and so must the pool"""
    from scratchpad_amd import _native
    x, res, w, lens, rows = make(4096, 3, dtype, 3, False)
    xa, ra = strided(x.cpu(), 3, "cuda"), strided(res.cpu(), 3, "cuda")
    _native.fused_add_rmsnorm(xa, ra, w, EPS)
    out = torch.full((3, 4096 + 5), 9.0, dtype=dtype, device="cuda")[:, :4096]       # a spare-element out as well
    _native.embedding_pool(x, lens, normalize=False, residual=res, weight=w, eps=EPS, out=out)
    assert torch.equal(out, xa[rows])
    # an aligned x with a misaligned out: the sums keep the 16-byte path's order, the stores go element by element
    x2, res2, w2, lens2, rows2 = make(4096, 3, dtype, 8, False)
    xb, rb = strided(x2.cpu(), 8, "cuda"), strided(res2.cpu(), 8, "cuda")
    _native.fused_add_rmsnorm(xb, rb, w2, EPS)
    _native.embedding_pool(x2, lens2, normalize=False, residual=res2, weight=w2, eps=EPS, out=out)
    assert torch.equal(out, xb[rows2])
    assert bool((out.as_strided((3, 5), (4101, 1), 4096) == 9).all())


@pytest.mark.parametrize("H", [100, 4096, 12288])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_a_sequence_does_not_see_its_batch(dtype, H):
    """alone, as sequence 37 of 70, and with the other sequences permuted: identical bits"""
    from scratchpad_amd import _native
    spare = 8 if H % 8 == 0 else 3
    x, res, w, lens, rows = make(H, 70, dtype, spare, False)
    full = _native.embedding_pool(x, lens, True, residual=res, weight=w, eps=EPS)
    r = int(rows[37])
    n = int(lens[37])
    one = torch.tensor([n], dtype=torch.int32, device="cuda")
    alone = _native.embedding_pool(x[r - n + 1: r + 1], one, True, residual=res[r - n + 1: r + 1], weight=w, eps=EPS)
    assert torch.equal(alone[0], full[37])
    # the batch with its sequences in another order (37 moves to the front)
    order = [37] + [i for i in reversed(range(70)) if i != 37]
    starts = (rows - lens.long() + 1).tolist()
    idx = torch.cat([torch.arange(starts[i], starts[i] + int(lens[i])) for i in order]).cuda()
    xp, rp = strided(x[idx].cpu(), spare, "cuda"), strided(res[idx].cpu(), spare, "cuda")     # the same row layout
    perm = _native.embedding_pool(xp, lens[order], True, residual=rp, weight=w, eps=EPS)
    assert torch.equal(perm[0], full[37]) and torch.equal(perm[1:], full[[i for i in order[1:]]])


@pytest.mark.parametrize("idx64", [False, True])
@pytest.mark.parametrize("H", [100, 4096])
def test_lengths_out_of_range_give_zero_rows(H, idx64):
    """a zero length, and lengths that overrun num_tokens: zero rows, no address formed, neighbours untouched"""
    from scratchpad_amd import _native
    dtype = torch.bfloat16
    g = torch.Generator().manual_seed(5)
    T = 10
    x = torch.randn(T, H, generator=g).to(dtype).cuda()
    res = torch.randn(T, H, generator=g).to(dtype).cuda()
    w = torch.ones(H, dtype=dtype, device="cuda")
    it = torch.int64 if idx64 else torch.int32
    lens = torch.tensor([3, 0, 2, 4, 1, 6, 2], dtype=it, device="cuda")          # rows 2, (4), 4, 8, 9, 15, 17
    good = torch.tensor([3, 2, 4, 1], dtype=it, device="cuda")
    want = _native.embedding_pool(x, good, True, residual=res, weight=w, eps=EPS)
    out = torch.full((7, H), 5.0, dtype=dtype, device="cuda")
    _native.embedding_pool(x, lens, True, residual=res, weight=w, eps=EPS, out=out)
    assert torch.equal(out[[0, 2, 3, 4]], want), "the neighbours of a refused row are what they are without it"
    assert bool((out[[1, 5, 6]] == 0).all()), "refused rows are written as zeros"
    first = torch.tensor([0, 2], dtype=it, device="cuda")                          # row -1, then row 1
    out2 = _native.embedding_pool(x, first, False)
    assert bool((out2[0] == 0).all()) and torch.equal(out2[1], x[1])
    huge = torch.tensor([2 ** 31 - 1, 2 ** 31 - 1, 3], dtype=it, device="cuda")    # the int64 sum, not an int32 wrap
    out3 = _native.embedding_pool(x, huge, False)
    assert bool((out3 == 0).all())


@pytest.mark.parametrize("H", [100, 256])
@pytest.mark.parametrize("name", ["bf16", "fp16", "fp32"])
def test_reference_pooler_rows(H, name):
    """Pooler(LAST, normalize=True) of the reference, the zero row and the fp16 overflow row included"""
    from scratchpad_amd import _native
    x, lens, want = cases.pooler_case(H, name)
    got = _native.embedding_pool(x.cuda(), lens.cuda(), True).cpu()
    rows = eo.last_rows(lens, x.shape[0])
    lo, hi = eo.l2_interval(x[rows])
    assert bool(eo.inside(got, lo, hi).all())
    # the reference summed in an order of its own: its bits are owed wherever no order can move them
    lo2, hi2 = eo.l2_interval(x[rows], any_order=True)
    point = eo.is_point(lo2, hi2)
    assert bool(eo.inside(want, lo2, hi2).all()) and bool(eo.same_bits(got, want)[point].all())
    assert float(point[[1, 2]].float().mean()) == 1.0 or name == "fp32", "the zero and the overflow row are pinned"
    assert torch.allclose(got.float(), want.float(), rtol=2.0 ** -7 if name != "fp32" else 1e-6, atol=0, equal_nan=True)
    assert bool(eo.same_bits(got[1], want[1]).all()) and bool(eo.same_bits(got[2], want[2]).all())


def test_wrapper_refusals():
    from scratchpad_amd import _native
    x = torch.zeros(4, 64, device="cuda")
    lens = torch.tensor([4], dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _native.embedding_pool(x.cpu(), lens.cpu())
    with pytest.raises(RuntimeError, match="residual goes with a norm weight"):
        _native.embedding_pool(x, lens, residual=x.clone())
    with pytest.raises(RuntimeError, match="int32 / int64"):
        _native.embedding_pool(x, lens.float())
    assert _native.embedding_pool(x, lens[:0]).shape == (0, 64)
