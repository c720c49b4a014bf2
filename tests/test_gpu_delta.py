"""sp_delta_group and sp_delta_mm on the GPU against tests/delta_oracle.py (fp64 on the stored values; the error bound
and its derivation are in that module's header).

Shapes: K in {64, 320, 4160} (one super-step with a single live lane group, a full super-step plus a tail, 17
super-steps over the 8 waves), N in {16, 48} (a second 16-row block), T in {1, 17, 70} (70 rows of which 35 name slot
0: a second row block of one slot), 3 slots interleaved with base-model rows (-1) and rows whose index is past the
slots.  x and y are column views of wider tensors, so both strides differ from the widths."""
import pytest
import torch

from tests import delta_oracle

pytestmark = pytest.mark.gpu

SLOTS = 3
PATTERN = [0, 1, 0, 2, 0, -1, 0, 3]          # 3 >= SLOTS: skipped like -1
SENTINEL = 0x3C5A                             # the bits skipped rows of y are pre-filled with
DTYPES = [torch.float16, torch.bfloat16]
_cache = {}


def indices_for(T):
    return torch.tensor([PATTERN[t % len(PATTERN)] for t in range(T)], dtype=torch.int32)


def packed_slots(N, K, dtype):
    """(codes [S, N, K/4], meta [S, N, K/8], scales [S, N]) of three seeded random deltas, and their fp64 integers q"""
    key = (N, K, dtype)
    if key not in _cache:
        from scratchpad_amd.delta import pack_delta
        g = torch.Generator().manual_seed(1000 + N + K)
        parts = [pack_delta(torch.randn(N, K, generator=g) * (0.02 * (s + 1)), dtype) for s in range(SLOTS)]
        codes, meta, scales = (torch.stack([p[i] for p in parts]) for i in range(3))
        _cache[key] = (codes, meta, scales, delta_oracle.dense_codes(codes, meta))
    return _cache[key]


def inputs(T, N, K, dtype):
    g = torch.Generator().manual_seed(7 * T + N + K)
    x = torch.randn(T, K + 8, generator=g).to(dtype)
    y = torch.randn(T, N + 16, generator=g).to(dtype)
    idx = indices_for(T)
    skipped = ~((idx >= 0) & (idx < SLOTS))
    y.view(torch.int16)[skipped] = SENTINEL
    return x, y, idx, skipped


def run(x, y, idx, codes, meta, scales, N, K):
    """group + product on the device; returns (y after, slot_offsets, sorted_rows) on the host"""
    from scratchpad_amd import _native
    T = x.shape[0]
    dev = "cuda"
    xd, yd, idd = x.to(dev), y.to(dev), idx.to(dev)
    offs = torch.full((SLOTS + 1,), -7, dtype=torch.int32, device=dev)
    rows = torch.full((max(T, 1),), -7, dtype=torch.int32, device=dev)
    _native.delta_group(idd, T, SLOTS, offs, rows)
    _native.delta_mm(yd[:, :N], xd[:, :K], codes.to(dev), meta.to(dev), scales.to(dev), offs, rows)
    torch.cuda.synchronize()
    return yd.cpu(), offs.cpu(), rows.cpu()


@pytest.mark.parametrize("T,slots", [(1, 3), (70, 3), (300, 5), (1000, 64)])
def test_group_is_the_stable_host_sort(T, slots):
    from scratchpad_amd import _native
    g = torch.Generator().manual_seed(T)
    idx = torch.randint(-1, slots + 2, (T,), generator=g, dtype=torch.int32)     # -1 and values >= slots included
    if slots >= 5:
        idx[idx == 1] = 0                                                        # slot 1 is empty, slot 0 large
    if T == 70:
        idx = indices_for(T)                                                     # 35 rows of slot 0: two row blocks
    offs = torch.full((slots + 1,), -7, dtype=torch.int32, device="cuda")
    rows = torch.full((T + 3,), -7, dtype=torch.int32, device="cuda")
    _native.delta_group(idx.cuda(), T, slots, offs, rows)
    want_offs, want_rows = delta_oracle.group(idx, slots)
    assert offs.tolist() == want_offs
    assert rows[: len(want_rows)].tolist() == want_rows
    assert rows[T:].tolist() == [-7] * 3, "nothing is written behind num_tokens entries"
    if slots == 5:
        assert want_offs[1] == want_offs[2] and want_offs[1] - want_offs[0] > 32, "an empty slot behind a large one"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("T", [1, 17, 70])
@pytest.mark.parametrize("N", [16, 48])
@pytest.mark.parametrize("K", [64, 320, 4160])
def test_mm_is_within_the_bound_and_leaves_skipped_rows_alone(K, N, T, dtype):
    codes, meta, scales, q = packed_slots(N, K, dtype)
    x, y, idx, skipped = inputs(T, N, K, dtype)
    got, offs, rows = run(x, y, idx, codes, meta, scales, N, K)
    want_offs, want_rows = delta_oracle.group(idx, SLOTS)
    assert offs.tolist() == want_offs and rows[: len(want_rows)].tolist() == want_rows
    want, mag = delta_oracle.mm(y[:, :N], x[:, :K], q, scales, idx)
    err = (got[:, :N].double() - want).abs()
    bound = delta_oracle.bound(want, mag, K, dtype)
    ratio = float((err / bound).max())
    print(f"[delta mm] K {K} N {N} T {T} {dtype}: largest error / bound {ratio:.3f} (depth {delta_oracle.depth(K)})")
    assert bool((err <= bound).all()), f"largest error / bound {ratio}"
    # skipped rows keep their sentinel bits; columns behind N keep theirs in every row
    assert bool((got.view(torch.int16)[skipped] == SENTINEL).all())
    assert torch.equal(got.view(torch.int16)[:, N:], y.view(torch.int16)[:, N:])
    live = ~skipped
    assert not torch.equal(got[live][:, :N], y[live][:, :N]), "the live rows did change"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("K", [320, 4160])
def test_mm_is_batch_invariant(K, dtype):
    """every live row of the 70-row batch, run alone, gets the bits it got in the batch"""
    N, T = 48, 70
    codes, meta, scales, _ = packed_slots(N, K, dtype)
    x, y, idx, skipped = inputs(T, N, K, dtype)
    batch, _, _ = run(x, y, idx, codes, meta, scales, N, K)
    dev = [t.cuda() for t in (codes, meta, scales)]
    from scratchpad_amd import _native
    offs = torch.zeros(SLOTS + 1, dtype=torch.int32, device="cuda")
    rows = torch.zeros(1, dtype=torch.int32, device="cuda")
    xd, yd, idd = x.cuda(), y.cuda(), idx.cuda()
    for t in range(T):
        if skipped[t]:
            continue
        yt = yd[t:t + 1].clone()
        _native.delta_group(idd[t:t + 1].clone(), 1, SLOTS, offs, rows)
        _native.delta_mm(yt[:, :N], xd[t:t + 1, :K], *dev, offs, rows)
        assert torch.equal(yt.cpu().view(torch.int16), batch[t:t + 1].view(torch.int16)), f"row {t} (slot {int(idx[t])})"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_an_empty_slot_adds_exactly_zero(dtype):
    """code 8, scale 1 (what the pool holds before an adapter is loaded): every value of y keeps its bits, except that
    -0.0 becomes +0.0 (y + (+0.0))"""
    from scratchpad_amd.delta import empty_delta
    N, K, T = 16, 320, 5
    codes, meta, scales = (t.unsqueeze(0).repeat(SLOTS, *[1] * t.dim()) for t in empty_delta(N, K, dtype))
    g = torch.Generator().manual_seed(5)
    x = torch.randn(T, K + 8, generator=g).to(dtype)
    y = torch.randn(T, N + 16, generator=g).to(dtype)
    y[0, 0] = -0.0
    got, _, _ = run(x, y, torch.tensor([0, 1, 2, 0, 1], dtype=torch.int32), codes, meta, scales, N, K)
    want = y.clone()
    want[0, 0] = 0.0
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
