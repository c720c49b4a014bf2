"""What the shared weight-streaming core (csrc/stream_gemm.h, csrc/group_sort.hip) guarantees by construction, pinned
bit for bit: the grouped MoE products equal the skinny kernel on the same rows (same k-steps per wave, same MFMA order,
same sum over the waves, same rounding points), and the two grouping entries are one sort.

Reduction lengths: 32 is ONE k-step (seven of the eight waves park zero tiles); 2336 is 73 k-steps (every wave runs one
unrolled group of 8 and then a one-step tail).  33 rows of one expert are one full 32-row block using both 16-row
sub-blocks, plus a block of one row.

Agreement is not correctness: a defect in the shared code is shared by both sides of these equalities.  Correctness is
checked in tests/test_gpu_stream_gemm_oracle.py, which holds each of the three kernels to an fp64 oracle of its own
(tests/stream_gemm_oracle.py, tests/delta_oracle.py) at every k-step class of the loop."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = 33
SLICES = ((0, 16), (16, 32), (32, 33))


def _native():
    from scratchpad_amd import _native
    return _native


def skinny(x, w, n_out, epilogue):
    """sp_gemm_skinny on x [M <= 16, K] and w [rows, K]"""
    nat = _native()
    M, K = x.shape
    out = torch.empty((M, n_out), dtype=x.dtype, device=DEV)
    assert nat.load().sp_gemm_skinny(out.data_ptr(), x.data_ptr(), w.data_ptr(), M, n_out, K, x.stride(0), w.stride(0),
                                     out.stride(0), epilogue, nat._DTYPES[x.dtype], nat._stream()) == 0
    return out


def one_expert_routing():
    """(ids, weights, offsets, sorted positions) of T tokens over ONE expert: every weight is exactly 1.0"""
    ids, wts, off, pos = _native().moe_route(torch.zeros((T, 1), dtype=torch.float32, device=DEV), 1)
    assert torch.equal(wts.cpu(), torch.ones(T, 1)) and torch.equal(pos.cpu().long(), torch.arange(T))
    assert off.cpu().tolist() == [0, T]
    return ids, wts, off, pos


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("hidden", [32, 2336])
def test_moe_gate_up_equals_skinny_silu_epilogue(hidden, dtype):
    inter = 32
    g = torch.Generator().manual_seed(4100 + hidden)
    x = torch.randn(T, hidden, generator=g).to(dtype).to(DEV)
    w13 = (torch.randn(1, 2 * inter, hidden, generator=g) * hidden ** -0.5).to(dtype).to(DEV)
    _ids, _wts, off, pos = one_expert_routing()
    h = _native().moe_gate_up(x, w13, off, pos, 1)
    for lo, hi in SLICES:
        assert torch.equal(h[lo:hi], skinny(x[lo:hi], w13[0], inter, 1)), f"rows {lo}..{hi - 1}"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("inter", [32, 2336])
def test_moe_down_equals_skinny_plain_epilogue(inter, dtype):
    hidden = 32
    g = torch.Generator().manual_seed(4200 + inter)
    h = torch.randn(T, inter, generator=g).to(dtype).to(DEV)
    w2 = (torch.randn(1, hidden, inter, generator=g) * inter ** -0.5).to(dtype).to(DEV)
    _ids, wts, off, pos = one_expert_routing()
    tmp = _native().moe_down(h, w2, wts, off, pos, 1)
    for lo, hi in SLICES:
        assert torch.equal(tmp[lo:hi], skinny(h[lo:hi], w2[0], hidden, 0)), f"rows {lo}..{hi - 1}"


def test_moe_route_and_delta_group_are_one_sort():
    nat = _native()
    tokens, groups = 300, 5
    key = torch.randint(0, groups, (tokens,), generator=torch.Generator().manual_seed(4300))
    logits = torch.nn.functional.one_hot(key, groups).float().to(DEV)
    ids, _wts, expert_offsets, sorted_pos = nat.moe_route(logits, 1)
    assert torch.equal(ids.cpu().long().flatten(), key)
    slot_offsets = torch.full((groups + 1,), -1, dtype=torch.int32, device=DEV)
    sorted_rows = torch.full((tokens,), -1, dtype=torch.int32, device=DEV)
    nat.delta_group(ids.flatten(), tokens, groups, slot_offsets, sorted_rows)
    assert torch.equal(expert_offsets, slot_offsets) and torch.equal(sorted_pos, sorted_rows)
    want_offsets = torch.cat([torch.zeros(1, dtype=torch.long), torch.bincount(key, minlength=groups).cumsum(0)])
    want_sorted = torch.sort(key, stable=True).indices
    assert torch.equal(expert_offsets.cpu().long(), want_offsets) and torch.equal(sorted_pos.cpu().long(), want_sorted)
