"""The mixture-of-experts kernels (csrc/moe.hip) against tests/moe_oracle.py: routing (ids exact, weights bit for bit,
the stable sort), the grouped expert MLP at row counts around the kernel's own block (every element within the
oracle's derived bound), canaries behind every output, batch invariance, and a captured sequence that follows a
rewritten routing."""
import pytest
import torch

from tests import moe_oracle
from tests.helpers import Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"


def sp_dtype(t):
    from scratchpad_amd import _native
    return _native._DTYPES[t.dtype]


def route_raw(logits, K, guard):
    """sp_moe_route into guarded buffers"""
    from scratchpad_amd import _native
    T, E = logits.shape
    ids, wts = guard.alloc((T, K), torch.int32), guard.alloc((T, K), torch.float32)
    off, pos = guard.alloc((E + 1,), torch.int32), guard.alloc((T * K,), torch.int32)
    st = _native.load().sp_moe_route(ids.data_ptr(), wts.data_ptr(), off.data_ptr(), pos.data_ptr(), logits.data_ptr(),
                                     T, E, K, logits.stride(0), sp_dtype(logits), _native._stream())
    assert st == 0
    return ids, wts, off, pos


def experts_raw(x, w13, w2, ids, wts, off, pos, guard):
    """gate_up, down and combine into guarded buffers"""
    from scratchpad_amd import _native
    lib, st = _native.load(), _native._stream()
    T, H = x.shape
    K, E, inter = ids.shape[1], w13.shape[0], w2.shape[2]
    h, tmp, out = guard.alloc((T * K, inter), x.dtype), guard.alloc((T * K, H), x.dtype), guard.alloc((T, H), x.dtype)
    dt = sp_dtype(x)
    assert lib.sp_moe_gate_up(h.data_ptr(), x.data_ptr(), w13.data_ptr(), off.data_ptr(), pos.data_ptr(), T, K, E, H,
                              inter, x.stride(0), h.stride(0), w13.stride(0), dt, st) == 0
    assert lib.sp_moe_down(tmp.data_ptr(), h.data_ptr(), w2.data_ptr(), wts.data_ptr(), off.data_ptr(), pos.data_ptr(),
                           T, K, E, H, inter, h.stride(0), tmp.stride(0), w2.stride(0), dt, st) == 0
    assert lib.sp_moe_combine(out.data_ptr(), tmp.data_ptr(), ids.data_ptr(), T, K, E, H, tmp.stride(0), out.stride(0),
                              dt, st) == 0
    return out


def check_route(logits, K):
    guard = Guarded()
    ids, wts, off, pos = route_raw(logits, K, guard)
    torch.cuda.synchronize()
    guard.check()
    want_ids, want_w = moe_oracle.route(logits, K)
    assert torch.equal(ids.cpu().long(), want_ids), "ids"
    assert torch.equal(wts.cpu(), want_w), "weights are bit-exact"
    want_off, want_pos = moe_oracle.sort_pairs(want_ids, logits.shape[1])
    assert torch.equal(off.cpu().long(), want_off) and torch.equal(pos.cpu().long(), want_pos), "the stable sort"
    return ids


# --------------------------------------------------------------------------- routing
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("E,K", [(4, 2), (8, 3), (64, 8), (8, 1)])
def test_route_matches_the_oracle(dtype, E, K):
    g = torch.Generator().manual_seed(1000 + 10 * E + K)
    for T in (1, 3, 65, 257):
        # 16-bit draws of this size hold equal logits within a row: the lower index has to win
        logits = (torch.randn(T, E, generator=g) * 2).to(dtype).to(DEV)
        check_route(logits, K)


def test_route_strided_view_ties_single_expert_and_nan():
    g = torch.Generator().manual_seed(7)
    wide = torch.randn(65, 24, generator=g).bfloat16().to(DEV)
    check_route(wide[:, 3:11], 3)                                     # row stride 24, first column 3
    ids = check_route(torch.full((5, 8), 0.75, dtype=torch.float16, device=DEV), 3)
    assert ids.cpu().tolist() == [[0, 1, 2]] * 5, "all-equal logits give ids 0 .. K-1"
    one = torch.full((70, 8), -3.0, dtype=torch.bfloat16, device=DEV)
    one[:, 5] = 4.0
    ids = check_route(one, 1)
    assert bool((ids == 5).all()), "every token on expert 5"
    bad = torch.randn(33, 8, generator=g).to(DEV)
    bad[::3, 2] = float("nan")
    bad[1::3] = float("nan")
    bad[5, :] = float("-inf")
    guard = Guarded()
    ids, _, off, pos = route_raw(bad, 3, guard)
    torch.cuda.synchronize()
    guard.check()
    assert int(ids.min()) >= 0 and int(ids.max()) < 8, "every id is in [0, E) whatever the logits hold"
    want_off, want_pos = moe_oracle.sort_pairs(ids.cpu().long(), 8)
    assert torch.equal(off.cpu().long(), want_off) and torch.equal(pos.cpu().long(), want_pos)
    assert all(len(set(r)) == 3 for r in ids.cpu().tolist()), "a token never takes an expert twice"


# --------------------------------------------------------------------------- the grouped MLP
def routed_logits(pairs, E, dtype, perm_seed):
    """router logits [T, E] that put token i on experts pairs[i] = (first, second), weights varying by token; the
    tokens are shuffled so that an expert's rows are scattered over the batch"""
    T = len(pairs)
    logits = torch.full((T, E), -4.0)
    for i, (a, b) in enumerate(pairs):
        logits[i, a] = 2.0 + 0.125 * (i % 5)
        logits[i, b] = 1.0 - 0.25 * (i % 3)
    perm = torch.randperm(T, generator=torch.Generator().manual_seed(perm_seed))
    return logits[perm].to(dtype).to(DEV)


def count_cases(BM):
    """per-expert row counts {0, 1, BM-1, BM, BM+1}; the first and the last expert are among the empty ones"""
    return {
        "0,1,BM-1,BM": [(1, 3)] + [(2, 3)] * (BM - 1),
        "BM+1,BM,1,0": [(0, 1)] * BM + [(0, 2)],
        "0,BM+1,BM+1,0": [(1, 2)] * (BM + 1),
    }


@pytest.fixture(scope="module")
def mlp_weights():
    cache = {}

    def get(H, inter, dtype):
        if (H, inter, dtype) not in cache:
            g = torch.Generator().manual_seed(H + inter)
            cache[H, inter, dtype] = ((torch.randn(4, 2 * inter, H, generator=g) * 0.08).to(dtype).to(DEV),
                                      (torch.randn(4, H, inter, generator=g) * 0.08).to(dtype).to(DEV))
        return cache[H, inter, dtype]
    return get


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("H,inter", [(256, 96), (128, 32)])
@pytest.mark.parametrize("case", ["0,1,BM-1,BM", "BM+1,BM,1,0", "0,BM+1,BM+1,0"])
def test_grouped_mlp_within_the_derived_bound(dtype, H, inter, case, mlp_weights):
    from scratchpad_amd import _native
    BM = _native.moe_block_rows()
    assert BM == _native.MOE_BLOCK_ROWS
    pairs = count_cases(BM)[case]
    w13, w2 = mlp_weights(H, inter, dtype)
    logits = routed_logits(pairs, 4, dtype, perm_seed=len(pairs))
    T = len(pairs)
    x = torch.randn(T, H, generator=torch.Generator().manual_seed(T + H)).to(dtype).to(DEV)
    guard = Guarded()
    ids, wts, off, pos = route_raw(logits, 2, guard)
    counts = (off[1:] - off[:-1]).cpu().tolist()
    assert counts == {"0,1,BM-1,BM": [0, 1, BM - 1, BM], "BM+1,BM,1,0": [BM + 1, BM, 1, 0],
                      "0,BM+1,BM+1,0": [0, BM + 1, BM + 1, 0]}[case]
    want_ids, want_w = moe_oracle.route(logits, 2)
    assert torch.equal(ids.cpu().long(), want_ids) and torch.equal(wts.cpu(), want_w)
    out = experts_raw(x, w13, w2, ids, wts, off, pos, guard)
    torch.cuda.synchronize()
    guard.check()
    want, bound = moe_oracle.experts(x, w13, w2, want_ids, want_w)
    err = (out.cpu().double() - want).abs()
    over = err > bound
    print(f"{case} H {H} I {inter} {dtype}: max err {float(err.max()):.3e}, max bound {float(bound.max()):.3e}, "
          f"elements with bound 0: {float((bound == 0).double().mean()):.3f}")
    assert not bool(over.any()), f"{int(over.sum())} of {over.numel()} elements outside the derived bound; worst " \
                                 f"{float((err - bound).max()):.3e}"
    assert float(want.abs().max()) > 0.01, "the case computes something"


# --------------------------------------------------------------------------- batch invariance
def test_a_tokens_output_does_not_depend_on_the_batch():
    from scratchpad_amd import _native
    g = torch.Generator().manual_seed(21)
    H, inter, E, K, dtype = 256, 96, 4, 2, torch.bfloat16
    w13 = (torch.randn(E, 2 * inter, H, generator=g) * 0.08).to(dtype).to(DEV)
    w2 = (torch.randn(E, H, inter, generator=g) * 0.08).to(dtype).to(DEV)
    x = torch.randn(70, H, generator=g).to(dtype).to(DEV)
    logits = (torch.randn(70, E, generator=g) * 2).to(dtype).to(DEV)
    full = _native.moe_experts(x, logits, w13, w2, K)
    alone = _native.moe_experts(x[37:38].contiguous(), logits[37:38].contiguous(), w13, w2, K)
    # the other rows' routing permuted: every expert receives other rows, in another order, in other numbers
    perm = torch.randperm(70, generator=g).to(DEV)
    mixed = logits[perm].clone()
    mixed[37] = logits[37]
    other = _native.moe_experts(x, mixed, w13, w2, K)
    torch.cuda.synchronize()
    assert torch.equal(alone[0], full[37]), "row 37 of T = 70 differs from the token run alone"
    assert torch.equal(other[37], full[37]), "row 37 changed with its neighbours' routing"
    assert not torch.equal(other, full)


# --------------------------------------------------------------------------- graph capture
def test_a_captured_sequence_follows_a_rewritten_routing():
    from scratchpad_amd import _native
    g = torch.Generator().manual_seed(31)
    H, inter, E, K, dtype = 128, 32, 4, 2, torch.float16
    w13 = (torch.randn(E, 2 * inter, H, generator=g) * 0.08).to(dtype).to(DEV)
    w2 = (torch.randn(E, H, inter, generator=g) * 0.08).to(dtype).to(DEV)
    x = torch.randn(4, H, generator=g).to(dtype).to(DEV)
    first = routed_logits([(0, 1), (0, 1), (2, 3), (0, 3)], E, dtype, perm_seed=0)
    second = routed_logits([(2, 3), (2, 3), (0, 1), (1, 2)], E, dtype, perm_seed=0)     # same shuffle: all move
    logits = first.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _native.moe_experts(x, logits, w13, w2, K)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    calls = dict(_native.MOE_CALLS)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _native.moe_experts(x, logits, w13, w2, K)
    assert all(_native.MOE_CALLS[k] == calls[k] + 1 for k in ("route", "gate_up", "down", "combine"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, _native.moe_experts(x, first, w13, w2, K))
    logits.copy_(second)
    graph.replay()
    torch.cuda.synchronize()
    want = _native.moe_experts(x, second, w13, w2, K)
    ids1, ids2 = moe_oracle.route(first, K)[0], moe_oracle.route(second, K)[0]
    assert all(not set(a) & set(b) for a, b in zip(ids1.tolist(), ids2.tolist())), "every token changed both experts"
    assert torch.equal(out, want), "the replay did not follow the rewritten logits"
    assert not torch.equal(want, _native.moe_experts(x, first, w13, w2, K))
