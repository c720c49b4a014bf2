"""The quantised mixture-of-experts kernels (csrc/quant_moe.hip) against tests/quant_moe_oracle.py: the two grouped
packed products within the oracle's derived bound (bit for bit where it is 0), the combine bit for bit in both orders,
the reduction order against sp_delta_mm, batch invariance, canaries around every output, and a captured sequence that
follows a rewritten routing."""
import pytest
import torch

from tests import moe_oracle, quant_moe_oracle as qo
from tests.helpers import Guarded
from tests.stream_gemm_oracle import compare

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
EK = [(1, 1), (4, 2), (64, 8)]
TOKENS = (1, 17, 70)


def dev(packed):
    return tuple(t.to(DEV) for t in packed)


def routed(T, E, K, dtype, seed):
    """seeded logits -> (ids, wts, offsets, pos) on the device, the ids and weights checked against the oracle"""
    from scratchpad_amd import _native
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(T, E, generator=g) * 2).to(dtype)
    ids, wts, off, pos = _native.moe_route(logits.to(DEV), K)
    want_ids, want_w = moe_oracle.route(logits, K)
    assert torch.equal(ids.cpu().long(), want_ids) and torch.equal(wts.cpu(), want_w)
    return want_ids, want_w, ids, wts, off, pos


@pytest.fixture(scope="module")
def experts_of():
    """seeded packed experts, generated and unpacked once per (E, rows, reduction length, dtype)"""
    cache = {}

    def get(E, N, K, dtype):
        key = (E, N, K, dtype)
        if key not in cache:
            packed = qo.random_packed(E, N, K, dtype, seed=E + N + K)
            cache[key] = (dev(packed), qo.unpack(packed))
        return cache[key]
    return get


# --------------------------------------------------------------------------- the derived bound
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hidden", [64, 320, 4160])      # one lane quarter live, a tail super-step, three rounds a wave
def test_gate_up_within_the_derived_bound(dtype, hidden, experts_of):
    from scratchpad_amd import _native
    inter = 64
    for E, K in EK:
        packed, unpacked = experts_of(E, 2 * inter, hidden, dtype)
        for T in TOKENS:
            want_ids, _, ids, wts, off, pos = routed(T, E, K, dtype, seed=100 * T + E)
            x = torch.randn(T, hidden, generator=torch.Generator().manual_seed(T + hidden)).to(dtype)
            guard = Guarded()
            h = _native.qmoe_gate_up(x.to(DEV), packed, off, pos, K, out=guard.alloc((T * K, inter), dtype))
            torch.cuda.synchronize()
            guard.check()
            want, bound = qo.gate_up(x, unpacked, want_ids)
            compare(f"qmoe gate_up {dtype} H {hidden} E {E} K {K} T {T}", h, want, bound, hidden)
            assert float(want.abs().max()) > 0.01, "the case computes something"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("inter", [64, 320])
def test_down_within_the_derived_bound(dtype, inter, experts_of):
    from scratchpad_amd import _native
    hidden = 64
    for E, K in EK:
        packed, unpacked = experts_of(E, hidden, inter, dtype)
        for T in TOKENS:
            want_ids, want_w, ids, wts, off, pos = routed(T, E, K, dtype, seed=200 * T + E)
            h = (torch.randn(T * K, inter, generator=torch.Generator().manual_seed(T + inter)) * 0.5).to(dtype)
            guard = Guarded()
            tmp = _native.qmoe_down(h.to(DEV), packed, wts, off, pos, K, out=guard.alloc((T * K, hidden), dtype))
            torch.cuda.synchronize()
            guard.check()
            want, bound = qo.down(h, unpacked, want_ids, want_w, dtype)
            compare(f"qmoe down {dtype} I {inter} E {E} K {K} T {T}", tmp, want, bound, inter)
            assert float(want.abs().max()) > 0.01, "the case computes something"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order", [qo.ORDER_EXPERT, qo.ORDER_RANK])
def test_block_with_an_empty_and_an_overfull_expert(dtype, order, experts_of):
    """the three launches chained, 70 tokens top-2 over 4 experts of which the last owns no row and the others more
    than one 32-row block each"""
    from scratchpad_amd import _native
    T, E, K, hidden, inter = 70, 4, 2, 320, 64
    g = torch.Generator().manual_seed(7)
    logits = torch.randn(T, E, generator=g) * 2
    logits[:, 3] = -30.0
    logits = logits.to(dtype)
    x = torch.randn(T, hidden, generator=g).to(dtype)
    base = torch.randn(T, hidden, generator=g).to(dtype)
    p13, u13 = experts_of(E, 2 * inter, hidden, dtype)
    p2, u2 = experts_of(E, hidden, inter, dtype)
    ids, wts, off, pos = _native.moe_route(logits.to(DEV), K)
    counts = (off[1:] - off[:-1]).cpu().tolist()
    assert counts[3] == 0 and min(counts[:3]) > 32 and sum(counts) == T * K
    want_ids, want_w = moe_oracle.route(logits, K)
    assert torch.equal(ids.cpu().long(), want_ids) and torch.equal(wts.cpu(), want_w)
    guard = Guarded()
    h = _native.qmoe_gate_up(x.to(DEV), p13, off, pos, K, out=guard.alloc((T * K, inter), dtype))
    tmp = _native.qmoe_down(h, p2, wts, off, pos, K, out=guard.alloc((T * K, hidden), dtype))
    out = _native.qmoe_combine(tmp, ids, E, base.to(DEV), order, out=guard.alloc((T, hidden), dtype))
    torch.cuda.synchronize()
    guard.check()
    want, bound = qo.experts(x, u13, u2, want_ids, want_w, base, order)
    compare(f"qmoe block {dtype} order {order}", out, want, bound, hidden)


# --------------------------------------------------------------------------- combine
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [1, 2, 8])
def test_combine_is_bit_exact_in_both_orders(dtype, K):
    from scratchpad_amd import _native
    T, E, H = 37, 8, 320
    g = torch.Generator().manual_seed(40 + K)
    tmp = torch.randn(T * K, H, generator=g).to(dtype)
    base = torch.randn(T, H, generator=g).to(dtype)
    ids = torch.randint(-2, E + 2, (T, K), generator=g).to(torch.int32)      # duplicates and ids outside [0, E)
    assert int(ids.min()) < 0 and int(ids.max()) >= E
    if K > 1:
        ids[3] = 5                                                           # one expert K times: ties go by k
        assert any(len(set(r)) < K for r in ids.tolist())
    outs = []
    for order in (qo.ORDER_EXPERT, qo.ORDER_RANK):
        guard = Guarded()
        out = _native.qmoe_combine(tmp.to(DEV), ids.to(DEV), E, base.to(DEV), order, out=guard.alloc((T, H), dtype))
        torch.cuda.synchronize()
        guard.check()
        want, bound = qo.combine(tmp, ids, E, base, order, dtype)
        assert float(bound.max()) == 0.0
        assert torch.equal(out.cpu().double(), want), f"order {order}"
        alias = base.to(DEV)
        assert _native.qmoe_combine(tmp.to(DEV), ids.to(DEV), E, alias, order, out=alias) is alias
        assert torch.equal(alias, out), "out may alias base"
        outs.append(out.cpu())
    assert (K < 3) == torch.equal(outs[0], outs[1]), "the orders differ once three rows are added, never below"


# --------------------------------------------------------------------------- the reduction order is sp_delta_mm's
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("inter", [64, 320, 4160])
def test_down_equals_delta_mm_on_a_zeroed_y(dtype, inter, experts_of):
    from scratchpad_amd import _native
    S, N = 3, 64
    packed, _ = experts_of(S, N, inter, dtype)
    ids = torch.tensor([0] * 5 + [1] * 34 + [2], dtype=torch.int32)          # ascending: pair t is sorted position t
    T = ids.numel()
    h = (torch.randn(T, inter, generator=torch.Generator().manual_seed(inter)) * 0.5).to(dtype).to(DEV)
    off = torch.zeros(S + 1, dtype=torch.int32, device=DEV)
    pos = torch.zeros(T, dtype=torch.int32, device=DEV)
    _native.delta_group(ids.to(DEV), T, S, off, pos)
    assert pos.cpu().tolist() == list(range(T))
    ones = torch.ones(T, 1, dtype=torch.float32, device=DEV)
    tmp = _native.qmoe_down(h, packed, ones, off, pos, 1)
    y = torch.zeros(T, N, dtype=dtype, device=DEV)
    _native.delta_mm(y, h, *packed, off, pos)
    torch.cuda.synchronize()
    assert float(y.float().abs().max()) > 0.01
    assert torch.equal(tmp.view(torch.int16), y.view(torch.int16)), "the bits differ from sp_delta_mm's"


# --------------------------------------------------------------------------- batch invariance
def test_a_tokens_output_does_not_depend_on_the_batch(experts_of):
    from scratchpad_amd import _native
    T, E, K, hidden, inter, dtype = 70, 3, 2, 320, 64, torch.bfloat16
    g = torch.Generator().manual_seed(21)
    p13, _ = experts_of(E, 2 * inter, hidden, dtype)
    p2, _ = experts_of(E, hidden, inter, dtype)
    x = torch.randn(T, hidden, generator=g).to(dtype).to(DEV)
    base = torch.randn(T, hidden, generator=g).to(dtype).to(DEV)
    logits = (torch.randn(T, E, generator=g) * 2).to(dtype).to(DEV)
    run = lambda xs, ls, bs, order: _native.qmoe_experts(xs, ls, p13, p2, K, order, bs.clone())
    for order in (qo.ORDER_EXPERT, qo.ORDER_RANK):
        full = run(x, logits, base, order)
        alone = torch.cat([run(x[t:t + 1].contiguous(), logits[t:t + 1].contiguous(), base[t:t + 1], order)
                           for t in range(T)])
        torch.cuda.synchronize()
        assert torch.equal(alone, full), f"order {order}: a row of T = 70 differs from the token run alone"
    # the other rows' routing permuted: every expert receives other rows, in another order, in other numbers
    perm = torch.randperm(T, generator=g).to(DEV)
    mixed = logits[perm].clone()
    mixed[37] = logits[37]
    other = run(x, mixed, base, qo.ORDER_RANK)
    torch.cuda.synchronize()
    assert torch.equal(other[37], full[37]), "row 37 changed with its neighbours' routing"
    assert not torch.equal(other, full)


# --------------------------------------------------------------------------- guards
def test_rows_past_the_last_valid_pair_are_left_untouched(experts_of):
    """ids outside [0, E) (a sort that leaves pairs out: expert_offsets[E] < T K): their rows of h and tmp keep their
    bytes, and the combine skips them"""
    from scratchpad_amd import _native
    T, E, K, hidden, inter, dtype = 19, 4, 2, 64, 64, torch.float16
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, E, (T, K), generator=g).to(torch.int32)
    ids[2, 1], ids[7, 0], ids[18, 1] = -1, E, 99
    left_out = [2 * K + 1, 7 * K, 18 * K + 1]
    wts = torch.rand(T, K, generator=g).to(dtype).float()
    x = torch.randn(T, hidden, generator=g).to(dtype)
    base = torch.randn(T, hidden, generator=g).to(dtype)
    p13, u13 = experts_of(E, 2 * inter, hidden, dtype)
    p2, u2 = experts_of(E, hidden, inter, dtype)
    guard = Guarded()
    off, pos = guard.alloc((E + 1,), torch.int32), guard.alloc((T * K,), torch.int32)
    _native.delta_group(ids.reshape(-1).to(DEV), T * K, E, off, pos)              # the shared stable sort
    valid = T * K - len(left_out)
    assert int(off[E]) == valid
    h = _native.qmoe_gate_up(x.to(DEV), p13, off, pos, K, out=guard.alloc((T * K, inter), dtype))
    tmp = _native.qmoe_down(h, p2, wts.to(DEV), off, pos, K, out=guard.alloc((T * K, hidden), dtype))
    out = _native.qmoe_combine(tmp, ids.to(DEV), E, base.to(DEV), qo.ORDER_EXPERT,
                               out=guard.alloc((T, hidden), dtype))
    torch.cuda.synchronize()
    guard.check()
    assert bool((h[valid:].view(torch.uint8) == 0xA5).all()), "rows of h past expert_offsets[E] were written"
    assert bool((h[:valid].view(torch.uint8) != 0xA5).any(dim=1).all())
    assert bool((tmp[left_out].view(torch.uint8) == 0xA5).all()), "a pair that is in no group had its tmp row written"
    want_off, want_pos = qo.sort_valid(ids, E)
    assert torch.equal(off.cpu().long(), want_off) and torch.equal(pos[:valid].cpu().long(), want_pos)
    hv, ev = qo.gate_up(x, u13, ids.long())
    tv, et = qo.down(hv, u2, ids.long(), wts, dtype, ev)
    want, bound = qo.combine(tv, ids, E, base, qo.ORDER_EXPERT, dtype, et)
    compare("qmoe block with pairs left out", out, want, bound, hidden)


# --------------------------------------------------------------------------- graph capture
def test_a_captured_sequence_follows_a_rewritten_routing(experts_of):
    from scratchpad_amd import _native
    T, E, K, hidden, inter, dtype = 4, 4, 2, 64, 64, torch.float16
    g = torch.Generator().manual_seed(31)
    p13, _ = experts_of(E, 2 * inter, hidden, dtype)
    p2, _ = experts_of(E, hidden, inter, dtype)
    x = torch.randn(T, hidden, generator=g).to(dtype).to(DEV)
    base = torch.randn(T, hidden, generator=g).to(dtype).to(DEV)

    def routed_logits(pairs):
        logits = torch.full((T, E), -4.0)
        for i, (a, b) in enumerate(pairs):
            logits[i, a], logits[i, b] = 2.0 + 0.125 * i, 1.0 - 0.25 * i
        return logits.to(dtype).to(DEV)
    first = routed_logits([(0, 1), (0, 1), (2, 3), (0, 3)])
    second = routed_logits([(2, 3), (2, 3), (0, 1), (1, 2)])
    run = lambda ls: _native.qmoe_experts(x, ls, p13, p2, K, qo.ORDER_RANK, base.clone())
    logits = first.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(logits)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    calls, route = dict(_native.QMOE_CALLS), _native.MOE_CALLS["route"]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(logits)
    assert all(_native.QMOE_CALLS[k] == calls[k] + 1 for k in calls) and _native.MOE_CALLS["route"] == route + 1
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, run(first))
    logits.copy_(second)
    graph.replay()
    torch.cuda.synchronize()
    want = run(second)
    ids1, ids2 = moe_oracle.route(first, K)[0], moe_oracle.route(second, K)[0]
    assert all(not set(a) & set(b) for a, b in zip(ids1.tolist(), ids2.tolist())), "every token changed both experts"
    assert torch.equal(out, want), "the replay did not follow the rewritten logits"
    assert not torch.equal(want, run(first))
