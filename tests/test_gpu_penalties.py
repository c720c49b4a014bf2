"""The penalty / vocab-mask kernels (csrc/penalties.hip) on the GPU, against the reference's recorded outputs
(tests/golden/penalties.npz) and against tests/penalty_oracle.py at real size.

Bound (tests/penalty_oracle.tolerance, derived there): |diff| <= c^2 u |f| + 3 u max(|x|, c |f| + |p|) per touched
element, u = 2^-24 (the first term not granted to penalties that are exact in binary); -inf positions equal;
untouched columns bit-identical (compared as int32); the store equal to a host Counter, exactly."""
from collections import Counter

import numpy as np
import pytest
import torch

from tests import golden, penalty_oracle as po

pytestmark = pytest.mark.gpu
G = golden.load("penalties")


def _state(pool_rows, capacity):
    from scratchpad_amd.penalty_state import PenaltyState
    return PenaltyState(pool_rows, capacity, "cuda")


def _feed(state, rows, histories, vocab):
    """cumulate histories[r] (lists of ids, any length) into pool rows `rows`, one launch per position"""
    longest = max(len(h) for h in histories)
    ids = np.full((longest, len(histories)), -1, dtype=np.int64)
    for j, h in enumerate(histories):
        ids[:len(h), j] = h
    ids = torch.from_numpy(ids).cuda()
    for s in range(longest):
        state.cumulate(rows, ids[s], vocab)


def _stops_table(stops, width=None):
    width = max(1, max(len(s) for s in stops)) if width is None else width
    t = np.full((len(stops), width), -1, dtype=np.int32)
    for i, s in enumerate(stops):
        t[i, :len(s)] = sorted(s)
    return torch.from_numpy(t).cuda()


def _assert_store_equals(state, rows, histories, vocab):
    nd, ol = state.n_distinct.cpu().numpy(), state.out_len.cpu().numpy()
    entries = state.entries.cpu().numpy()
    for row, h in zip(rows.tolist(), histories):
        want = Counter(t for t in h if 0 <= t < vocab)
        assert nd[row] == len(want) and ol[row] == sum(want.values()), (row, nd[row], len(want), ol[row])
        got = {int(t): int(c) for t, c in entries[row, :nd[row]]}
        assert got == dict(want), f"pool row {row}"


@pytest.mark.parametrize("key", [f"orch{i}_{w}" for i in range(int(G["orch_cases"])) for w in ("mid", "fin")])
def test_kernels_reproduce_the_reference_orchestrator(key):
    x, want = G[key + "_logits_in"], G[key + "_logits_out"]
    hist, freq, pres, min_new = G[key + "_history"], G[key + "_freq"], G[key + "_pres"], G[key + "_min_new"]
    bs, vocab = x.shape
    histories = [[int(t) for t in h if t >= 0] for h in hist]
    state = _state(16, 96)
    rows = torch.tensor([11, 3, 7, 0, 15, 9, 2, 5][:bs], dtype=torch.int64, device="cuda")
    _feed(state, rows, histories, vocab)
    _assert_store_equals(state, rows, histories, vocab)
    logits = torch.from_numpy(x).cuda()
    state.apply(logits, vocab, rows, torch.from_numpy(freq).cuda(), torch.from_numpy(pres).cuda(),
                torch.ones(bs, device="cuda"), torch.from_numpy(min_new).cuda(), torch.from_numpy(G[key + "_stops"]).cuda())
    state.check()
    worst = po.check_against(logits.cpu().numpy(), want, x, po.tolerance(x, hist, freq, pres), key)
    print(f"{key}: worst |diff| / bound = {worst:.3f}")


@pytest.mark.parametrize("ci", [0, 1])
def test_kernels_reproduce_apply_logits_bias_with_repetition(ci):
    key = f"bias{ci}"
    x, want = G[key + "_logits_in"], G[key + "_logits_out"]
    hist, freq, pres, rep = G[key + "_history"], G[key + "_freq"], G[key + "_pres"], G[key + "_rep"]
    bs, vocab = x.shape
    state = _state(8, 32)
    rows = torch.tensor([5, 0, 7, 2, 6, 1], dtype=torch.int32, device="cuda")          # int32 indices: graph mode
    _feed(state, rows, [list(map(int, h)) for h in hist], vocab)
    logits = torch.from_numpy(x).cuda()
    state.apply(logits, vocab, rows, torch.from_numpy(freq).cuda(), torch.from_numpy(pres).cuda(), torch.from_numpy(rep).cuda())
    tol = po.tolerance(x, hist, freq, pres, rep)
    worst = po.check_against(logits.cpu().numpy(), want, x, tol, key)
    print(f"{key}: worst |diff| / bound = {worst:.3f}")


def test_real_size_against_the_oracle():
    """bs 256, vocab 128 256, row stride > vocab, 1 ... 2 048 emitted tokens per row with heavy repetition, pool rows
    scrambled and beyond the batch size"""
    bs, vocab, stride, pool_rows, capacity = 256, 128256, 128256 + 64, 700, 2048
    rng = np.random.default_rng(2024)
    want_lens = rng.integers(1, 2049, bs)
    want_lens[4:8] = [1, 2, 2048, 2047]
    histories = []
    for n in want_lens:
        pool = rng.integers(0, vocab, max(1, int(n) // int(rng.integers(2, 9))))
        histories.append(pool[rng.integers(0, len(pool), int(n))].tolist())
    histories[0] = [vocab - 1] * 37 + [0] * 5                                   # the edges of the vocabulary
    lens = np.array([len(h) for h in histories])
    assert lens.min() == 1 and lens.max() == 2048
    rows = torch.from_numpy(rng.permutation(pool_rows)[:bs].astype(np.int64)).cuda()
    assert int(rows.max()) >= bs
    state = _state(pool_rows, capacity)
    state.entries.fill_(-7)                                                     # stale words behind n_distinct
    _feed(state, rows, histories, vocab)
    state.check()
    _assert_store_equals(state, rows, histories, vocab)
    others = np.setdiff1d(np.arange(pool_rows), rows.cpu().numpy())
    assert not state.n_distinct.cpu().numpy()[others].any() and not state.out_len.cpu().numpy()[others].any()

    choices_f = np.array([0.0, 0.5, -0.25, 1.5, 0.3, -0.7, 1.9, -2.0], dtype=np.float32)
    choices_p = np.array([0.0, 0.5, -1.3, 1.1, 2.0], dtype=np.float32)
    choices_r = np.array([1.0, 1.0, 1.5, 0.5, 1.1, 0.9], dtype=np.float32)
    freq, pres, rep = (c[rng.integers(0, len(c), bs)] for c in (choices_f, choices_p, choices_r))
    freq[1], pres[1], rep[1] = 0.0, 0.0, 1.0                                    # a neutral row
    min_new = np.where(rng.random(bs) < 0.5, 0, lens + rng.integers(-2, 3, bs)).astype(np.int32)
    min_new[2], min_new[3] = lens[2], lens[3] + 1                               # exactly at, and one short of, release
    stops = [set(rng.integers(0, vocab, int(rng.integers(1, 4))).tolist()) | ({histories[i][0]} if i % 3 == 0 else set())
             for i in range(bs)]
    x = (rng.standard_normal((bs, vocab)) * 3).astype(np.float32)
    buf = torch.full((bs, stride), 12345.0, dtype=torch.float32, device="cuda")
    logits = buf[:, :vocab]
    logits.copy_(torch.from_numpy(x))
    state.apply(logits, vocab, rows, torch.from_numpy(freq).cuda(), torch.from_numpy(pres).cuda(),
                torch.from_numpy(rep).cuda(), torch.from_numpy(min_new).cuda(), _stops_table(stops))
    got = logits.cpu().numpy()
    assert bool((buf[:, vocab:] == 12345.0).all()), "columns behind the vocabulary were written"
    want = po.apply_penalties(x, histories, freq, pres, rep, min_new, [sorted(s) for s in stops])
    tol = po.tolerance(x, histories, freq, pres, rep)
    worst = po.check_against(got, want, x, tol, "real size")
    print(f"real size: worst |diff| / bound = {worst:.3f}; -inf cells {int(np.isneginf(want).sum())}")
    assert np.isneginf(want[3]).any() and not np.isneginf(want[2]).any()


def test_reset_ignored_ids_and_empty_batch():
    vocab = 500
    state = _state(12, 16)
    rows = torch.tensor([9, 4, 6], dtype=torch.int64, device="cuda")
    hist = [[1, 2, 1, 499], [3, 3, 3], [0, 7]]
    _feed(state, rows, hist, vocab)
    # ids outside [0, vocab): padding rows, unresolved placeholders of the overlap worker - the row is untouched
    state.cumulate(rows, torch.tensor([-1, 500, -12345], dtype=torch.int64, device="cuda"), vocab)
    state.cumulate(torch.tensor([-1, 12, 4], dtype=torch.int64, device="cuda"),
                   torch.tensor([5, 5, 8], dtype=torch.int64, device="cuda"), vocab)      # rows outside the pool: skipped
    hist[1].append(8)
    _assert_store_equals(state, rows, hist, vocab)
    state.reset(torch.tensor([4, -1, 99], dtype=torch.int64, device="cuda"))
    hist[1] = []
    _assert_store_equals(state, rows, hist, vocab)
    # batch_size == 0 is fine and launches nothing
    empty = torch.zeros(0, dtype=torch.int64, device="cuda")
    state.cumulate(empty, empty, vocab)
    state.reset(empty)
    state.apply(torch.zeros((0, vocab), device="cuda"), vocab, empty, *(torch.zeros(0, device="cuda"),) * 3)
    from scratchpad_amd import _native
    _native.vocab_mask_apply_(torch.zeros((0, vocab), device="cuda"), torch.zeros((0, 16), dtype=torch.int32, device="cuda"))
    _assert_store_equals(state, rows, hist, vocab)
    # a full row is never written past: the error word is raised and stays
    small = _state(2, 3)
    r0 = torch.tensor([1], dtype=torch.int64, device="cuda")
    for t in (5, 6, 7, 7):
        small.cumulate(r0, torch.tensor([t], dtype=torch.int64, device="cuda"), vocab)
    small.check()
    small.cumulate(r0, torch.tensor([8], dtype=torch.int64, device="cuda"), vocab)
    with pytest.raises(RuntimeError, match="full"):
        small.check()
    assert small.history(1) == ([[5, 1], [6, 1], [7, 2]], 4) and small.history(0) == ([], 0)


@pytest.mark.parametrize("ci", range(int(G["bitmask_cases"])))
def test_packed_bitmask_kernel(ci):
    from scratchpad_amd import _native
    key = f"bitmask{ci}"
    x, mask, want = G[key + "_logits_in"], G[key + "_mask"], G[key + "_logits_out"]
    bs, vocab = x.shape
    buf = torch.full((bs, vocab + 40), 7.0, device="cuda")
    logits = buf[:, :vocab]
    logits.copy_(torch.from_numpy(x))
    _native.vocab_mask_apply_(logits, torch.from_numpy(mask).cuda())
    assert np.array_equal(logits.cpu().numpy().view(np.int32), want.view(np.int32))
    assert bool((buf[:, vocab:] == 7.0).all())
    with pytest.raises(RuntimeError, match="too large"):
        _native.vocab_mask_apply_(logits, torch.zeros((bs, (vocab + 31) // 32 + 1), dtype=torch.int32, device="cuda"))


def test_bool_mask_kernel_and_real_size_masks():
    from scratchpad_amd import _native
    x, mask, want = G["boolmask_logits_in"], G["boolmask_mask"], G["boolmask_logits_out"]
    logits = torch.from_numpy(x).cuda()
    _native.vocab_mask_apply_(logits, torch.from_numpy(mask).cuda())
    assert np.array_equal(logits.cpu().numpy().view(np.int32), want.view(np.int32))
    with pytest.raises(RuntimeError, match="neither"):
        _native.vocab_mask_apply_(logits, torch.zeros(x.shape, dtype=torch.uint8, device="cuda"))
    rng = np.random.default_rng(5)
    bs, vocab = 256, 128256
    x = (rng.standard_normal((bs, vocab)) * 3).astype(np.float32)
    for w in (vocab // 32, vocab // 32 - 1):
        bits = rng.integers(-2 ** 31, 2 ** 31, (bs, w)).astype(np.int32)
        logits = torch.from_numpy(x).cuda()
        _native.vocab_mask_apply_(logits, torch.from_numpy(bits).cuda())
        assert np.array_equal(logits.cpu().numpy().view(np.int32), po.apply_bitmask(x, bits).view(np.int32)), w
    forbid = rng.random((bs, vocab)) < 0.7
    logits = torch.from_numpy(x).cuda()
    _native.vocab_mask_apply_(logits, torch.from_numpy(forbid).cuda())
    assert np.array_equal(logits.cpu().numpy().view(np.int32), po.apply_bool_mask(x, forbid).view(np.int32))


def test_reset_cumulate_apply_mask_in_one_hip_graph():
    """a plain single-branch capture of the four launches, replayed with changed inputs"""
    from scratchpad_amd import _native
    bs, vocab = 8, 2000
    rng = np.random.default_rng(9)
    state = _state(20, 64)
    rows = torch.tensor(rng.permutation(20)[:bs].astype(np.int64)).cuda()
    reset_rows = rows.clone()
    ids = torch.zeros(bs, dtype=torch.int64, device="cuda")
    logits = torch.zeros((bs, vocab), device="cuda")
    mask = torch.zeros((bs, (vocab + 31) // 32), dtype=torch.int32, device="cuda")
    freq = torch.tensor([0.5, 0.3, 0.0, -0.25, 1.5, 0.0, -0.7, 1.0], device="cuda")
    pres = torch.tensor([0.0, 0.5, 0.0, 1.1, 0.0, -1.3, 0.0, 0.25], device="cuda")
    rep = torch.tensor([1.0, 1.5, 1.0, 0.5, 1.0, 1.1, 1.0, 0.9], device="cuda")
    min_new = torch.tensor([0, 2, 0, 1, 0, 0, 3, 0], dtype=torch.int32, device="cuda")
    stops = _stops_table([{5}, {6, 7}, set(), {8}, set(), set(), {1, 2, 3}, set()])

    def step():
        state.reset(reset_rows)
        state.cumulate(rows, ids, vocab)
        state.apply(logits, vocab, rows, freq, pres, rep, min_new, stops)
        _native.vocab_mask_apply_(logits, mask)

    step()                                   # (loads the library, warms the launch paths)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    histories = [[] for _ in range(bs)]
    for replay in range(3):
        new_ids = rng.integers(0, 6, bs) if replay else rng.integers(0, vocab, bs)
        x = (rng.standard_normal((bs, vocab)) * 3).astype(np.float32)
        bits = rng.integers(-2 ** 31, 2 ** 31, mask.shape).astype(np.int32)
        ids.copy_(torch.from_numpy(new_ids))
        logits.copy_(torch.from_numpy(x))
        mask.copy_(torch.from_numpy(bits))
        if replay == 0:
            reset_rows.copy_(rows)           # first replay: forget what the warm-up and the capture left
        else:
            reset_rows.fill_(-1)             # later ones: reset nothing, the history grows
        graph.replay()
        torch.cuda.synchronize()
        for h, t in zip(histories, new_ids.tolist()):
            h.append(t)
        _assert_store_equals(state, rows, histories, vocab)
        st = [sorted(t for t in row if t >= 0) for row in stops.cpu().tolist()]
        want = po.apply_bitmask(po.apply_penalties(x, histories, freq.cpu().numpy(), pres.cpu().numpy(),
                                                   rep.cpu().numpy(), min_new.cpu().numpy(), st), bits)
        tol = po.tolerance(x, histories, freq.cpu().numpy(), pres.cpu().numpy(), rep.cpu().numpy())
        forbidden = np.isneginf(po.apply_bitmask(x, bits))
        tol[forbidden] = 1.0                 # (a masked column is -inf on both sides, not "untouched")
        po.check_against(logits.cpu().numpy(), want, x, tol, f"replay {replay}")


def test_zero_rows_return_ok_and_write_nothing_through_the_header_binding():
    """the four entry points as an integrator calls them (tests/c_header.py): num_rows == 0 is SP_OK and nothing is
    written, whatever the buffers hold - what tests/test_gpu_c_abi.py::test_batch_size_zero_writes_nothing checks of
    the entry points whose batch parameter is called batch_size, with the same guarded buffer"""
    from scratchpad_amd import _native
    from tests import c_header
    from tests.test_gpu_c_abi import Guarded
    lib = c_header.bind(_native.lib_path())
    buf = Guarded(1, 1 << 16, 1 << 16, torch.uint8)
    a = buf.t[0, 4096:]
    s = torch.cuda.current_stream().cuda_stream
    calls = {
        "sp_penalty_reset": dict(n_distinct=a, out_len=a, pool_row_indices=a, idx64=1, pool_rows=8),
        "sp_penalty_cumulate": dict(entries=a, n_distinct=a, out_len=a, error=a, req_pool_indices=a, idx64=1,
                                    token_ids=a, pool_rows=8, capacity=64, vocab=1000),
        "sp_penalty_apply": dict(logits=a, row_stride=1030, entries=a, n_distinct=a, out_len=a, req_pool_indices=a,
                                 idx64=0, frequency_penalties=a, presence_penalties=a, repetition_penalties=a,
                                 min_new_tokens=a, stop_token_ids=a, max_stops=3, pool_rows=8, capacity=64, vocab=1000),
        "sp_vocab_mask_apply": dict(logits=a, row_stride=1030, mask=a, mask_stride=32, mask_width=32, mask_kind=0,
                                    vocab=1000),
    }
    takes_rows = sorted(n for n, (_, args) in lib.sp_prototypes.items()
                        if n.startswith(("sp_penalty_", "sp_vocab_mask_")) and any(p == "num_rows" for p, _ in args))
    assert sorted(calls) == takes_rows
    for name, kw in calls.items():
        rc = c_header.call(lib, name, num_rows=0, stream=s, **kw)
        torch.cuda.synchronize()
        assert rc == 0, (name, rc)
        buf.check(f"{name} with num_rows 0", None)
