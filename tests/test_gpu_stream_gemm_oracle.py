"""The three kernels of the weight-streaming core (csrc/stream_gemm.h: gemm_skinny_kernel, moe_gemm_kernel,
delta_mm_kernel) against fp64 statements of their own: tests/stream_gemm_oracle.py for the dense products (bound c(K)
2^-23 sum|a||b| carried through the roundings; 0 - bit equality - wherever no rounding boundary is near) and
tests/delta_oracle.py for the delta product.  tests/test_gpu_stream_gemm.py pins that the kernels AGREE; this file
checks that they are RIGHT, at the smallest shapes that reach every path of the shared k-step loop, the row-block
search, the row gather and the sum over the waves.  tests/test_stream_gemm_oracle.py proves on the CPU that the bound
rejects a missing fragment, a k-step counted twice, a dropped tail step, exchanged rows and a dropped wave on exactly
these operands.

Reduction lengths, by k-steps of 32 (8 waves take them round-robin, in groups of UNROLL = 8 per wave, then one by one):
    K =   32    1 k-step: seven waves park zeros
    K =  224    7 k-steps: wave 7 idle, tails only
    K = 1920   60 k-steps, the split class: waves 0-3 run one unrolled group, waves 4-7 seven tail steps each
    K = 2048   64 k-steps: one exact group per wave, no tail
    K = 2336   73 k-steps: a group, then one tail step (wave 0: two)
    K = 4384  137 k-steps: two groups, then a tail
Every output is a view into a buffer pre-filled with 0xA5 bytes whose other bytes are checked afterwards; every input
is a view into a NaN-filled wider tensor, so that a read or a write outside the operands shows."""
import pytest
import torch

from tests import delta_oracle, moe_oracle
from tests import stream_gemm_oracle as O
from tests.helpers import Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL = -23131                 # 0xA5A5 as int16
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]


def nat():
    from scratchpad_amd import _native
    return _native


def canary(rows, cols, dtype):
    """([rows, cols] of ``dtype`` whose every byte is 0xA5, the Guarded it is carved from)"""
    guard = Guarded()
    return guard.alloc((rows, cols), dtype), guard


def assert_untouched(backing, guard, written, what):
    """``written``: bool [rows, cols] of the backing buffer, True where the kernel may write; the rest keeps 0xA5, and
    so do the canaries around the buffer"""
    guard.check()
    bits = backing.view(torch.int16).cpu()
    assert bool((bits[~written] == FILL).all()), f"{what}: {int((bits[~written] != FILL).sum())} elements outside " \
                                                 "the output were written"


def in_nan(t, pad_cols=16, lead=8):
    """the device copy of the 2-d host tensor t as a column view into a wider NaN-filled tensor"""
    rows, cols = t.shape
    wide = torch.full((rows, cols + pad_cols), float("nan"), dtype=t.dtype, device=DEV)
    view = wide[:rows, lead:lead + cols]
    view.copy_(t)
    return view


# --------------------------------------------------------------------------- sp_gemm_skinny
def skinny_into(out, x, w, M, N, K, epilogue):
    n = nat()
    st = n.load().sp_gemm_skinny(out.data_ptr(), x.data_ptr(), w.data_ptr(), M, N, K, x.stride(0), w.stride(0),
                                 out.stride(0), epilogue, n._DTYPES[x.dtype], n._stream())
    assert st == 0, st


def skinny_case(x, w, epilogue, N, M, what):
    """one launch on views with x_stride > K, w_stride > K and out_stride > N; returns the [M, N] result on the host
    after checking every other element of its backing buffer"""
    K = x.shape[1]
    backing, guard = canary(M + 3, N + 24, x.dtype)
    out = backing[1:1 + M, 8:8 + N]
    assert x.stride(0) > K and w.stride(0) > K and out.stride(0) > N
    skinny_into(out, x[:M], w, M, N, K, epilogue)
    torch.cuda.synchronize()
    written = torch.zeros(M + 3, N + 24, dtype=torch.bool)
    written[1:1 + M, 8:8 + N] = True
    assert_untouched(backing, guard, written, what)
    return out.cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("epilogue", [0, 1])
@pytest.mark.parametrize("K", O.K_MATRIX)
def test_skinny_is_within_the_bound_at_every_kstep_class(K, epilogue, dtype):
    """1, 7, 60 (split class), 64, 73 (group + tail) and 137 (two groups + tail) k-steps at M = 1, 7, 16.  N = I = 40:
    the third workgroup of epilogue 0 clamps 8 columns, the fifth of epilogue 1 is the last; w is a column slice of a
    wider matrix (a row-parallel shard), x a row-strided view, out a view with out_stride = N + 24"""
    N = 40
    x, w = O.operands(K, dtype)                                  # [16, K], [80, K]
    xd, wd = in_nan(x, pad_cols=24), in_nan(w, pad_cols=40, lead=16)
    if epilogue == 0:
        want, bound = O.plain(x, w[:N])[:2]
        wd = wd[:N]
    else:
        want, bound = O.silu_mul(x, w[:N], w[N:])[:2]            # gate rows 0 .. 39, up rows 40 .. 79
    for M in (1, 7, 16):
        what = f"skinny epilogue {epilogue} K {K} ({O.ksteps(K)} k-steps) M {M} {dtype}"
        got = skinny_case(xd, wd, epilogue, N, M, what)
        O.compare(what, got, want[:M], bound[:M], K)
    assert float(want.abs().max()) > 0.1, "the case computes something"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_skinny_debug_instantiations_give_the_default_bits(dtype):
    """UNROLL = 16 ("skinny_unroll16", taken where (K / 32) % 128 == 0: K = 4096, 128 k-steps, each wave's 16 in ONE
    round of loads) and NT = true ("skinny_nt", at 73 and 128 k-steps): the bits of the default instantiation on the
    same operands, and the default itself inside the oracle's bound"""
    n = nat()
    N = 40
    try:
        for K, key, epilogues in ((4096, "skinny_unroll16", (0, 1)), (2336, "skinny_nt", (0,)),
                                  (4096, "skinny_nt", (0,))):
            x, w = O.operands(K, dtype)
            xd, wd = in_nan(x, pad_cols=24), in_nan(w, pad_cols=40, lead=16)
            for epilogue in epilogues:
                wv = wd[:N] if epilogue == 0 else wd
                what = f"skinny epilogue {epilogue} K {K} {dtype}"
                base = skinny_case(xd, wv, epilogue, N, 16, what)
                want, bound = (O.plain(x, w[:N]) if epilogue == 0 else O.silu_mul(x, w[:N], w[N:]))[:2]
                O.compare(what + " (default)", base, want, bound, K)
                n.debug_set(key, 1)
                got = skinny_case(xd, wv, epilogue, N, 16, what + " " + key)
                n.debug_set(key, 0)
                assert torch.equal(got.view(torch.int16), base.view(torch.int16)), f"{what}: {key} changed the bits"
    finally:
        n.debug_set("skinny_unroll16", 0)
        n.debug_set("skinny_nt", 0)


# --------------------------------------------------------------------------- sp_moe_gate_up / sp_moe_down
def layout(flat_ids, E):
    """(expert_offsets [E + 1], sorted_pos [pairs]) of moe_oracle.sort_pairs; pairs with id -1 are routed nowhere (the
    sort leaves keys outside [0, E) out): they are sorted as a group of their own behind the last expert"""
    ids = flat_ids.clone()
    if bool((ids < 0).any()):
        ids[ids < 0] = E
        off, pos = moe_oracle.sort_pairs(ids, E + 1)
        return off[:E + 1], pos
    return moe_oracle.sort_pairs(ids, E)


def moe_gate_up_case(x, w13, off, pos, topk, what, check=True):
    """sp_moe_gate_up through the C ABI on x [T, H] (x_stride = H + 16), w13 [E, 2 I, H] sliced out of a taller
    stacked tensor (w_expert_stride = (2 I + 8) H), into h [T topk, I] with h_stride = I + 24; compares every routed
    row with the oracle and returns h on the host"""
    n = nat()
    T, H = x.shape
    E, I = w13.shape[0], w13.shape[1] // 2
    NP = T * topk
    xd = in_nan(x)
    tall = torch.full((E, 2 * I + 8, H), float("nan"), dtype=x.dtype, device=DEV)
    wv = tall[:, :2 * I]
    wv.copy_(w13)
    backing, guard = canary(NP + 2, I + 24, x.dtype)
    h = backing[1:1 + NP, 8:8 + I]
    offd, posd = off.to(torch.int32).to(DEV), pos.to(torch.int32).to(DEV)
    assert wv.stride(0) > 2 * I * H and xd.stride(0) > H and h.stride(0) > I
    st = n.load().sp_moe_gate_up(h.data_ptr(), xd.data_ptr(), wv.data_ptr(), offd.data_ptr(), posd.data_ptr(), T, topk,
                                 E, H, I, xd.stride(0), h.stride(0), wv.stride(0), n._DTYPES[x.dtype], n._stream())
    assert st == 0, st
    torch.cuda.synchronize()
    routed = int(off[E])
    written = torch.zeros(NP + 2, I + 24, dtype=torch.bool)
    written[1:1 + routed, 8:8 + I] = True
    assert_untouched(backing, guard, written, what)
    got = h.cpu()
    if check:
        want, bound = torch.zeros(routed, I, dtype=torch.float64), torch.zeros(routed, I, dtype=torch.float64)
        for e in range(E):
            lo, hi = int(off[e]), int(off[e + 1])
            if hi > lo:
                want[lo:hi], bound[lo:hi] = O.silu_mul(x[pos[lo:hi] // topk], w13[e, :I], w13[e, I:])[:2]
        O.compare(what, got[:routed], want, bound, H)
    return got


def moe_down_case(h, w2, wts, off, pos, topk, what):
    """sp_moe_down through the C ABI on h [T topk, I] by sorted position (h_stride = I + 16), w2 [E, H, I] sliced out
    of a taller stacked tensor, wts fp32 [T topk] by pair, into tmp [T topk, H] by pair with tmp_stride = H + 24"""
    n = nat()
    NP, I = h.shape
    E, H = w2.shape[0], w2.shape[1]
    hd = in_nan(h)
    tall = torch.full((E, H + 8, I), float("nan"), dtype=h.dtype, device=DEV)
    wv = tall[:, :H]
    wv.copy_(w2)
    backing, guard = canary(NP + 2, H + 24, h.dtype)
    tmp = backing[1:1 + NP, 8:8 + H]
    offd, posd, wd = off.to(torch.int32).to(DEV), pos.to(torch.int32).to(DEV), wts.to(DEV)
    assert wv.stride(0) > H * I and hd.stride(0) > I and tmp.stride(0) > H
    st = n.load().sp_moe_down(tmp.data_ptr(), hd.data_ptr(), wv.data_ptr(), wd.data_ptr(), offd.data_ptr(),
                              posd.data_ptr(), NP // topk, topk, E, H, I, hd.stride(0), tmp.stride(0), wv.stride(0),
                              n._DTYPES[h.dtype], n._stream())
    assert st == 0, st
    torch.cuda.synchronize()
    routed = int(off[E])
    named = pos[:routed]
    written = torch.zeros(NP + 2, H + 24, dtype=torch.bool)
    written[1 + named, 8:8 + H] = True
    assert_untouched(backing, guard, written, what)
    want, bound = torch.zeros(NP, H, dtype=torch.float64), torch.zeros(NP, H, dtype=torch.float64)
    for e in range(E):
        lo, hi = int(off[e]), int(off[e + 1])
        if hi > lo:
            pairs = pos[lo:hi]
            want[pairs], bound[pairs] = O.down(h[lo:hi], w2[e], wts[pairs].double())[:2]
    O.compare(what, tmp.cpu()[named], want[named], bound[named], I)


def routing_weights(pairs, dtype, seed):
    """fp32 [pairs] holding values of the activation dtype, as sp_moe_route leaves them"""
    g = torch.Generator().manual_seed(seed)
    return (0.05 + 0.9 * torch.rand(pairs, generator=g)).to(dtype).float()


def expert_weights(E, rows, K, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(E, rows, K, generator=g) * K ** -0.5).to(dtype)


def long_ids(seed):
    """36 pairs (12 tokens, top_k = 3) over E = 4: 33 on expert 1, one on expert 3, two routed nowhere"""
    ids = torch.tensor([1] * 33 + [3] + [-1] * 2)
    return ids[torch.randperm(36, generator=torch.Generator().manual_seed(seed))]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("hidden", [1920, 2336])
def test_moe_gate_up_long_reduction_with_strides(hidden, dtype):
    """60 k-steps (the split class) and 73 (a group, then a tail) in moe_gemm_kernel<GATE_UP>: E = 4 with 33 rows on
    expert 1 (a full 32-row block with both sub-blocks, plus a block of one row), one on expert 3, experts 0 and 2
    empty; top_k = 3 (pair / topk is no shift); every stride larger than its width"""
    topk, E, inter = 3, 4, 32
    x = O.operands(hidden, dtype, rows=12)[0]
    w13 = expert_weights(E, 2 * inter, hidden, dtype, 6100 + hidden)
    off, pos = layout(long_ids(hidden), E)
    assert (off[1:] - off[:-1]).tolist() == [0, 33, 0, 1]
    moe_gate_up_case(x, w13, off, pos, topk, f"moe gate_up H {hidden} ({O.ksteps(hidden)} k-steps) {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("inter", [1920, 2336])
def test_moe_down_long_reduction_with_strides(inter, dtype):
    """the same row layout and k-step classes in moe_gemm_kernel<down>, scattered to the pair's row and scaled by the
    pair's routing weight"""
    topk, E, hidden = 3, 4, 32
    h = O.operands(inter, dtype, rows=36, seed=O.SEED + 1)[0]
    w2 = expert_weights(E, hidden, inter, dtype, 6200 + inter)
    off, pos = layout(long_ids(inter), E)
    h[int(off[E]):] = float("nan")                               # positions behind the routed pairs are never read
    moe_down_case(h, w2, routing_weights(36, dtype, inter), off, pos, topk,
                  f"moe down I {inter} ({O.ksteps(inter)} k-steps) {dtype}")


def wide_ids(case):
    """[T, topk] ids over 64 experts and topk"""
    g = torch.Generator().manual_seed(6300)
    if case == "counts":          # per-expert counts from {0, 1, 31, 32, 33, 65}; expert 0 empty, lane 63 live
        menu = torch.tensor([0, 1, 31, 32, 33, 65])
        counts = menu[torch.randint(0, 6, (64,), generator=g)]
        counts[0], counts[63] = 0, 33
        assert set(counts.tolist()) == set(menu.tolist())
        flat = torch.repeat_interleave(torch.arange(64), counts)
        return flat[torch.randperm(flat.numel(), generator=g)].view(-1, 1), 1
    if case == "33 each":         # 128 row blocks on a grid of ceil(2112 / 32) + 64 = 130
        flat = torch.arange(64).repeat(33)
        return flat[torch.randperm(flat.numel(), generator=g)].view(-1, 1), 1
    assert case == "top8"         # 9 tokens x 8 distinct experts each
    return torch.stack([torch.randperm(64, generator=g)[:8] for _ in range(9)]), 8


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", ["counts", "33 each", "top8"])
def test_moe_products_over_64_experts(case, dtype):
    """find_row_block with all 64 lanes: many empty groups, expert 0 empty and expert 63 (lane 63) live; 33 rows on
    every expert = 128 row blocks against the host's grid bound of 130; top_k = 8 for down's scale lookup.  Each
    product on its own: down reads the oracle's h, not gate_up's"""
    E, hidden, inter = 64, 64, 32
    ids, topk = wide_ids(case)
    T = ids.shape[0]
    off, pos = layout(ids.reshape(-1), E)
    counts = off[1:] - off[:-1]
    if case != "top8":
        assert int(counts[0]) == (0 if case == "counts" else 33) and int(counts[63]) == 33
    if case == "33 each":
        assert int(((counts + 31) // 32).sum()) == 128 and (T + 31) // 32 + E == 130
    g = torch.Generator().manual_seed(6400)
    x = torch.randn(T, hidden, generator=g).to(dtype)
    w13 = expert_weights(E, 2 * inter, hidden, dtype, 6401)
    w2 = expert_weights(E, hidden, inter, dtype, 6402)
    what = f"E 64 '{case}' T {T} top_k {topk} {dtype}"
    moe_gate_up_case(x, w13, off, pos, topk, "moe gate_up " + what)
    h = torch.zeros(T * topk, inter, dtype=torch.float64)
    for e in range(E):
        lo, hi = int(off[e]), int(off[e + 1])
        if hi > lo:
            h[lo:hi] = O.silu_mul(x[pos[lo:hi] // topk], w13[e, :inter], w13[e, inter:])[0]
    moe_down_case(h.to(dtype), w2, routing_weights(T * topk, dtype, 6403), off, pos, topk, "moe down " + what)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_moe_gate_up_rows_do_not_see_a_poisoned_neighbour(dtype):
    """one token's x row filled with NaN and Inf: its three pairs come out NaN, every other row of the same 32-row
    block keeps the bits it has without it (73 k-steps)"""
    topk, E, inter, hidden = 3, 4, 32, 2336
    x = O.operands(hidden, dtype, rows=12)[0]
    w13 = expert_weights(E, 2 * inter, hidden, dtype, 6100 + hidden)
    off, pos = layout(long_ids(hidden), E)
    token = int(pos[int(off[1]) + 5]) // topk                    # a token with a pair inside expert 1's first block
    clean = moe_gate_up_case(x, w13, off, pos, topk, f"moe gate_up clean {dtype}")
    bad = x.clone()
    bad[token, 0::2], bad[token, 1::2] = float("nan"), float("inf")
    got = moe_gate_up_case(bad, w13, off, pos, topk, f"moe gate_up poisoned {dtype}", check=False)
    routed = int(off[E])
    hit = (pos[:routed] // topk) == token
    assert int(hit.sum()) >= 1 and bool(torch.isnan(got[:routed][hit]).all()), "the poisoned pairs are NaN"
    assert torch.equal(got[:routed][~hit].view(torch.int16), clean[:routed][~hit].view(torch.int16))


# --------------------------------------------------------------------------- sp_delta_mm
_packed = {}


def packed(slots, N, K, dtype):
    key = (slots, N, K, dtype)
    if key not in _packed:
        from scratchpad_amd.delta import pack_delta
        g = torch.Generator().manual_seed(7000 + slots + K)
        parts = [pack_delta(torch.randn(N, K, generator=g) * (0.02 * (s % 3 + 1)), dtype) for s in range(slots)]
        codes, meta, scales = (torch.stack([p[i] for p in parts]) for i in range(3))
        _packed[key] = (codes, meta, scales, delta_oracle.dense_codes(codes, meta))
    return _packed[key]


def delta_case(x, y, idx, slots, N, K, what, check=True):
    """sp_delta_mm on the host grouping of delta_oracle.group; x and y are column views (both strides larger than the
    widths); returns y's [T, N + 16] backing tensor on the host"""
    n = nat()
    T = x.shape[0]
    codes, meta, scales, q = packed(slots, N, K, x.dtype)
    offs, rows = delta_oracle.group(idx, slots)
    xd = in_nan(x)
    yd = y.to(DEV)
    offd = torch.tensor(offs, dtype=torch.int32, device=DEV)
    rowd = torch.tensor(rows + [-7] * (T - len(rows)), dtype=torch.int32, device=DEV)
    n.delta_mm(yd[:, :N], xd, codes.to(DEV), meta.to(DEV), scales.to(DEV), offd, rowd)
    torch.cuda.synchronize()
    got = yd.cpu()
    live = torch.tensor([0 <= int(s) < slots for s in idx])
    assert torch.equal(got.view(torch.int16)[:, N:], y.view(torch.int16)[:, N:]), f"{what}: columns behind N"
    assert torch.equal(got.view(torch.int16)[~live], y.view(torch.int16)[~live]), f"{what}: rows of no slot"
    if check:
        want, mag = delta_oracle.mm(y[:, :N], x, q, scales, idx)
        err = (got[:, :N].double() - want).abs()
        bound = delta_oracle.bound(want, mag, K, x.dtype)
        assert bool(torch.isfinite(got[:, :N]).all())
        print(f"[stream gemm] {what}: largest err/bound {float((err / bound).max()):.3f}, bound 0 on "
              f"{float((bound == 0).double().mean()):.3f} of {bound.numel()} elements (depth {delta_oracle.depth(K)})")
        assert bool((err <= bound).all()), f"{what}: largest err/bound {float((err / bound).max()):.3f}"
        assert not torch.equal(got[live][:, :N], y[live][:, :N]), "the live rows did change"
    return got


def delta_inputs(T, N, K, dtype):
    g = torch.Generator().manual_seed(7100 + T + K)
    return torch.randn(T, K, generator=g).to(dtype), torch.randn(T, N + 16, generator=g).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_delta_mm_over_64_slots(dtype):
    """find_row_block in delta_mm_kernel with 64 groups of which three have rows: slot 0 (35 rows: two row blocks), 37
    and 63 (lane 63)"""
    T, N, K = 70, 16, 64
    idx = torch.tensor([(37, 63, -1, 64)[(t // 2) % 4] if t % 2 else 0 for t in range(T)], dtype=torch.int32)
    assert sorted(set(idx.tolist())) == [-1, 0, 37, 63, 64]
    x, y = delta_inputs(T, N, K, dtype)
    delta_case(x, y, idx, 64, N, K, f"delta mm 64 slots K {K} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_delta_mm_one_super_step_per_wave_and_a_tail(dtype):
    """K = 1856: 29 chunks of 64 columns = 8 super-steps, one per wave; the last has ONE live lane group.  Then one row
    of x filled with NaN and Inf: every other row of its 32-row block keeps its bits"""
    T, N, K, slots = 40, 16, 1856, 3
    idx = torch.tensor([(0, 1, 0, 2, 0, -1, 0, 3)[t % 8] for t in range(T)], dtype=torch.int32)
    x, y = delta_inputs(T, N, K, dtype)
    clean = delta_case(x, y, idx, slots, N, K, f"delta mm K {K} (29 chunks) {dtype}")
    bad = x.clone()
    bad[4, 0::2], bad[4, 1::2] = float("nan"), float("inf")      # row 4: slot 0, inside its first block
    got = delta_case(bad, y, idx, slots, N, K, f"delta mm poisoned {dtype}", check=False)
    assert int(idx[4]) == 0 and bool(torch.isnan(got[4, :N]).all())
    others = torch.arange(T) != 4
    assert torch.equal(got[others].view(torch.int16), clean[others].view(torch.int16))


# --------------------------------------------------------------------------- the stated safety rules
SLACK = 128        # rows (entries) of every array before and after the part the call names
BAD_OFFSETS = {    # 4 groups over total = 40 sorted entries; every value within 48 of [0, total]
    "decreasing": [0, 8, 30, 12, 12],
    "beyond the total": [0, 10, 25, 80, 88],
    "negative": [-48, -5, 10, 20, 40],
    "in order": [0, 10, 20, 30, 40],
}
TOTAL = 40


def ruled_groups(offsets, entries):
    """[(group, sorted index, entry)] that stream_gemm.h's rules leave: offsets clamped to [0, total], a group that
    would end before it begins is empty, entries outside [0, total) are skipped"""
    out = []
    for g in range(len(offsets) - 1):
        b = min(max(offsets[g], 0), TOTAL)
        en = min(max(offsets[g + 1], b), TOTAL)
        out += [(g, p, int(entries[p])) for p in range(b, en) if 0 <= int(entries[p]) < TOTAL]
    named = [e for _, _, e in out]
    assert len(set(named)) == len(named), "the case names no row twice"
    return out


def slack_metadata(offsets, seed):
    """(offsets view, sorted view, sorted entries on the host): both are views into longer int32 arrays whose slack
    holds in-range values; the entries are a permutation of 0 .. total - 1 with -3 and total + 3 in four places"""
    g = torch.Generator().manual_seed(seed)
    entries = torch.randperm(TOTAL, generator=g)
    for at, v in ((3, -3), (17, TOTAL + 3), (26, -3), (38, TOTAL + 3)):
        entries[at] = v
    off_arr = torch.randint(0, TOTAL + 1, (2 * SLACK + 5,), generator=g).to(torch.int32)
    off_arr[SLACK:SLACK + 5] = torch.tensor(offsets, dtype=torch.int32)
    ent_arr = torch.randint(0, TOTAL, (2 * SLACK + TOTAL,), generator=g).to(torch.int32)
    ent_arr[SLACK:SLACK + TOTAL] = entries.to(torch.int32)
    off_d, ent_d = off_arr.to(DEV), ent_arr.to(DEV)
    return off_d[SLACK:SLACK + 5], ent_d[SLACK:SLACK + TOTAL], entries


@pytest.mark.parametrize("case", list(BAD_OFFSETS))
def test_moe_down_obeys_the_safety_rules(case):
    """offsets that decrease, exceed the total or are negative, sorted entries of -3 and total + 3.  Every pointer the
    kernel indexes is a view with 128 rows of slack on either side and the slack of the index arrays holds in-range
    values, so a kernel WITHOUT the checks changes a row it should not or hits a canary instead of faulting"""
    n = nat()
    dtype, E, hidden, inter = torch.bfloat16, 4, 32, 64
    offsets = BAD_OFFSETS[case]
    off_v, pos_v, entries = slack_metadata(offsets, 8000)
    g = torch.Generator().manual_seed(8001)
    rows = 2 * SLACK + TOTAL
    h_all = torch.randn(rows, inter + 16, generator=g).to(dtype)
    w2 = expert_weights(E, hidden, inter, dtype, 8002)
    wts_all = routing_weights(rows, dtype, 8003)
    hd, wd, w2d = h_all.to(DEV), wts_all.to(DEV), w2.to(DEV)
    backing, guard = canary(rows, hidden + 24, dtype)
    h_v, wts_v, tmp_v = hd[SLACK:SLACK + TOTAL, 8:8 + inter], wd[SLACK:SLACK + TOTAL], \
        backing[SLACK:SLACK + TOTAL, 8:8 + hidden]
    st = n.load().sp_moe_down(tmp_v.data_ptr(), h_v.data_ptr(), w2d.data_ptr(), wts_v.data_ptr(), off_v.data_ptr(),
                              pos_v.data_ptr(), TOTAL, 1, E, hidden, inter, h_v.stride(0), tmp_v.stride(0),
                              w2d.stride(0), n._DTYPES[dtype], n._stream())
    assert st == 0, st
    torch.cuda.synchronize()
    valid = ruled_groups(offsets, entries)
    assert valid, "the case names some rows"
    written = torch.zeros(rows, hidden + 24, dtype=torch.bool)
    h_host, wts_host = h_all[SLACK:SLACK + TOTAL, 8:8 + inter], wts_all[SLACK:SLACK + TOTAL]
    named = torch.tensor([pair for _, _, pair in valid])
    written[SLACK + named, 8:8 + hidden] = True
    assert_untouched(backing, guard, written, f"moe down, offsets {case}")
    want, bound = torch.zeros(TOTAL, hidden, dtype=torch.float64), torch.zeros(TOTAL, hidden, dtype=torch.float64)
    for e in range(E):
        sel = [(p, pair) for grp, p, pair in valid if grp == e]
        if sel:
            ps, pairs = torch.tensor([s[0] for s in sel]), torch.tensor([s[1] for s in sel])
            want[pairs], bound[pairs] = O.down(h_host[ps], w2[e], wts_host[pairs].double())[:2]
    O.compare(f"moe down, offsets {case}", tmp_v.cpu()[named], want[named], bound[named], inter)


@pytest.mark.parametrize("case", list(BAD_OFFSETS))
def test_delta_mm_obeys_the_safety_rules(case):
    """the same metadata presented to delta_mm_kernel: nothing but the rows that valid metadata names changes, in y's
    whole backing tensor (128 rows of slack on either side), and those rows are within delta_oracle.bound"""
    n = nat()
    dtype, slots, N, K = torch.float16, 4, 16, 64
    offsets = BAD_OFFSETS[case]
    off_v, row_v, entries = slack_metadata(offsets, 8100)
    codes, meta, scales, q = packed(slots, N, K, dtype)
    g = torch.Generator().manual_seed(8101)
    rows = 2 * SLACK + TOTAL
    x_all = torch.randn(rows, K + 16, generator=g).to(dtype)
    y_all = torch.randn(rows, N + 16, generator=g).to(dtype)
    xd, yd = x_all.to(DEV), y_all.to(DEV)
    n.delta_mm(yd[SLACK:SLACK + TOTAL, 8:8 + N], xd[SLACK:SLACK + TOTAL, 8:8 + K], codes.to(DEV), meta.to(DEV),
               scales.to(DEV), off_v, row_v)
    torch.cuda.synchronize()
    valid = ruled_groups(offsets, entries)
    assert valid, "the case names some rows"
    idx = torch.full((TOTAL,), -1, dtype=torch.int32)
    for grp, _, row in valid:
        idx[row] = grp
    got = yd.cpu()
    changed = torch.zeros(rows, N + 16, dtype=torch.bool)
    named = torch.tensor([row for _, _, row in valid])
    changed[SLACK + named, 8:8 + N] = True
    assert torch.equal(got.view(torch.int16)[~changed], y_all.view(torch.int16)[~changed]), \
        f"delta mm, offsets {case}: an element outside the named rows changed"
    y_host, x_host = y_all[SLACK:SLACK + TOTAL, 8:8 + N], x_all[SLACK:SLACK + TOTAL, 8:8 + K]
    want, mag = delta_oracle.mm(y_host, x_host, q, scales, idx)
    err = (got[SLACK:SLACK + TOTAL, 8:8 + N].double() - want).abs()
    bound = delta_oracle.bound(want, mag, K, dtype)
    print(f"[stream gemm] delta mm, offsets {case}: largest err/bound {float((err / bound).max()):.3f}, bound 0 on "
          f"{float((bound == 0).double().mean()):.3f} of {bound.numel()} elements")
    assert bool(torch.isfinite(got).all()) and bool((err <= bound).all())
    assert not torch.equal(got[SLACK + named, 8:8 + N], y_all[SLACK + named, 8:8 + N]), "the named rows did change"

