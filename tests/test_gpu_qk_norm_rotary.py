"""sp_qk_norm_rotary (per-head RMSNorm of q and k + rotary + fused KV store in one launch) against the three-launch
form it replaces: sp_rmsnorm on the [T*Hq, D] rows of q, sp_rmsnorm on the [T*Hkv, D] rows of k, then
sp_rotary_embedding with the same store arguments.  The bar is bit-identity (torch.equal) on q, on k and on the pool's
K and V rows, for every dtype, head shape, rotary layout and view below; the two halves of the three-launch form are
themselves pinned to the reference's vectors by tests/test_gpu_elementwise.py.  At fp32 the result is also anchored to
the CPU restatement of the reference's own order (tests/qwen3_oracle.py)."""
import itertools

import pytest
import torch

from oracle import ops
from tests import qwen3_oracle

pytestmark = pytest.mark.gpu

DEV = "cuda"
MAX_POS = 64
EPS = 1e-6
HEADS = [(32, 8), (5, 1), (8, 1), (1, 1), (3, 2)]        # the product shape, then partly filled waves / lane groups
TOKENS = [1, 3, 257]
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
SENTINEL = 7.0


@pytest.fixture(scope="module")
def nat():
    from scratchpad_amd import _native
    _native.load()
    return _native


def make_problem(dtype, T, Hq, Hkv, D, rot, merged, seed):
    """q, k, v as column slices of one [T, (Hq + 2 Hkv) D] tensor (the model's layout) or as separate tensors whose
    rows carry 16 bytes of padding; weights on the 1 + 0.1 randn grid; a pool of T + 9 slots filled with a sentinel."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, device=DEV, dtype=torch.float32)
    pad = 16 // torch.empty(0, dtype=dtype).element_size()
    if merged:
        qkv = rnd(T, (Hq + 2 * Hkv) * D).to(dtype)
        q, k, v = qkv.split([Hq * D, Hkv * D, Hkv * D], dim=-1)
        holders = [qkv]
    else:
        holders = [torch.full((T, H * D + pad), SENTINEL, device=DEV, dtype=dtype) for H in (Hq, Hkv, Hkv)]
        q, k, v = (h[:, : h.shape[1] - pad] for h in holders)
        for t in (q, k, v):
            t.copy_(rnd(*t.shape).to(dtype))
    # rows that stress the norm: an all-zero head, a head scaled by 2^8, a head scaled by 2^-8
    q[0, :D] = 0
    k[0, :D] *= 256.0
    q[T - 1, (Hq - 1) * D:] *= 2.0 ** -8
    wq = (1.0 + 0.1 * rnd(D)).to(dtype)
    wk = (1.0 + 0.1 * rnd(D)).to(dtype)
    cache = ops.rope_cos_sin_cache(MAX_POS, 1000000.0, rot, None, dtype).to(DEV)
    pos = torch.randint(0, MAX_POS, (T,), generator=g, device=DEV, dtype=torch.int64)
    pos[0], pos[T - 1] = 0, MAX_POS - 1
    if T == 1:
        pos[0] = MAX_POS - 1
    P = T + 9
    loc = (torch.randperm(P, generator=g, device=DEV)[:T] + 1).to(torch.int64)       # a permutation with gaps
    return dict(q=q, k=k, v=v, wq=wq, wk=wk, cache=cache, pos=pos, loc=loc, P=P, holders=holders)


def pools(p, dtype, Hkv, D):
    return (torch.full((p["P"] + 1, Hkv, D), SENTINEL, device=DEV, dtype=dtype),
            torch.full((p["P"] + 1, Hkv, D), SENTINEL, device=DEV, dtype=dtype))


def three_launch(nat, p, D, neox, store, dtype, Hkv):
    """the form the fused launch replaces, on contiguous copies of q and k"""
    q = nat.rmsnorm(p["q"].reshape(-1, D).contiguous(), p["wq"], EPS).view(p["q"].shape[0], -1)
    k = nat.rmsnorm(p["k"].reshape(-1, D).contiguous(), p["wk"], EPS).view(p["k"].shape[0], -1)
    kb, vb = pools(p, dtype, Hkv, D) if store else (None, None)
    nat.rotary_embedding(p["pos"], q, k, D, p["cache"], neox, value=p["v"].contiguous() if store else None,
                         k_buffer=kb, v_buffer=vb, out_cache_loc=p["loc"] if store else None)
    return q, k, kb, vb


def run_fused(nat, p, D, neox, store, dtype, Hkv):
    kb, vb = pools(p, dtype, Hkv, D) if store else (None, None)
    nat.qk_norm_rotary(p["pos"], p["q"], p["k"], p["wq"], p["wk"], EPS, D, p["cache"], neox,
                       value=p["v"] if store else None, k_buffer=kb, v_buffer=vb,
                       out_cache_loc=p["loc"] if store else None)
    return kb, vb


@pytest.mark.parametrize("D", [128, 64, 256, 80])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
def test_bit_identical_to_the_three_launch_form(nat, dtype, D):
    """Every (heads, T, rotary_dim, layout, view, store) combination at this dtype and head size.  D = 64 / 128 / 256
    must take the fused kernel (QK_NORM_CALLS), D = 80 the wrapper's three-launch fallback; both give the same bits."""
    expect = "three_launch" if D == 80 else "fused"
    heads = HEADS if D != 256 else [(5, 1), (3, 2)]
    tokens = TOKENS if D != 256 else [3]
    seed = 0
    for (Hq, Hkv), T, rot, neox, merged, store in itertools.product(heads, tokens, (D, D // 2), (True, False),
                                                                     (True, False), (True, False)):
        seed += 1
        p = make_problem(dtype, T, Hq, Hkv, D, rot, merged, seed)
        what = f"{dtype} D {D} heads {Hq}/{Hkv} T {T} rot {rot} neox {neox} merged {merged} store {store}"
        v_before = p["v"].clone()
        want_q, want_k, want_kb, want_vb = three_launch(nat, p, D, neox, store, dtype, Hkv)
        before = dict(nat.QK_NORM_CALLS)
        kb, vb = run_fused(nat, p, D, neox, store, dtype, Hkv)
        after = dict(nat.QK_NORM_CALLS)
        assert after[expect] == before[expect] + 1 and sum(after.values()) == sum(before.values()) + 1, \
            f"{what}: expected the {expect} path, counters went {before} -> {after}"
        assert torch.equal(p["q"], want_q), f"{what}: q differs"
        assert torch.equal(p["k"], want_k), f"{what}: k differs"
        assert torch.equal(p["v"], v_before), f"{what}: v was written"
        if not merged:
            pad = p["holders"][0].shape[1] - p["q"].shape[1]
            for h in p["holders"]:
                assert bool((h[:, -pad:] == SENTINEL).all()), f"{what}: the padding of a row was written"
        if store:
            assert torch.equal(kb, want_kb) and torch.equal(vb, want_vb), f"{what}: pool rows differ"
            assert torch.equal(kb[p["loc"]].view(T, -1), p["k"]), f"{what}: the pool's K rows are not k"
            assert torch.equal(vb[p["loc"]].view(T, -1), p["v"]), f"{what}: the pool's V rows are not v"
            untouched = torch.ones(p["P"] + 1, dtype=torch.bool, device=DEV)
            untouched[p["loc"]] = False
            assert bool((kb[untouched] == SENTINEL).all()) and bool((vb[untouched] == SENTINEL).all()), \
                f"{what}: a slot outside out_cache_loc was written"
    assert seed == len(heads) * len(tokens) * 16


def test_product_shape_takes_the_fused_kernel_through_the_c_abi(nat):
    """Qwen3-8B heads in bf16 on the model's qkv layout: the library itself accepts the launch (SP_OK, no refusal the
    wrapper could paper over), and refuses head_size 80 with SP_ERR_UNSUPPORTED before any launch."""
    dtype, Hq, Hkv, D, T = torch.bfloat16, 32, 8, 128, 3
    p = make_problem(dtype, T, Hq, Hkv, D, D, True, 99)
    lib = nat.load()
    call = lambda head: lib.sp_qk_norm_rotary(
        p["pos"].data_ptr(), p["q"].data_ptr(), p["k"].data_ptr(), p["wq"].data_ptr(), p["wk"].data_ptr(), EPS,
        p["cache"].data_ptr(), T, Hq, Hkv, head, min(head, D), p["q"].stride(0), p["k"].stride(0), 1, None, 0, None,
        None, None, 0, nat.SP_BF16, torch.cuda.current_stream().cuda_stream)
    assert call(D) == nat.SP_OK
    q_after = p["q"].clone()
    assert call(80) == nat.SP_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(p["q"], q_after), "a refused call wrote q"


@pytest.mark.parametrize("D", [128, 64])
def test_fp32_agrees_with_the_reference_order_on_the_cpu(nat, D):
    """The same inputs through the CPU restatement of _apply_qk_norm + forward_native rotary: every head within 2e-6
    of its largest magnitude (the fp32 bar of the elementwise suite)."""
    for (Hq, Hkv), T, rot, neox in itertools.product([(32, 8), (3, 2)], [3, 257], (D, D // 2), (True, False)):
        p = make_problem(torch.float32, T, Hq, Hkv, D, rot, True, 1000 + T + Hq + rot + neox)
        ref_q, ref_k = qwen3_oracle.qk_norm_rotary(p["pos"].cpu(), p["q"].cpu().contiguous(), p["k"].cpu().contiguous(),
                                                   p["wq"].cpu(), p["wk"].cpu(), EPS, D, p["cache"].cpu(), neox)
        run_fused(nat, p, D, neox, False, torch.float32, Hkv)
        for got, ref, what in ((p["q"], ref_q, "q"), (p["k"], ref_k, "k")):
            got, ref = got.cpu().view(T, -1, D).double(), ref.view(T, -1, D).double()
            err = (got - ref).abs().amax(-1)
            bound = 2e-6 * ref.abs().amax(-1)
            assert bool((err <= bound).all()), \
                f"D {D} heads {Hq}/{Hkv} T {T} rot {rot} neox {neox} {what}: worst {float((err / bound.clamp_min(1e-30)).max()):.3f} of the bound"


def test_graph_replay_equals_eager(nat):
    """One capture of the fused launch; positions and out_cache_loc are rewritten between replays (no host reads, no
    allocation inside the launch)."""
    dtype, Hq, Hkv, D, T = torch.bfloat16, 32, 8, 128, 5
    probs = [make_problem(dtype, T, Hq, Hkv, D, D, True, 500 + i) for i in range(3)]
    s = probs[0]
    static = dict(qkv=s["holders"][0].clone(), pos=s["pos"].clone(), loc=s["loc"].clone())
    q, k, v = static["qkv"].split([Hq * D, Hkv * D, Hkv * D], dim=-1)
    kb, vb = pools(s, dtype, Hkv, D)
    launch = lambda: nat.qk_norm_rotary(static["pos"], q, k, s["wq"], s["wk"], EPS, D, s["cache"], True, value=v,
                                        k_buffer=kb, v_buffer=vb, out_cache_loc=static["loc"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for p in probs[1:]:
        static["qkv"].copy_(p["holders"][0])
        static["pos"].copy_(p["pos"])
        static["loc"].copy_(p["loc"])
        kb.fill_(SENTINEL)
        vb.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        # eager on the same inputs, same weights and cache as the captured launch
        e = dict(p, wq=s["wq"], wk=s["wk"], cache=s["cache"])
        ekb, evb = run_fused(nat, e, D, True, True, dtype, Hkv)
        assert torch.equal(static["qkv"], p["holders"][0]), "replay differs from eager on q / k / v"
        assert torch.equal(kb, ekb) and torch.equal(vb, evb), "replay differs from eager on the pool"
