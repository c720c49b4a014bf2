"""End-to-end parity of the hosted Llama-MoE decoder (ModelRunner -> ForwardBatch -> HipAttnBackend -> C ABI) against
the logits of the reference's own LlamaMoEForCausalLM (tests/golden/tiny_llama_moe.npz), at the bars
tests/test_gpu_apertus.py holds Apertus to.  Variant a has 4 experts top-2 and an untied head, variant b 8 experts
top-3 and a tied head.  fp32 runs take the per-expert library loop behind the device router, 16-bit runs the grouped
kernels; the fixture's router gaps (>= 0.125) keep a 16-bit run on the reference's experts, so the tolerances below
measure arithmetic and cannot hide a different routing."""
import pytest
import torch

from tests import moe_oracle

pytestmark = pytest.mark.gpu
FUSED = ("route", "gate_up", "down", "combine")


def rel(got, want):
    return float((got - want).abs().max() / want.abs().max())


@pytest.fixture(scope="module")
def oracle16():
    """the oracle evaluated in fp16 / bf16, once per (variant, dtype)"""
    cache = {}

    def get(name, dtype):
        if (name, dtype) not in cache:
            cache[name, dtype] = moe_oracle.oracle_run(name, dtype)[:2]
        return cache[name, dtype]
    return get


@pytest.mark.parametrize("name", ["a", "b"])
def test_tiny_llama_moe_fp32_matches_reference_logits(name):
    from scratchpad_amd import _native
    g, pfx, _, _ = moe_oracle.load_case(name)
    gp, gd, gn = (torch.from_numpy(g[pfx + k]) for k in ("prefill_logits", "decode_logits", "next_ids"))
    calls = dict(_native.MOE_CALLS)
    prefill, decode, nxt, mr = moe_oracle.run_case(name, torch.float32)
    # fp32: the device router, then the per-expert library loop - two layers x two steps
    assert _native.MOE_CALLS["fallback"] == calls["fallback"] + 4 and _native.MOE_CALLS["route"] == calls["route"] + 4
    assert all(_native.MOE_CALLS[k] == calls[k] for k in ("gate_up", "down", "combine"))
    for got, want, what in ((prefill, gp, "prefill"), (decode, gd, "decode")):
        assert rel(got, want) <= 1e-4, f"{name} {what}: relative logit deviation {rel(got, want):.2e}"
    assert torch.equal(nxt, gn)
    k0 = mr.token_to_kv_pool.get_key_buffer(0).float().cpu()
    v1 = mr.token_to_kv_pool.get_value_buffer(1).float().cpu()
    assert torch.allclose(k0, torch.from_numpy(g[pfx + "k_buffer0_after"]), atol=2e-5)
    assert torch.allclose(v1, torch.from_numpy(g[pfx + "v_buffer1_after"]), atol=2e-5)


@pytest.mark.parametrize("name", ["a", "b"])
def test_tiny_llama_moe_fp16_within_1e3_on_the_grouped_kernels(name, oracle16):
    from scratchpad_amd import _native
    g, pfx, _, _ = moe_oracle.load_case(name)
    gp = torch.from_numpy(g[pfx + "prefill_logits"])
    calls = dict(_native.MOE_CALLS)
    prefill, decode, _, _ = moe_oracle.run_case(name, torch.float16)
    assert all(_native.MOE_CALLS[k] == calls[k] + 4 for k in FUSED) and _native.MOE_CALLS["fallback"] == calls["fallback"]
    o1, o2 = oracle16(name, torch.float16)
    for got, want, what in ((prefill, o1, "prefill"), (decode, o2, "decode")):
        assert rel(got, want) <= 1e-3, f"{name} {what}: relative logit deviation {rel(got, want):.2e} vs fp16 oracle"
    assert rel(prefill, gp) <= 5e-3


@pytest.mark.parametrize("name", ["a", "b"])
def test_tiny_llama_moe_bf16_and_graph_replay(name, oracle16):
    from scratchpad_amd import _native
    calls = dict(_native.MOE_CALLS)
    eager = moe_oracle.run_case(name, torch.bfloat16)
    assert all(_native.MOE_CALLS[k] == calls[k] + 4 for k in FUSED)
    graph = moe_oracle.run_case(name, torch.bfloat16, graph_bs=[2, 4])
    assert _native.MOE_CALLS["fallback"] == calls["fallback"], "a 16-bit step took the per-expert loop"
    o1, o2 = oracle16(name, torch.bfloat16)
    for got, want, what in ((eager[0], o1, "prefill"), (eager[1], o2, "decode")):
        assert rel(got, want) <= 3e-2, f"{name} {what}: {rel(got, want):.2e} vs bf16 oracle"
    # graph replay (padded from bs 3 to the bs-4 bucket) computes the same thing as eager: the MoE part is batch
    # invariant, attention under the range geometry is not
    assert torch.allclose(graph[1], eager[1], atol=1e-2 * float(eager[1].abs().max()))
    assert torch.equal(graph[0], eager[0]), "prefill is eager in both runs"


def test_exchanged_experts_change_the_logits_and_follow_the_oracle():
    """a checkpoint with experts 0 and 1 of layer 0 exchanged, gate rows left alone: each slot applies its own weights"""
    _, _, _, w = moe_oracle.load_case("a")
    swapped = moe_oracle.swap_experts(w, layer=0, a=0, b=1)
    base = moe_oracle.run_case("a", torch.float32)
    other = moe_oracle.run_case("a", torch.float32, w=swapped)
    want = moe_oracle.oracle_run("a", w=swapped)[0]
    assert rel(other[0], base[0]) > 1e-3, "exchanging two experts left the logits where they were"
    assert rel(other[0], want) <= 1e-4, "the exchanged checkpoint does not follow the oracle run on the same weights"
