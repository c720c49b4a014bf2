"""End-to-end parity of the hosted Apertus decoder (ModelRunner -> ForwardBatch -> HipAttnBackend -> C ABI) against the
logits of the reference's own SwissAIForCausalLM (tests/golden/tiny_apertus.npz), at the bars tests/test_gpu_qwen3.py
holds Qwen3 to.  Variant a has head_dim 64 and an untied head, variant b head_dim 128 and a tied head; both run the
fused per-head norm + rotary + KV-store launch in every layer and the ungated xIELU MLP."""
import pytest
import torch

from tests import apertus_oracle

pytestmark = pytest.mark.gpu


def rel(got, want):
    return float((got - want).abs().max() / want.abs().max())


@pytest.fixture(scope="module")
def oracle16():
    """the oracle evaluated in fp16 / bf16, once per (variant, dtype)"""
    cache = {}

    def get(name, dtype):
        if (name, dtype) not in cache:
            cache[name, dtype] = apertus_oracle.oracle_run(name, dtype)[:2]
        return cache[name, dtype]
    return get


@pytest.mark.parametrize("name", ["a", "b"])
def test_tiny_apertus_fp32_matches_reference_logits(name):
    from scratchpad_amd import _native
    g, pfx, _, _ = apertus_oracle.load_case(name)
    gp, gd, gn = (torch.from_numpy(g[pfx + k]) for k in ("prefill_logits", "decode_logits", "next_ids"))
    qk, xi = dict(_native.QK_NORM_CALLS), dict(_native.XIELU_CALLS)
    prefill, decode, nxt, mr = apertus_oracle.run_case(name, torch.float32)
    assert _native.QK_NORM_CALLS["fused"] == qk["fused"] + 4, "two layers x two steps of the fused launch"
    assert _native.QK_NORM_CALLS["three_launch"] == qk["three_launch"]
    # fp32: the skinny kernel is 16-bit only, so both steps (15 and 3 rows) are refused and take the two calls
    assert _native.XIELU_CALLS["two_call"] == xi["two_call"] + 4 and _native.XIELU_CALLS["xielu"] == xi["xielu"] + 4
    assert _native.XIELU_CALLS["gemm_skinny_xielu"] == xi["gemm_skinny_xielu"]
    for got, want, what in ((prefill, gp, "prefill"), (decode, gd, "decode")):
        assert rel(got, want) <= 1e-4, f"{name} {what}: relative logit deviation {rel(got, want):.2e}"
    assert torch.equal(nxt, gn)
    k0 = mr.token_to_kv_pool.get_key_buffer(0).float().cpu()
    v1 = mr.token_to_kv_pool.get_value_buffer(1).float().cpu()
    assert torch.allclose(k0, torch.from_numpy(g[pfx + "k_buffer0_after"]), atol=2e-5)
    assert torch.allclose(v1, torch.from_numpy(g[pfx + "v_buffer1_after"]), atol=2e-5)
    written = torch.from_numpy(g[pfx + "k_buffer0_after"]).abs().sum((1, 2)) > 0
    assert torch.equal(k0.abs().sum((1, 2)) > 0, written), "exactly the reference's slots are written"


@pytest.mark.parametrize("name", ["a", "b"])
def test_tiny_apertus_fp16_within_1e3_on_the_fused_mlp(name, oracle16):
    from scratchpad_amd import _native
    g, pfx, _, _ = apertus_oracle.load_case(name)
    gp = torch.from_numpy(g[pfx + "prefill_logits"])
    xi = dict(_native.XIELU_CALLS)
    prefill, decode, _, _ = apertus_oracle.run_case(name, torch.float16)
    # the prefill (15 rows) and the decode step (3 rows) both fit the skinny kernel: one launch per layer and step
    assert _native.XIELU_CALLS["gemm_skinny_xielu"] == xi["gemm_skinny_xielu"] + 4
    assert _native.XIELU_CALLS["two_call"] == xi["two_call"] and _native.XIELU_CALLS["xielu"] == xi["xielu"]
    o1, o2 = oracle16(name, torch.float16)
    for got, want, what in ((prefill, o1, "prefill"), (decode, o2, "decode")):
        assert rel(got, want) <= 1e-3, f"{name} {what}: relative logit deviation {rel(got, want):.2e} vs fp16 oracle"
    assert rel(prefill, gp) <= 5e-3


@pytest.mark.parametrize("name", ["a", "b"])
def test_tiny_apertus_bf16_and_graph_replay(name, oracle16):
    from scratchpad_amd import _native
    eager = apertus_oracle.run_case(name, torch.bfloat16)
    xi = dict(_native.XIELU_CALLS)
    graph = apertus_oracle.run_case(name, torch.bfloat16, graph_bs=[2, 4])
    assert _native.XIELU_CALLS["two_call"] == xi["two_call"], "a graph bucket fell off the fused MLP launch"
    o1, o2 = oracle16(name, torch.bfloat16)
    for got, want, what in ((eager[0], o1, "prefill"), (eager[1], o2, "decode")):
        assert rel(got, want) <= 3e-2, f"{name} {what}: {rel(got, want):.2e} vs bf16 oracle"
    # graph replay (padded from bs 3 to the bs-4 bucket) computes the same thing as eager
    assert torch.allclose(graph[1], eager[1], atol=1e-2 * float(eager[1].abs().max()))
    assert torch.equal(graph[0], eager[0]), "prefill is eager in both runs"


def test_exchanged_activation_scalars_change_the_logits():
    """a checkpoint with the two layers' alpha_p and alpha_n exchanged: each layer applies its own pair"""
    _, _, _, w = apertus_oracle.load_case("a")
    swapped = dict(w)
    for s in ("alpha_p", "alpha_n"):
        l0, l1 = (f"model.layers.{i}.mlp.act_fn.{s}" for i in (0, 1))
        swapped[l0], swapped[l1] = w[l1], w[l0]
    base = apertus_oracle.run_case("a", torch.float32)
    other = apertus_oracle.run_case("a", torch.float32, w=swapped)
    want = apertus_oracle.oracle_run("a", w=swapped)[0]
    assert rel(other[0], base[0]) > 1e-3, "exchanging the layers' activation scalars left the logits where they were"
    assert rel(other[0], want) <= 1e-4, "the exchanged checkpoint does not follow the oracle run on the same weights"
