"""End-to-end parity of the hosted Qwen3 decoder (ModelRunner -> ForwardBatch -> HipAttnBackend -> C ABI) against the
logits of the reference's own Qwen3ForCausalLM (tests/golden/tiny_qwen3.npz), at the bars tests/test_gpu_llama.py holds
Llama to.  Variant a has an explicit head_dim of 128 over hidden 256 (q_size 512), variant b head_dim 64 and a tied
head; both run the fused per-head norm + rotary + KV-store launch (sp_qk_norm_rotary) in every layer."""
import pytest
import torch

from tests import qwen3_oracle

pytestmark = pytest.mark.gpu


def rel(got, want):
    return float((got - want).abs().max() / want.abs().max())


@pytest.fixture(scope="module")
def oracle16():
    """the oracle evaluated in fp16 / bf16, once per (variant, dtype)"""
    cache = {}

    def get(name, dtype):
        if (name, dtype) not in cache:
            cache[name, dtype] = qwen3_oracle.oracle_run(name, dtype)[:2]
        return cache[name, dtype]
    return get


@pytest.mark.parametrize("name", ["a", "b"])
def test_tiny_qwen3_fp32_matches_reference_logits(name):
    from scratchpad_amd import _native
    g, pfx, _, _ = qwen3_oracle.load_case(name)
    gp, gd, gn = (torch.from_numpy(g[pfx + k]) for k in ("prefill_logits", "decode_logits", "next_ids"))
    before = dict(_native.QK_NORM_CALLS)
    prefill, decode, nxt, mr = qwen3_oracle.run_case(name, torch.float32)
    assert _native.QK_NORM_CALLS["fused"] == before["fused"] + 4, "two layers x two steps of the fused launch"
    assert _native.QK_NORM_CALLS["three_launch"] == before["three_launch"]
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
def test_tiny_qwen3_fp16_within_1e3(name, oracle16):
    g, pfx, _, _ = qwen3_oracle.load_case(name)
    gp = torch.from_numpy(g[pfx + "prefill_logits"])
    prefill, decode, _, _ = qwen3_oracle.run_case(name, torch.float16)
    o1, o2 = oracle16(name, torch.float16)
    for got, want, what in ((prefill, o1, "prefill"), (decode, o2, "decode")):
        assert rel(got, want) <= 1e-3, f"{name} {what}: relative logit deviation {rel(got, want):.2e} vs fp16 oracle"
    assert rel(prefill, gp) <= 5e-3


@pytest.mark.parametrize("name", ["a", "b"])
def test_tiny_qwen3_bf16_and_graph_replay(name, oracle16):
    eager = qwen3_oracle.run_case(name, torch.bfloat16)
    graph = qwen3_oracle.run_case(name, torch.bfloat16, graph_bs=[2, 4])
    o1, o2 = oracle16(name, torch.bfloat16)
    for got, want, what in ((eager[0], o1, "prefill"), (eager[1], o2, "decode")):
        assert rel(got, want) <= 3e-2, f"{name} {what}: {rel(got, want):.2e} vs bf16 oracle"
    # graph replay (padded from bs 3 to the bs-4 bucket) computes the same thing as eager
    assert torch.allclose(graph[1], eager[1], atol=1e-2 * float(eager[1].abs().max()))
    assert torch.equal(graph[0], eager[0]), "prefill is eager in both runs"


@pytest.mark.parametrize("name", ["a", "b"])
def test_fused_and_reference_order_give_the_same_bits(name):
    """fused_rope_kv_store on (one launch) and off (the reference's order: norm, norm, rotary, attention with store):
    the kernel's contract seen from the model"""
    fused = qwen3_oracle.run_case(name, torch.float16, fused=True)
    plain = qwen3_oracle.run_case(name, torch.float16, fused=False)
    assert torch.equal(fused[0], plain[0]), "prefill logits differ"
    assert torch.equal(fused[1], plain[1]), "decode logits differ"
    for layer in range(2):
        for a, b in zip(fused[3].token_to_kv_pool.get_kv_buffer(layer), plain[3].token_to_kv_pool.get_kv_buffer(layer)):
            assert torch.equal(a, b), f"layer {layer}: the pools differ"


def test_swapped_norm_weights_change_the_logits():
    """a checkpoint with q_norm and k_norm exchanged: both weights are loaded, and each is applied to its own side"""
    _, _, _, w = qwen3_oracle.load_case("a")
    swapped = dict(w)
    for i in range(2):
        qn, kn = (f"model.layers.{i}.self_attn.{s}_norm.weight" for s in "qk")
        swapped[qn], swapped[kn] = w[kn], w[qn]
    base = qwen3_oracle.run_case("a", torch.float32)
    other = qwen3_oracle.run_case("a", torch.float32, w=swapped)
    want = qwen3_oracle.oracle_run("a", w=swapped)[0]
    assert rel(other[0], base[0]) > 1e-3, "swapping q_norm and k_norm left the logits where they were"
    assert rel(other[0], want) <= 1e-4, "the swapped checkpoint does not follow the oracle run on the same weights"
