"""End-to-end parity of the hosted Llama-Quant-MoE decoders (ModelRunner -> ForwardBatch -> HipAttnBackend -> C ABI),
both variants, against tests/quant_moe_oracle.forward on the tiny model of tests/golden/tiny_llama_moe.npz case "a"
(hidden 128, inter 64, 2 layers, 4 experts top-2): the experts are ``pack_delta(fixture expert.float(), fp16)``, the
gate is the fixture's, the base MLP is drawn from ``torch.Generator().manual_seed(2)``
(tests/quant_moe_oracle.quant_weights).  The reference cannot run this model here (triteia is not part of its tree), so
the oracle is the two blocks' statements in plain torch.

With exactly this recipe the fp32 oracle's smallest router gap is 0.142 over the prefill and 0.82 over the decode step;
every test asserts ``>= 0.125`` on its own oracle run before it compares anything, so a 16-bit run cannot take another
expert and the tolerances - tests/test_gpu_llama_moe.py's - measure arithmetic."""
import pytest
import torch

from tests import moe_oracle, quant_moe_oracle as qo

pytestmark = pytest.mark.gpu
ARCHS = ("llama_quant_moe", "llama_naive_quant_moe")
TOL = {torch.float16: 1e-3, torch.bfloat16: 3e-2}
LAUNCHES = 4          # two layers x two steps


def rel(got, want):
    return float((got - want).abs().max() / want.abs().max())


def gap_holds(arch):
    _, _, t1, t2 = qo.oracle_run(arch)
    K = moe_oracle.load_case("a")[2].K
    gap = min(qo.router_gap(t1, K), qo.router_gap(t2, K))
    assert gap >= 0.125, f"{arch}: the fp32 oracle's smallest router gap is {gap:.3f}"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("arch", ARCHS)
def test_tiny_llama_quant_moe_eager_and_graph_replay(arch, dtype):
    from scratchpad_amd import _native
    gap_holds(arch)
    calls, moe = dict(_native.QMOE_CALLS), dict(_native.MOE_CALLS)
    eager = qo.run_case(arch, dtype)
    assert all(_native.QMOE_CALLS[k] == calls[k] + LAUNCHES for k in calls), "the packed expert kernels did not run"
    assert _native.MOE_CALLS["route"] == moe["route"] + LAUNCHES
    assert all(_native.MOE_CALLS[k] == moe[k] for k in ("gate_up", "down", "combine", "fallback"))
    o1, o2 = qo.oracle_run(arch, dtype)[:2]
    for got, want, what in ((eager[0], o1, "prefill"), (eager[1], o2, "decode")):
        print(f"[quant moe] {arch} {dtype} {what}: relative logit deviation {rel(got, want):.2e} (bar {TOL[dtype]:.0e})")
        assert rel(got, want) <= TOL[dtype], f"{arch} {what}: {rel(got, want):.2e} vs the {dtype} oracle"
    if dtype == torch.float16:
        assert rel(eager[0], qo.oracle_run(arch)[0]) <= 5e-3, "against the fp32 oracle"
    # graph replay (padded from bs 3 to the bs-4 bucket) computes the same thing as eager: the MoE part is batch
    # invariant, attention under the range geometry is not
    graph = qo.run_case(arch, dtype, graph_bs=[2, 4])
    assert all(_native.MOE_CALLS[k] == moe[k] for k in ("gate_up", "down", "combine", "fallback"))
    assert torch.allclose(graph[1], eager[1], atol=1e-2 * float(eager[1].abs().max()))
    assert torch.equal(graph[0], eager[0]), "prefill is eager in both runs"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_the_two_variants_differ_within_round_off(dtype):
    """on this fixture every token's two experts are added in one order or the other: a + b and b + a round alike, so
    the variants - same routing, same kernels - give the same logits; the oracle's variants differ by their own
    round-off only"""
    for arch in ARCHS:
        gap_holds(arch)
    a, b = qo.run_case(ARCHS[0], dtype), qo.run_case(ARCHS[1], dtype)
    for x, y, what in ((a[0], b[0], "prefill"), (a[1], b[1], "decode")):
        assert rel(x, y) <= TOL[dtype], f"{what}: {rel(x, y):.2e}"
    oa, ob = qo.oracle_run(ARCHS[0], dtype), qo.oracle_run(ARCHS[1], dtype)
    assert rel(oa[0], ob[0]) <= TOL[dtype]


@pytest.mark.parametrize("arch", ARCHS)
def test_exchanged_experts_change_the_logits_and_follow_the_oracle(arch):
    """a checkpoint with experts 0 and 2 of layer 0 exchanged, gate rows left alone: each slot applies its own packed
    weights.  (This exchange keeps the fp32 oracle's router gap at 0.142 / 0.756 - scanned on the CPU; exchanging 0 and
    1 brings layer 1's down to 0.064.)"""
    gap_holds(arch)
    _, _, shape, w0 = moe_oracle.load_case("a")
    swapped = qo.swap_experts(qo.quant_weights(w0, shape), layer=0, a=0, b=2)
    fp32 = qo.oracle_run(arch, w=swapped)
    gap = min(qo.router_gap(fp32[2], shape.K), qo.router_gap(fp32[3], shape.K))
    assert gap >= 0.125, f"the exchanged run's smallest router gap is {gap:.3f}"
    dtype = torch.float16
    base = qo.run_case(arch, dtype)
    other = qo.run_case(arch, dtype, w=swapped)
    want = qo.oracle_run(arch, dtype, w=swapped)
    assert rel(other[0], base[0]) > 10 * TOL[dtype], "exchanging two experts left the logits where they were"
    assert rel(other[0], want[0]) <= TOL[dtype], "the exchanged checkpoint does not follow the oracle on the same weights"
