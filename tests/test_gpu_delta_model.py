"""Delta toppings through the whole Llama path: ModelRunner + ToppingsManager + topping layers + HIP graph.

The tiny Llama of tests/golden/tiny_llama.npz (case "b": hidden 256, inter 320, 2 layers) in fp16, two seeded random
delta adapters (4-bit, 2:4) on all four projections of every layer, a batch of four requests with toppings
[a, None, b, a]: extend, then two decode steps (the flow of tests/test_gpu_lora_model.py).  The oracle is the existing
CPU Llama oracle in fp32 on W + unpack(delta), from the same stored fp16 weights and the same packed tensors.
Tolerance: what tests/test_gpu_llama.py applies to its fp16 run against the golden fp32 logits, 5e-3 of the logit
scale."""
import pytest
import torch

from tests import smoke_impl
from tests.test_gpu_lora_model import PATHS, TOL, Flow, oracle_flow, run_flow

pytestmark = pytest.mark.gpu

DTYPE = torch.float16
PROJ = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")


def adapter_state(shape, seed):
    """packed tensors under the names DeltaAdapter.initialize_weights reads"""
    from scratchpad_amd.delta import pack_delta
    g = torch.Generator().manual_seed(seed)
    D = shape.D
    dims = {"q_proj": (shape.Hq * D, shape.hidden), "k_proj": (shape.Hkv * D, shape.hidden),
            "v_proj": (shape.Hkv * D, shape.hidden), "o_proj": (shape.hidden, shape.Hq * D),
            "gate_proj": (shape.inter, shape.hidden), "up_proj": (shape.inter, shape.hidden),
            "down_proj": (shape.hidden, shape.inter)}
    sd = {}
    for layer in range(shape.layers):
        for t in PROJ:
            block = "self_attn" if t in PROJ[:4] else "mlp"
            packed = pack_delta(torch.randn(dims[t], generator=g) * 0.02, DTYPE)
            for k, v in zip(("codes", "meta", "scales"), packed):
                sd[f"model.layers.{layer}.{block}.{t}.{k}"] = v
    return sd


def merged_weights(w16, sd, layers):
    """fp32 weights of the base model (stored fp16 values) plus the unpacked delta of the adapter"""
    from scratchpad_amd.delta import unpack_delta
    w = {k: v.float().clone() for k, v in w16.items()}
    if sd is None:
        return w
    for layer in range(layers):
        def delta(block, t):
            base = f"model.layers.{layer}.{block}.{t}"
            return unpack_delta(sd[base + ".codes"], sd[base + ".meta"], sd[base + ".scales"])
        p = f"model.layers.{layer}."
        w[p + "self_attn.qkv_proj.weight"] += torch.cat([delta("self_attn", t) for t in ("q_proj", "k_proj", "v_proj")], 0)
        w[p + "self_attn.o_proj.weight"] += delta("self_attn", "o_proj")
        w[p + "mlp.gate_up_proj.weight"] += torch.cat([delta("mlp", t) for t in ("gate_proj", "up_proj")], 0)
        w[p + "mlp.down_proj.weight"] += delta("mlp", "down_proj")
    return w


def make_runner(shape, w16, adapters=None, graph_bs=None, slots=2):
    from scratchpad_amd.model_runner import ModelConfig, ModelRunner, ServerArgs
    from scratchpad_amd.toppings import DeltaAdapter, ToppingConfig
    scaling = None
    if shape.rope_scaling is not None:
        f = shape.rope_scaling
        scaling = {"rope_type": "llama3", "factor": f[0], "low_freq_factor": f[1], "high_freq_factor": f[2],
                   "original_max_position_embeddings": int(f[3])}
    cfg = ModelConfig(shape.hidden, shape.inter, shape.layers, shape.Hq, shape.Hkv, shape.vocab, context_len=60,
                      rms_norm_eps=shape.rms_eps, rope_theta=shape.rope_theta, rope_scaling=scaling,
                      max_position_embeddings=shape.max_pos, tie_word_embeddings=shape.tie)
    args = ServerArgs(max_total_tokens=96, max_running_requests=8, disable_cuda_graph=graph_bs is None,
                      cuda_graph_bs=graph_bs, max_toppings_per_batch=slots if adapters else None)
    ads = None
    if adapters:
        conf = lambda u: ToppingConfig("delta", u, {"compress_config": {"bits": 4, "sparsity": 0.5}})
        ads = [DeltaAdapter(u, conf(u), cfg).initialize_weights(sd) for u, sd in adapters.items()]
    mr = ModelRunner(cfg, args, dtype=DTYPE, init_weights=False, toppings=ads)
    assert (mr.topping_manager is not None) == bool(adapters)
    mr.model.load_full_state_dict({k: v.to(mr.device) for k, v in w16.items()})
    if graph_bs is not None:
        mr.init_cuda_graphs()
    return mr


@pytest.fixture(scope="module")
def world():
    from scratchpad_amd import _native
    _, _, shape, w = smoke_impl.load_case("b")
    w16 = {k: v.to(DTYPE) for k, v in w.items()}
    sds = {"a": adapter_state(shape, 1), "b": adapter_state(shape, 2)}
    flow = Flow(shape)
    ns = dict(shape=shape, w16=w16, sds=sds, flow=flow)
    eager = make_runner(shape, w16, sds)
    ns["eager_runner"] = eager
    c0 = dict(_native.DELTA_CALLS)
    ns["eager"] = run_flow(eager, flow, PATHS)
    ns["eager_calls"] = {k: _native.DELTA_CALLS[k] - c0[k] for k in c0}
    ns["oracle"] = {u: oracle_flow(shape, merged_weights(w16, sds.get(u), shape.layers), flow) for u in ("a", "b", None)}
    return ns


def test_every_request_follows_its_own_adapter(world):
    """(i) per request: logits against the oracle on weights with THAT request's delta added"""
    assert world["eager_calls"] == {"group": 3, "mm": 3 * 4 * world["shape"].layers}, \
        "per step one grouping, per layer 4 products"
    worst = []
    for step, what in enumerate(("extend", "decode 1", "decode 2")):
        for i, u in enumerate(PATHS):
            want, got = world["oracle"][u][step][i], world["eager"][step][i]
            dev = float((got - want).abs().max() / world["oracle"][u][step].abs().max())
            print(f"[delta model] {what} request {i} ({u}): relative logit deviation {dev:.2e} (bound {TOL})")
            worst.append((dev, what, i, u))
            # ... and the adapters matter: another adapter's oracle is far outside the tolerance
            for other in ("a", "b", None):
                if other != u:
                    far = float((got - world["oracle"][other][step][i]).abs().max() / world["oracle"][u][step].abs().max())
                    assert far > 4 * TOL, f"{what} request {i}: adapter {u} cannot be told from {other} ({far:.2e})"
    top = max(worst, key=lambda t: t[0])
    assert top[0] <= TOL, f"largest deviation (value, step, request, adapter): {top}"


def test_base_model_rows_are_untouched_bit_for_bit(world):
    """(ii) the None request.  Extend (18 rows: the same base path with and without a manager): bit-identical to a
    runner built WITHOUT a manager.  Decode: a runner without a manager takes the fused gate_up + SiLU launch at
    these row counts, which a layer with toppings must not, so the base path differs; there the comparison is
    against the same runner with every row at -1."""
    from scratchpad_amd import _native
    plain = make_runner(world["shape"], world["w16"])
    c0 = dict(_native.DELTA_CALLS)
    base = run_flow(plain, world["flow"], [None] * 4)
    assert _native.DELTA_CALLS == c0, "no manager: no topping launch"
    assert torch.equal(world["eager"][0][1], base[0][1])
    skipped = run_flow(world["eager_runner"], world["flow"], [None] * 4)
    assert _native.DELTA_CALLS["mm"] > c0["mm"], "the kernels ran, with every row skipped"
    for step in range(3):
        assert torch.equal(world["eager"][step][1], skipped[step][1]), f"step {step}"
    for step in range(3):
        dev = float((skipped[step] - base[step]).abs().max() / base[step].abs().max())
        assert dev <= 1e-3, (step, dev)
    assert torch.equal(skipped[0], base[0])


def test_graph_replay_equals_eager_and_follows_a_slot_swap(world):
    """(iii) replay == eager bit for bit, the kernels - the grouping included - having run at capture; (iv) adapter b
    loaded into a's slot between two replays is picked up without recapturing, and equals an eager run with the same
    slot contents"""
    from scratchpad_amd import _native
    c0 = dict(_native.DELTA_CALLS)
    gr = make_runner(world["shape"], world["w16"], world["sds"], graph_bs=[4])
    layers = world["shape"].layers
    assert _native.DELTA_CALLS["group"] - c0["group"] == 3, "2 warm-up runs + the captured one"
    assert _native.DELTA_CALLS["mm"] - c0["mm"] == 3 * 4 * layers
    c1 = dict(_native.DELTA_CALLS)
    got = run_flow(gr, world["flow"], PATHS)
    assert _native.DELTA_CALLS["group"] - c1["group"] == 1 and _native.DELTA_CALLS["mm"] - c1["mm"] == 4 * layers, \
        "only the eager extend launches from the host"
    for step in range(3):
        assert torch.equal(got[step], world["eager"][step]), f"step {step}: replay differs from eager"

    def swap(mr):
        tm = mr.topping_manager
        tm.load_topping("b", tm.buffer_id["a"])

    swapped_graph = run_flow(gr, world["flow"], PATHS, between_decodes=swap)
    swapped_eager = run_flow(world["eager_runner"], world["flow"], PATHS, between_decodes=swap)
    tm = world["eager_runner"].topping_manager
    tm.load_topping("a", tm.buffer_id["a"])          # (restore the slot for whoever uses the shared runner next)
    assert torch.equal(swapped_graph[1], got[1]) and torch.equal(swapped_graph[2], swapped_eager[2])
    assert not torch.equal(swapped_graph[2][0], got[2][0]), "rows of a follow the new slot contents"
    assert torch.equal(swapped_graph[2][1], got[2][1]) and torch.equal(swapped_graph[2][2], got[2][2]), \
        "the base-model row and the row of b do not"


def test_padded_bucket_leaves_no_trace(world):
    """(v) four requests replayed in the bs-8 bucket: the live rows equal the unpadded eager run"""
    gr = make_runner(world["shape"], world["w16"], world["sds"], graph_bs=[8])
    gr.topping_manager.weight_indices[:8].fill_(1)   # slot numbers left behind in the rows that will be padding
    got = run_flow(gr, world["flow"], PATHS)
    assert gr.topping_manager.weight_indices[4:8].tolist() == [-1] * 4
    for step in range(3):
        assert torch.equal(got[step], world["eager"][step]), f"step {step}"
