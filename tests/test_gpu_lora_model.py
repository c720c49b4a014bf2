"""LoRA toppings through the whole Llama path: ModelRunner + ToppingsManager + topping layers + HIP graph.

The tiny Llama of tests/golden/tiny_llama.npz (case "b": hidden 256, 2 layers) in fp16, two seeded random adapters
(r 8, lora_alpha 16) on all four projections of every layer, a batch of four requests with toppings [a, None, b, a]:
extend, then two decode steps.  The oracle is the existing CPU Llama oracle in fp32 on weights with a request's adapter
merged in fp32 (W + scale * B A in PEFT orientation = W + scale (A B)^T in buffer orientation), from the same stored
fp16 values.  Tolerance: what tests/test_gpu_llama.py applies to its fp16 run against the golden fp32 logits, 5e-3 of
the logit scale."""
import pytest
import torch

from oracle import llama as ollama
from oracle import ops
from tests import smoke_impl

pytestmark = pytest.mark.gpu

DTYPE = torch.float16
EXT = [5, 9, 1, 3]
REQ = [2, 0, 3, 1]
PATHS = ["a", None, "b", "a"]
R, ALPHA = 8, 16
TOL = 5e-3


def adapter_state(shape, seed):
    g = torch.Generator().manual_seed(seed)
    D = shape.D
    dims = {"q_proj": (shape.hidden, shape.Hq * D), "k_proj": (shape.hidden, shape.Hkv * D),
            "v_proj": (shape.hidden, shape.Hkv * D), "o_proj": (shape.Hq * D, shape.hidden),
            "gate_proj": (shape.hidden, shape.inter), "up_proj": (shape.hidden, shape.inter),
            "down_proj": (shape.inter, shape.hidden)}
    sd = {}
    for layer in range(shape.layers):
        for t, (din, dout) in dims.items():
            block = "self_attn" if t in ("q_proj", "k_proj", "v_proj", "o_proj") else "mlp"
            base = f"base_model.model.model.layers.{layer}.{block}.{t}"
            sd[base + ".lora_A.weight"] = (torch.randn(R, din, generator=g) * 0.05).to(DTYPE)
            sd[base + ".lora_B.weight"] = (torch.randn(dout, R, generator=g) * 0.05).to(DTYPE)
    return sd


def merged_weights(w16, sd, layers):
    """fp32 weights of the base model (stored fp16 values) with the adapter merged in fp32"""
    w = {k: v.float().clone() for k, v in w16.items()}
    if sd is None:
        return w
    scale = ALPHA / R
    for layer in range(layers):
        def delta(block, t):
            base = f"base_model.model.model.layers.{layer}.{block}.{t}"
            return scale * (sd[base + ".lora_B.weight"].float() @ sd[base + ".lora_A.weight"].float())
        p = f"model.layers.{layer}."
        w[p + "self_attn.qkv_proj.weight"] += torch.cat([delta("self_attn", t) for t in ("q_proj", "k_proj", "v_proj")], 0)
        w[p + "self_attn.o_proj.weight"] += delta("self_attn", "o_proj")
        w[p + "mlp.gate_up_proj.weight"] += torch.cat([delta("mlp", t) for t in ("gate_proj", "up_proj")], 0)
        w[p + "mlp.down_proj.weight"] += delta("mlp", "down_proj")
    return w


class Flow:
    """the token ids, pool rows and KV slots of the three steps (the scheduler's part), shared by every run"""

    def __init__(self, shape):
        g = torch.Generator().manual_seed(77)
        self.ext = torch.tensor(EXT, dtype=torch.int32)
        self.req = torch.tensor(REQ, dtype=torch.int64)
        n = int(self.ext.sum())
        perm = torch.randperm(60, generator=g) + 1
        self.loc = perm[:n].to(torch.int64)
        self.dloc = [perm[n + 4 * i:n + 4 * (i + 1)].to(torch.int64) for i in range(2)]
        self.ids = torch.randint(0, shape.vocab, (n,), generator=g)
        self.next_ids = [torch.randint(0, shape.vocab, (4,), generator=g) for _ in range(2)]


def make_runner(shape, w16, adapters=None, graph_bs=None, slots=2):
    from scratchpad_amd.model_runner import ModelConfig, ModelRunner, ServerArgs
    from scratchpad_amd.toppings import LoRAAdapter, ToppingConfig
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
    # the documented entry: ModelRunner(..., toppings=[adapters]) wraps the projections in the constructor, and the
    # checkpoint is loaded afterwards by the project's usual loader, through the wrappers
    ads = None
    if adapters:
        conf = lambda u: ToppingConfig("lora", u, {"r": R, "lora_alpha": ALPHA, "target_modules": [
            "q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"]})
        ads = [LoRAAdapter(u, conf(u), cfg).initialize_weights(sd) for u, sd in adapters.items()]
    mr = ModelRunner(cfg, args, dtype=DTYPE, init_weights=False, toppings=ads)
    assert (mr.topping_manager is not None) == bool(adapters)
    mr.model.load_full_state_dict({k: v.to(mr.device) for k, v in w16.items()})
    if graph_bs is not None:
        mr.init_cuda_graphs()
    return mr


def run_flow(mr, flow, paths, between_decodes=None):
    """extend + two decode steps; returns the three logits matrices (fp32, CPU)"""
    from scratchpad_amd import _native
    from scratchpad_amd.forward_info import ForwardMode, ModelWorkerBatch
    from scratchpad_amd.model_runner import TpModelWorker
    worker, dev = TpModelWorker(mr), mr.device
    req, loc, seq = flow.req.to(dev), flow.loc.to(dev), flow.ext.long().to(dev)
    _native.write_req_to_token(mr.req_to_token_pool.req_to_token, req, torch.zeros_like(seq), seq, seq, loc)
    batch = ModelWorkerBatch(bid=1, forward_mode=ForwardMode.EXTEND, input_ids=flow.ids.to(dev), req_pool_indices=req,
                             seq_lens=seq, out_cache_loc=loc, seq_lens_sum=int(flow.ext.sum()),
                             extend_num_tokens=int(flow.ext.sum()), extend_seq_lens=flow.ext.tolist(),
                             extend_prefix_lens=[0] * 4, toppings_paths=paths)
    out, _ = worker.forward_batch_generation(batch, skip_sample=True)
    logits = [out.next_token_logits.float().cpu()]
    for step in range(2):
        if step == 1 and between_decodes is not None:
            between_decodes(mr)
        dloc = flow.dloc[step].to(dev)
        mr.req_to_token_pool.write((req, seq), dloc.to(torch.int32))
        seq = seq + 1
        b = ModelWorkerBatch(bid=2 + step, forward_mode=ForwardMode.DECODE, input_ids=flow.next_ids[step].to(dev),
                             req_pool_indices=req, seq_lens=seq, out_cache_loc=dloc, seq_lens_sum=int(seq.sum()),
                             toppings_paths=paths)
        out, _ = worker.forward_batch_generation(b, skip_sample=True)
        logits.append(out.next_token_logits.float().cpu())
    torch.cuda.synchronize()
    return logits


def oracle_flow(shape, w, flow):
    kv = ollama.OracleKV(shape, 96, 9, 64, torch.float32)
    ext, req = flow.ext, flow.req
    pre = torch.zeros_like(ext)
    ops.write_req_to_token(kv.req_to_token, req, pre, ext, ext, flow.loc)
    positions, start = ops.compute_position(pre, ext)
    out = [ollama.forward(shape, w, kv, mode="extend", input_ids=flow.ids, positions=positions, req_pool_indices=req,
                          seq_lens=ext.long(), out_cache_loc=flow.loc, extend_seq_lens=ext, extend_start_loc=start)]
    seq = ext.long()
    for step in range(2):
        seq2 = seq + 1
        ops.write_req_to_token(kv.req_to_token, req, seq, seq2, torch.ones_like(seq2), flow.dloc[step])
        out.append(ollama.forward(shape, w, kv, mode="decode", input_ids=flow.next_ids[step],
                                  positions=ops.clamp_position(seq2), req_pool_indices=req, seq_lens=seq2,
                                  out_cache_loc=flow.dloc[step]))
        seq = seq2
    return out


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
    c0 = dict(_native.LORA_CALLS)
    ns["eager"] = run_flow(eager, flow, PATHS)
    ns["eager_calls"] = {k: _native.LORA_CALLS[k] - c0[k] for k in c0}
    ns["oracle"] = {u: oracle_flow(shape, merged_weights(w16, sds.get(u), shape.layers), flow) for u in ("a", "b", None)}
    return ns


def test_every_request_follows_its_own_adapter(world):
    """(i) per request: logits against the oracle on weights with THAT request's adapter merged"""
    assert world["eager_calls"] == {"shrink": 3 * 4 * world["shape"].layers, "expand": 3 * 5 * world["shape"].layers}, \
        "per layer and step: 4 shrinks and 5 expands (qkv takes two)"
    worst = []
    for step, what in enumerate(("extend", "decode 1", "decode 2")):
        for i, u in enumerate(PATHS):
            want, got = world["oracle"][u][step][i], world["eager"][step][i]
            dev = float((got - want).abs().max() / world["oracle"][u][step].abs().max())
            print(f"[lora model] {what} request {i} ({u}): relative logit deviation {dev:.2e} (bound {TOL})")
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
    c0 = dict(_native.LORA_CALLS)
    base = run_flow(plain, world["flow"], [None] * 4)
    assert _native.LORA_CALLS == c0, "no manager: no topping launch"
    assert torch.equal(world["eager"][0][1], base[0][1])
    skipped = run_flow(world["eager_runner"], world["flow"], [None] * 4)
    assert _native.LORA_CALLS["shrink"] > c0["shrink"], "the kernels ran, with every row skipped"
    for step in range(3):
        assert torch.equal(world["eager"][step][1], skipped[step][1]), f"step {step}"
    # and a manager with every row at -1 computes what the base model computes
    for step in range(3):
        dev = float((skipped[step] - base[step]).abs().max() / base[step].abs().max())
        assert dev <= 1e-3, (step, dev)
    assert torch.equal(skipped[0], base[0])


def test_graph_replay_equals_eager_and_follows_a_slot_swap(world):
    """(iii) replay == eager bit for bit, the kernels having run at capture; (iv) adapter b loaded into a's slot
    between two replays is picked up without recapturing, and equals an eager run with the same slot contents"""
    from scratchpad_amd import _native
    c0 = dict(_native.LORA_CALLS)
    gr = make_runner(world["shape"], world["w16"], world["sds"], graph_bs=[4])
    layers = world["shape"].layers
    assert _native.LORA_CALLS["shrink"] - c0["shrink"] == 3 * 4 * layers, "2 warm-up runs + the captured one"
    assert _native.LORA_CALLS["expand"] - c0["expand"] == 3 * 5 * layers
    c1 = dict(_native.LORA_CALLS)
    got = run_flow(gr, world["flow"], PATHS)
    assert _native.LORA_CALLS["shrink"] - c1["shrink"] == 4 * layers, "only the eager extend launches from the host"
    for step in range(3):
        assert torch.equal(got[step], world["eager"][step]), f"step {step}: replay differs from eager"

    def swap(mr):
        tm = mr.topping_manager
        tm.load_topping("b", tm.buffer_id["a"])

    swapped_graph = run_flow(gr, world["flow"], PATHS, between_decodes=swap)
    swapped_eager = run_flow(world["eager_runner"], world["flow"], PATHS, between_decodes=swap)
    # (restore slot contents for whoever uses the shared eager runner next)
    tm = world["eager_runner"].topping_manager
    tm.load_topping("a", tm.buffer_id["a"])
    assert torch.equal(swapped_graph[1], got[1]) and torch.equal(swapped_graph[2], swapped_eager[2])
    assert not torch.equal(swapped_graph[2][0], got[2][0]), "rows of a follow the new slot contents"
    assert torch.equal(swapped_graph[2][1], got[2][1]) and torch.equal(swapped_graph[2][2], got[2][2]), \
        "the base-model row and the row of b do not"


def test_padded_bucket_leaves_no_trace(world):
    """(v) four requests replayed in the bs-8 bucket: the live rows equal the unpadded eager run"""
    gr = make_runner(world["shape"], world["w16"], world["sds"], graph_bs=[8])
    # leave slot numbers behind in the rows that will be padding
    gr.topping_manager.weight_indices[:8].fill_(1)
    got = run_flow(gr, world["flow"], PATHS)
    assert gr.topping_manager.weight_indices[4:8].tolist() == [-1] * 4
    for step in range(3):
        assert torch.equal(got[step], world["eager"][step]), f"step {step}"
