"""Fixture access and the ModelRunner flow of tests/golden/tiny_embedding.npz (TEST INFRASTRUCTURE ONLY)."""
import torch

from tests import golden

DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
_FIXTURE = None


def fixture():
    global _FIXTURE
    if _FIXTURE is None:
        _FIXTURE = golden.load("tiny_embedding")
    return _FIXTURE


def from_bits(a, dtype):
    """a recorded result: 16-bit ones are stored as their bit patterns"""
    t = torch.from_numpy(a)
    return t if dtype == torch.float32 else t.view(dtype)


def pooler_case(H, name):
    """(x [T, H] in the dtype, lens int32, the reference Pooler's rows) of the fixture"""
    g = fixture()
    dt = DTYPES[name]
    return (torch.from_numpy(g[f"pool_{H}_x"]).to(dt), torch.from_numpy(g["pool_lens"]),
            from_bits(g[f"pool_{name}_{H}_out"], dt))


def pool_lens(B):
    """ragged lengths of the kernel tests, with sequences of one token"""
    return [1 + (5 * i + 2) % 4 for i in range(B)] if B > 1 else [1]


def pool_inputs(H, B, dtype):
    """the seeded (x [T, H], residual [T, H], norm weight [H], lengths) of the kernel tests, on the host"""
    lens = pool_lens(B)
    T = sum(lens)
    g = torch.Generator().manual_seed(17 * H + B)
    x = torch.randn(T, H, generator=g).to(dtype)
    res = torch.randn(T, H, generator=g).to(dtype)
    w = (1.0 + 0.1 * torch.randn(H, generator=g)).to(dtype)
    return x, res, w, lens


def model_case(name):
    """(fixture, prefix, ModelConfig, weights) of "llama" (LlamaEmbeddingModel) or "qwen3" (get_embedding)"""
    from scratchpad_amd.model_runner import ModelConfig
    g, pfx = fixture(), name + "_"
    hidden, inter, nl, Hq, Hkv, vocab, _tie, D = (int(x) for x in g[pfx + "cfg"])
    cfg = ModelConfig(hidden, inter, nl, Hq, Hkv, vocab, context_len=60, head_dim=D,
                      rms_norm_eps=float(g[pfx + "rms_eps"]), rope_theta=float(g[pfx + "rope_theta"]),
                      max_position_embeddings=int(g[pfx + "max_pos"]),
                      architecture="llama_embedding" if name == "llama" else "qwen3", is_embedding=name != "llama")
    w = {k[len(pfx) + 3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith(pfx + "w::")}
    return g, pfx, cfg, w


def make_runner(name, dtype, generation=False):
    """a ModelRunner over the fixture's weights; generation=True: the same checkpoint served for generation (qwen3, or
    the Llama decoder under LlamaForCausalLM with a seeded LM head)"""
    import dataclasses
    from scratchpad_amd.model_runner import ModelRunner, ServerArgs
    g, pfx, cfg, w = model_case(name)
    if generation:
        cfg = dataclasses.replace(cfg, architecture="llama" if name == "llama" else "qwen3", is_embedding=False)
        if name == "llama":
            w = dict(w, **{"lm_head.weight": w["model.embed_tokens.weight"].flip(0).contiguous()})
    mr = ModelRunner(cfg, ServerArgs(max_total_tokens=96, max_running_requests=3, disable_cuda_graph=True), dtype=dtype,
                     init_weights=False)
    mr.model.load_full_state_dict({k: v.to(mr.device) for k, v in w.items()})
    return mr


def extend_batch(mr, ids, lens, req, loc, prefix=None, bid=1):
    """the ModelWorkerBatch of a ragged prefill, req_to_token written as the scheduler would"""
    from scratchpad_amd import _native
    from scratchpad_amd.forward_info import ForwardMode, ModelWorkerBatch
    dev = mr.device
    prefix = prefix or [0] * len(lens)
    ext = torch.tensor(lens, dtype=torch.int64, device=dev)
    pre = torch.tensor(prefix, dtype=torch.int64, device=dev)
    req, loc, ids = req.to(dev), loc.to(dev), ids.to(dev)
    _native.write_req_to_token(mr.req_to_token_pool.req_to_token, req, pre, pre + ext, ext, loc)
    return ModelWorkerBatch(bid=bid, forward_mode=ForwardMode.EXTEND, input_ids=ids, req_pool_indices=req,
                            seq_lens=pre + ext, out_cache_loc=loc, seq_lens_sum=int(sum(lens) + sum(prefix)),
                            extend_num_tokens=int(sum(lens)), extend_seq_lens=list(lens),
                            extend_prefix_lens=list(prefix))


def fixture_batch(mr, name):
    g, pfx, _, _ = model_case(name)
    return extend_batch(mr, torch.from_numpy(g[pfx + "input_ids"]), g[pfx + "extend_lens"].tolist(),
                        torch.from_numpy(g[pfx + "req_pool_indices"]), torch.from_numpy(g[pfx + "out_cache_loc"]))
