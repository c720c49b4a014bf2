"""CPU oracle of the Qwen3 decoder and the fixture flow of tests/golden/tiny_qwen3.npz (TEST INFRASTRUCTURE ONLY).

A plain-torch restatement of nn/models/qwen/qwen3.py as the reference hosts it: the Llama layer of oracle/llama.py
with an explicit head_dim and ``_apply_qk_norm`` (qwen3.py:114-123: RMSNorm.forward_native on the [T*H, head_dim] rows
of q and of k, each with its own weight) between qkv_proj and the rotary embedding.  Pinned by tiny_qwen3.npz, the
logits of the reference's own ``Qwen3ForCausalLM`` (tests/test_qwen3_host.py).

``run_case`` drives the same fixture through ModelRunner -> HipAttnBackend (GPU tests only)."""
from dataclasses import dataclass
from typing import Dict, Optional

import torch

from oracle import ops
from oracle.llama import OracleKV
from tests import golden


@dataclass
class Qwen3Shape:
    hidden: int
    inter: int
    layers: int
    Hq: int
    Hkv: int
    vocab: int
    D: int                          # explicit head_dim: Hq * D need not equal hidden
    tie: bool = False
    rope_theta: float = 1000000.0
    max_pos: int = 32768
    rms_eps: float = 1e-6


def qk_norm(q: torch.Tensor, k: torch.Tensor, q_weight: torch.Tensor, k_weight: torch.Tensor, eps: float, D: int):
    """Qwen3Attention._apply_qk_norm - qwen3.py:114-123.  q: [T, Hq*D], k: [T, Hkv*D]; returns new (q, k)."""
    qn = ops.rmsnorm(q.reshape(-1, D), q_weight, eps).view(q.shape)
    kn = ops.rmsnorm(k.reshape(-1, D), k_weight, eps).view(k.shape)
    return qn, kn


def qk_norm_rotary(positions, q, k, q_weight, k_weight, eps, D, cos_sin_cache, is_neox=True):
    """_apply_qk_norm followed by RotaryEmbedding.forward_native (qwen3.py:133-134).  Returns new (q, k)."""
    q, k = qk_norm(q, k, q_weight, k_weight, eps, D)
    return ops.rotary_embedding(positions, q, k, D, cos_sin_cache, is_neox)


def forward(shape: Qwen3Shape, w: Dict[str, torch.Tensor], kv: OracleKV, *, mode: str, input_ids, positions,
            req_pool_indices, seq_lens, out_cache_loc, extend_seq_lens: Optional[torch.Tensor] = None,
            extend_start_loc: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One forward pass (qwen3.py:125-137, 180-202, 268-283 and Qwen2Model.forward); next-token logits [bs, vocab]
    fp32.  Arguments as oracle.llama.forward."""
    dtype = w["model.embed_tokens.weight"].dtype
    D, Hq, Hkv = shape.D, shape.Hq, shape.Hkv
    cache = ops.rope_cos_sin_cache(shape.max_pos, shape.rope_theta, D, None, dtype)
    scale = D ** -0.5
    h = torch.nn.functional.embedding(input_ids, w["model.embed_tokens.weight"])
    residual = None
    for i in range(shape.layers):
        p = f"model.layers.{i}."
        if residual is None:
            residual = h
            h = ops.rmsnorm(h, w[p + "input_layernorm.weight"], shape.rms_eps)
        else:
            h, residual = ops.rmsnorm(h, w[p + "input_layernorm.weight"], shape.rms_eps, residual)
        qkv = torch.nn.functional.linear(h, w[p + "self_attn.qkv_proj.weight"])
        q, k, v = qkv.split([Hq * D, Hkv * D, Hkv * D], dim=-1)
        q, k = qk_norm_rotary(positions, q, k, w[p + "self_attn.q_norm.weight"], w[p + "self_attn.k_norm.weight"],
                              shape.rms_eps, D, cache)
        ops.kv_store(kv.k[i], kv.v[i], out_cache_loc, k.reshape(-1, Hkv, D), v.reshape(-1, Hkv, D))
        q3 = q.reshape(-1, Hq, D)
        if mode == "decode":
            a = ops.decode_attention(q3, kv.k[i], kv.v[i], kv.req_to_token, req_pool_indices, seq_lens, scale)
        else:
            a = ops.extend_attention(q3, kv.k[i], kv.v[i], kv.req_to_token, req_pool_indices, seq_lens,
                                     extend_seq_lens, extend_start_loc, scale)
        h = torch.nn.functional.linear(a.reshape(-1, Hq * D), w[p + "self_attn.o_proj.weight"])
        h, residual = ops.rmsnorm(h, w[p + "post_attention_layernorm.weight"], shape.rms_eps, residual)
        gu = torch.nn.functional.linear(h, w[p + "mlp.gate_up_proj.weight"])
        h = torch.nn.functional.linear(ops.silu_and_mul(gu), w[p + "mlp.down_proj.weight"])
    h, _ = ops.rmsnorm(h, w["model.norm.weight"], shape.rms_eps, residual)
    if mode == "extend":
        h = h[torch.cumsum(extend_seq_lens.long(), 0) - 1]
    head = w["model.embed_tokens.weight"] if shape.tie else w["lm_head.weight"]
    return torch.matmul(h.to(head.dtype), head.T)[:, : shape.vocab].float()


# --------------------------------------------------------------------------- the fixture
_FIXTURE = None


def load_case(name):
    global _FIXTURE
    if _FIXTURE is None:
        _FIXTURE = golden.load("tiny_qwen3")
    g, pfx = _FIXTURE, name + "_"
    hidden, inter, nl, Hq, Hkv, vocab, tie, D = (int(x) for x in g[pfx + "cfg"])
    shape = Qwen3Shape(hidden, inter, nl, Hq, Hkv, vocab, D, bool(tie), float(g[pfx + "rope_theta"]),
                       int(g[pfx + "max_pos"]), float(g[pfx + "rms_eps"]))
    w = {k[len(pfx) + 3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith(pfx + "w::")}
    return g, pfx, shape, w


def oracle_run(name, dtype=torch.float32, w=None):
    """(prefill logits, decode logits, kv) of the oracle evaluated in `dtype` over the fixture's two steps"""
    g, pfx, shape, w0 = load_case(name)
    w = {k: v.to(dtype) for k, v in (w or w0).items()}
    kv = OracleKV(shape, 96, 4, 64, dtype)
    ext = torch.from_numpy(g[pfx + "extend_lens"])
    req = torch.from_numpy(g[pfx + "req_pool_indices"])
    loc = torch.from_numpy(g[pfx + "out_cache_loc"])
    pre = torch.zeros_like(ext)
    ops.write_req_to_token(kv.req_to_token, req, pre, ext, ext, loc)
    positions, start = ops.compute_position(pre, ext)
    l1 = forward(shape, w, kv, mode="extend", input_ids=torch.from_numpy(g[pfx + "input_ids"]), positions=positions,
                 req_pool_indices=req, seq_lens=ext.long(), out_cache_loc=loc, extend_seq_lens=ext,
                 extend_start_loc=start)
    seq2 = ext.long() + 1
    dloc = torch.from_numpy(g[pfx + "decode_out_cache_loc"])
    ops.write_req_to_token(kv.req_to_token, req, ext.long(), seq2, torch.ones_like(seq2), dloc)
    l2 = forward(shape, w, kv, mode="decode", input_ids=torch.from_numpy(g[pfx + "next_ids"]),
                 positions=ops.clamp_position(seq2), req_pool_indices=req, seq_lens=seq2, out_cache_loc=dloc)
    return l1, l2, kv


def model_config(shape: Qwen3Shape):
    from scratchpad_amd.model_runner import ModelConfig
    return ModelConfig(shape.hidden, shape.inter, shape.layers, shape.Hq, shape.Hkv, shape.vocab, context_len=60,
                       head_dim=shape.D, rms_norm_eps=shape.rms_eps, rope_theta=shape.rope_theta,
                       max_position_embeddings=shape.max_pos, tie_word_embeddings=shape.tie, architecture="qwen3")


def run_case(name, dtype, graph_bs=None, fused=True, w=None):
    """The fixture's prefill and decode step through ModelRunner -> HipAttnBackend, as the scheduler hands them over.
    Returns (prefill logits, decode logits, next ids, model runner), logits as fp32 CPU tensors.  ``fused`` sets the
    backend's fused_rope_kv_store; ``w`` replaces the fixture's weights."""
    from scratchpad_amd import _native
    from scratchpad_amd.forward_info import ForwardMode, ModelWorkerBatch
    from scratchpad_amd.model_runner import ModelRunner, ServerArgs, TpModelWorker
    g, pfx, shape, w0 = load_case(name)
    args = ServerArgs(max_total_tokens=96, max_running_requests=3, disable_cuda_graph=graph_bs is None,
                      cuda_graph_bs=graph_bs)
    mr = ModelRunner(model_config(shape), args, dtype=dtype, init_weights=False)
    mr.model.load_full_state_dict({k: v.to(mr.device) for k, v in (w or w0).items()})
    mr.attn_backend.fused_rope_kv_store = fused
    if graph_bs is not None:
        mr.init_cuda_graphs()
    worker = TpModelWorker(mr)
    dev = mr.device
    ext = torch.from_numpy(g[pfx + "extend_lens"])
    req = torch.from_numpy(g[pfx + "req_pool_indices"]).to(dev)
    loc = torch.from_numpy(g[pfx + "out_cache_loc"]).to(dev)
    ids = torch.from_numpy(g[pfx + "input_ids"]).to(dev)
    seq = ext.long().to(dev)
    _native.write_req_to_token(mr.req_to_token_pool.req_to_token, req, torch.zeros_like(seq), seq, seq, loc)
    batch = ModelWorkerBatch(bid=1, forward_mode=ForwardMode.EXTEND, input_ids=ids, req_pool_indices=req,
                             seq_lens=seq, out_cache_loc=loc, seq_lens_sum=int(ext.sum()),
                             extend_num_tokens=int(ext.sum()), extend_seq_lens=ext.tolist(),
                             extend_prefix_lens=[0] * len(ext))
    out, nxt = worker.forward_batch_generation(batch)
    prefill = out.next_token_logits.float().cpu()
    dloc = torch.from_numpy(g[pfx + "decode_out_cache_loc"]).to(dev)
    seq2 = seq + 1
    mr.req_to_token_pool.write((req, seq), dloc.to(torch.int32))
    nxt_in = torch.from_numpy(g[pfx + "next_ids"]).to(dev)       # the reference's sampled ids
    batch2 = ModelWorkerBatch(bid=2, forward_mode=ForwardMode.DECODE, input_ids=nxt_in, req_pool_indices=req,
                              seq_lens=seq2, out_cache_loc=dloc, seq_lens_sum=int(seq2.sum()))
    out2, _ = worker.forward_batch_generation(batch2)
    return prefill, out2.next_token_logits.float().cpu(), nxt.cpu(), mr
