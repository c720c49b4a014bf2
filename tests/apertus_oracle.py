"""CPU oracle of the Apertus decoder and the fixture flow of tests/golden/tiny_apertus.npz (TEST INFRASTRUCTURE ONLY).

A plain-torch restatement of nn/models/swissai/apertus.py as the reference hosts it: Qwen3's attention block
(tests/qwen3_oracle.py: per-head RMSNorm of q and k, rotary embedding, KV store) between ``attention_layernorm`` and
``feedforward_layernorm``, and the ungated MLP ``down_proj(xIELU(up_proj(h)))`` with two raw scalars per layer.
Pinned by tiny_apertus.npz, the logits of the reference's own ``SwissAIForCausalLM`` (tests/test_apertus_host.py).

``xielu`` is the KERNEL's contract (sp_xielu): fp32 arithmetic from the stored inputs and ONE rounding to the
activation dtype.  The reference's ``XIELU.forward`` in fp32 is exactly that.  A reference run in bf16 or fp16 is not:
there torch rounds after every tensor operation (softplus, each product, expm1, each sum).  The model-level bars
absorb the difference (16-bit runs are held to this oracle in the same dtype, and fp16 to the fp32 reference at 5e-3).

``run_case`` drives the same fixture through ModelRunner -> HipAttnBackend (GPU tests only)."""
from typing import Dict, Optional

import torch

from oracle import ops
from oracle.llama import OracleKV
from tests import golden
from tests.qwen3_oracle import Qwen3Shape, qk_norm_rotary

XIELU_BETA = 0.5
XIELU_EPS = float(torch.tensor(-1e-6, dtype=torch.bfloat16))      # the reference's stored constant, in every dtype


class ApertusShape(Qwen3Shape):
    """the fields of Qwen3Shape; D = hidden / Hq (SwissAIConfig carries no head_dim)"""


def xielu(x: torch.Tensor, alpha_p_raw: torch.Tensor, alpha_n_raw: torch.Tensor, beta: float = XIELU_BETA,
          eps: float = XIELU_EPS, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """XIELU.forward (nn/layers/activation.py:53-60) in fp32 from the stored x and raw scalars, rounded once"""
    xf = x.float()
    ap = torch.nn.functional.softplus(alpha_p_raw.float())
    an = beta + torch.nn.functional.softplus(alpha_n_raw.float())
    y = torch.where(xf > 0, ap * xf * xf + beta * xf,
                    an * torch.expm1(torch.min(xf, torch.tensor(eps))) - an * xf + beta * xf)
    return y.to(dtype or x.dtype)


def forward(shape: ApertusShape, w: Dict[str, torch.Tensor], kv: OracleKV, *, mode: str, input_ids, positions,
            req_pool_indices, seq_lens, out_cache_loc, extend_seq_lens: Optional[torch.Tensor] = None,
            extend_start_loc: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One forward pass (apertus.py:163-176, 235-257, 287-308, 339-352); next-token logits [bs, vocab] fp32.
    Arguments as oracle.llama.forward."""
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
            h = ops.rmsnorm(h, w[p + "attention_layernorm.weight"], shape.rms_eps)
        else:
            h, residual = ops.rmsnorm(h, w[p + "attention_layernorm.weight"], shape.rms_eps, residual)
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
        h, residual = ops.rmsnorm(h, w[p + "feedforward_layernorm.weight"], shape.rms_eps, residual)
        up = torch.nn.functional.linear(h, w[p + "mlp.up_proj.weight"])
        act = xielu(up, w[p + "mlp.act_fn.alpha_p"], w[p + "mlp.act_fn.alpha_n"])
        h = torch.nn.functional.linear(act, w[p + "mlp.down_proj.weight"])
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
        _FIXTURE = golden.load("tiny_apertus")
    g, pfx = _FIXTURE, name + "_"
    hidden, inter, nl, Hq, Hkv, vocab, tie, D = (int(x) for x in g[pfx + "cfg"])
    shape = ApertusShape(hidden, inter, nl, Hq, Hkv, vocab, D, bool(tie), float(g[pfx + "rope_theta"]),
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


def model_config(shape: ApertusShape):
    from scratchpad_amd.model_runner import ModelConfig
    return ModelConfig(shape.hidden, shape.inter, shape.layers, shape.Hq, shape.Hkv, shape.vocab, context_len=60,
                       head_dim=shape.D, rms_norm_eps=shape.rms_eps, rope_theta=shape.rope_theta,
                       max_position_embeddings=shape.max_pos, tie_word_embeddings=shape.tie, hidden_act="xielu",
                       architecture="apertus")


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
