"""Qwen3 decoder hosted on the HIP hot path.

Re-hosts nn/models/qwen/qwen3.py (Qwen3Attention 38-137, Qwen3DecoderLayer 140-202, Qwen3Model 205-217,
Qwen3ForCausalLM 220-283): the reference's module tree and parameter names, ``self_attn.q_norm.weight`` and
``self_attn.k_norm.weight`` included, so its checkpoints and state_dicts map 1:1.  A Qwen3 layer is the Llama layer
with an explicit ``head_dim`` and a per-head RMSNorm of q and k between qkv_proj and the rotary embedding
(``_apply_qk_norm``, 114-123); everything else - the MLP, the sharded linears, the logits processor, the deferred
all-reduce protocol under tensor parallelism, weight loading - is llama.py's and is reused from there.

On the fused path (``HipAttnBackend.fused_rope_kv_store``) the two norms, the rotation and the KV store are ONE launch
(sp_qk_norm_rotary), bit-identical to the reference's order norm, norm, rotary, store, which the non-fused branch runs.
The q_norm / k_norm weights are [head_dim] and replicated on every tensor-parallel rank.  ``forward(get_embedding=True)``
is the reference's pooler branch (qwen3.py:247-250): llama.pooled_embedding."""
from typing import Any, Dict, Optional, Tuple

import torch
from torch import nn

from .attention import RadixAttention
from .distributed import get_tensor_model_parallel_world_size
from .forward_info import ForwardBatch
from .layers import Pooler, PoolingType, RMSNorm, get_rope
from .llama import (LlamaForCausalLM, LlamaMLP, LogitsProcessor, LogitsProcessorOutput, ParallelLMHead,
                    QKVParallelLinear, RowParallelLinear, VocabParallelEmbedding, norm_after_row_parallel,
                    pooled_embedding)


class Qwen3Attention(nn.Module):
    def __init__(self, hidden_size: int, num_heads: int, num_kv_heads: int, layer_id: int = 0,
                 rope_theta: float = 1000000, rope_scaling: Optional[Dict[str, Any]] = None,
                 head_dim: Optional[int] = None, max_position_embeddings: int = 32768,
                 rms_norm_eps: float = 1e-6, attention_bias: bool = False, dtype=None):
        super().__init__()
        if attention_bias:
            raise NotImplementedError("attention_bias=True (a bias on qkv_proj / o_proj) is not built: no released "
                                      "dense Qwen3 checkpoint sets it")
        self.hidden_size = hidden_size
        tp_size = get_tensor_model_parallel_world_size()
        self.total_num_heads = num_heads
        assert self.total_num_heads % tp_size == 0
        self.num_heads = self.total_num_heads // tp_size
        self.total_num_kv_heads = num_kv_heads
        if self.total_num_kv_heads >= tp_size:
            assert self.total_num_kv_heads % tp_size == 0
        else:
            assert tp_size % self.total_num_kv_heads == 0
        self.num_kv_heads = max(1, self.total_num_kv_heads // tp_size)
        self.head_dim = head_dim or hidden_size // self.total_num_heads
        self.q_size = self.num_heads * self.head_dim
        self.kv_size = self.num_kv_heads * self.head_dim
        self.scaling = self.head_dim ** -0.5
        self.rope_theta = rope_theta
        self.max_position_embeddings = max_position_embeddings
        self.q_norm = RMSNorm(self.head_dim, eps=rms_norm_eps)
        self.k_norm = RMSNorm(self.head_dim, eps=rms_norm_eps)
        self.qkv_proj = QKVParallelLinear(hidden_size, self.head_dim, self.total_num_heads,
                                          self.total_num_kv_heads, dtype)
        self.o_proj = RowParallelLinear(self.total_num_heads * self.head_dim, hidden_size, dtype)
        self.rotary_emb = get_rope(self.head_dim, rotary_dim=self.head_dim, max_position=max_position_embeddings,
                                   base=rope_theta, rope_scaling=rope_scaling, dtype=dtype)
        self.attn = RadixAttention(self.num_heads, self.head_dim, self.scaling, num_kv_heads=self.num_kv_heads,
                                   layer_id=layer_id)

    def _apply_qk_norm(self, q: torch.Tensor, k: torch.Tensor) -> None:
        """qwen3.py:114-123, written back into the qkv views the rotary embedding then rotates in place"""
        q.copy_(self.q_norm(q.reshape(-1, self.head_dim)).view(q.shape))
        k.copy_(self.k_norm(k.reshape(-1, self.head_dim)).view(k.shape))

    def forward(self, positions: torch.Tensor, hidden_states: torch.Tensor, forward_batch: ForwardBatch,
                reduce_output: bool = True) -> torch.Tensor:
        qkv, _ = self.qkv_proj(hidden_states)
        q, k, v = qkv.split([self.q_size, self.kv_size, self.kv_size], dim=-1)
        backend = forward_batch.attn_backend
        if getattr(backend, "fused_rope_kv_store", False):
            # one launch: normalise every head of q and k, rotate them in place AND scatter k + v into the KV pool
            backend.rotary_and_store(self.rotary_emb, positions, q, k, v, self.attn, forward_batch,
                                     q_norm=self.q_norm, k_norm=self.k_norm)
            attn_output = self.attn(q, k, v, forward_batch, save_kv_cache=False)
        else:
            self._apply_qk_norm(q, k)
            q, k = self.rotary_emb(positions, q, k)       # in place on the qkv views
            attn_output = self.attn(q, k, v, forward_batch)
        output, _ = self.o_proj(attn_output, reduce_output)
        return output


class Qwen3DecoderLayer(nn.Module):
    def __init__(self, config, layer_id: int = 0, dtype=None):
        super().__init__()
        self.hidden_size = config.hidden_size
        self.self_attn = Qwen3Attention(
            hidden_size=self.hidden_size, num_heads=config.num_attention_heads,
            num_kv_heads=config.num_key_value_heads, layer_id=layer_id,
            rope_theta=getattr(config, "rope_theta", 1000000), rope_scaling=getattr(config, "rope_scaling", None),
            head_dim=getattr(config, "head_dim", None),
            max_position_embeddings=getattr(config, "max_position_embeddings", 32768),
            rms_norm_eps=config.rms_norm_eps, attention_bias=getattr(config, "attention_bias", False), dtype=dtype)
        self.mlp = LlamaMLP(self.hidden_size, config.intermediate_size, config.hidden_act, dtype)
        self.input_layernorm = RMSNorm(config.hidden_size, eps=config.rms_norm_eps)
        self.post_attention_layernorm = RMSNorm(config.hidden_size, eps=config.rms_norm_eps)

    def forward(self, positions, hidden_states, forward_batch: ForwardBatch, residual: Optional[torch.Tensor],
                defer_reduce: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """qwen3.py:180-202 with llama.py's deferred all-reduce protocol (LlamaDecoderLayer.forward)."""
        if residual is None:
            residual = hidden_states
            hidden_states = self.input_layernorm(hidden_states)
        elif defer_reduce:
            hidden_states, residual = norm_after_row_parallel(self.input_layernorm, hidden_states, residual)
        else:
            hidden_states, residual = self.input_layernorm(hidden_states, residual)
        hidden_states = self.self_attn(positions=positions, hidden_states=hidden_states,
                                       forward_batch=forward_batch, reduce_output=not defer_reduce)
        if defer_reduce:
            hidden_states, residual = norm_after_row_parallel(self.post_attention_layernorm, hidden_states,
                                                              residual)
        else:
            hidden_states, residual = self.post_attention_layernorm(hidden_states, residual)
        hidden_states = self.mlp(hidden_states, reduce_output=not defer_reduce)
        return hidden_states, residual


class Qwen3Model(nn.Module):
    """Qwen2Model with Qwen3DecoderLayer (qwen3.py:205-217)."""

    def __init__(self, config, dtype=None):
        super().__init__()
        self.config = config
        self.vocab_size = config.vocab_size
        self.embed_tokens = VocabParallelEmbedding(config.vocab_size, config.hidden_size, dtype)
        self.layers = nn.ModuleList(
            [Qwen3DecoderLayer(config, i, dtype) for i in range(config.num_hidden_layers)])
        self.norm = RMSNorm(config.hidden_size, eps=config.rms_norm_eps)

    def forward(self, input_ids, positions, forward_batch: ForwardBatch,
                input_embeds: torch.Tensor = None, before_final_norm: bool = False) -> torch.Tensor:
        """before_final_norm: as LlamaModel.forward"""
        hidden_states = self.embed_tokens(input_ids) if input_embeds is None else input_embeds
        residual = None
        defer = get_tensor_model_parallel_world_size() > 1
        for layer in self.layers:
            hidden_states, residual = layer(positions, hidden_states, forward_batch, residual, defer)
        if before_final_norm:
            if defer:
                raise ValueError("before_final_norm under tensor parallelism: the hidden states are partial sums")
            return hidden_states, residual
        if defer:
            hidden_states, _ = norm_after_row_parallel(self.norm, hidden_states, residual)
        else:
            hidden_states, _ = self.norm(hidden_states, residual)
        return hidden_states


class Qwen3ForCausalLM(nn.Module):
    def __init__(self, config, dtype=None):
        super().__init__()
        self.config = config
        self.model = Qwen3Model(config, dtype)
        if getattr(config, "tie_word_embeddings", False):
            self.lm_head = self.model.embed_tokens
        else:
            self.lm_head = ParallelLMHead(config.vocab_size, config.hidden_size, dtype)
        self.logits_processor = LogitsProcessor(config)
        self.pooler = Pooler(pooling_type=PoolingType.LAST, normalize=True)

    @torch.no_grad()
    def forward(self, input_ids, positions, forward_batch: ForwardBatch,
                input_embeds: torch.Tensor = None, get_embedding: bool = False) -> LogitsProcessorOutput:
        if get_embedding:
            return pooled_embedding(self.model, self.pooler, input_ids, positions, forward_batch, input_embeds)
        hidden_states = self.model(input_ids, positions, forward_batch, input_embeds)
        return self.logits_processor(input_ids, hidden_states, self.lm_head, forward_batch)

    # the merged-parameter loaders are llama.py's: they go by parameter names and ``shard_from_full`` alone, and the
    # q_norm / k_norm weights, like every norm weight, are replicated
    load_full_state_dict = LlamaForCausalLM.load_full_state_dict

    def load_weights(self, weights) -> None:
        """HF checkpoint names -> merged parameters (qwen3.py:285-325).  A tied checkpoint's lm_head is skipped."""
        tied = getattr(self.config, "tie_word_embeddings", False)
        LlamaForCausalLM.load_weights(self, ((n, w) for n, w in weights if not (tied and "lm_head.weight" in n)))
