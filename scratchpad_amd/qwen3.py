"""Qwen3 decoder hosted on the HIP hot path.

Re-hosts nn/models/qwen/qwen3.py (Qwen3Attention 38-137, Qwen3DecoderLayer 140-202, Qwen3Model 205-217,
Qwen3ForCausalLM 220-283): the reference's module tree and parameter names, ``self_attn.q_norm.weight`` and
``self_attn.k_norm.weight`` included, so its checkpoints and state_dicts map 1:1.

What Qwen3 adds to llama.py's skeleton is its attention block: an explicit ``head_dim`` and a per-head RMSNorm of q
and k between qkv_proj and the rotary embedding (``_apply_qk_norm``, 114-123), both switched on in LlamaAttention by
this file's constructor, which also holds the ``attention_bias`` refusal.  The layer protocol with its deferred
all-reduce under tensor parallelism, the decoder loop, the causal-LM shell, ``forward(get_embedding=True)`` (the
reference's pooler branch, qwen3.py:247-250) and the loaders are inherited from LlamaDecoderLayer, LlamaModel and
LlamaForCausalLM; the MLP is LlamaMLP.

On the fused path (``HipAttnBackend.fused_rope_kv_store``) the two norms, the rotation and the KV store are ONE launch
(sp_qk_norm_rotary), bit-identical to the reference's order norm, norm, rotary, store, which the non-fused branch runs.
The q_norm / k_norm weights are [head_dim] and replicated on every tensor-parallel rank."""
from typing import Any, Dict, Optional

from torch import nn

from .layers import RMSNorm
from .llama import LlamaAttention, LlamaDecoderLayer, LlamaForCausalLM, LlamaMLP, LlamaModel


class Qwen3Attention(LlamaAttention):
    def __init__(self, hidden_size: int, num_heads: int, num_kv_heads: int, layer_id: int = 0,
                 rope_theta: float = 1000000, rope_scaling: Optional[Dict[str, Any]] = None,
                 head_dim: Optional[int] = None, max_position_embeddings: int = 32768,
                 rms_norm_eps: float = 1e-6, attention_bias: bool = False, dtype=None):
        if attention_bias:
            raise NotImplementedError("attention_bias=True (a bias on qkv_proj / o_proj) is not built: no released "
                                      "dense Qwen3 checkpoint sets it")
        super().__init__(None, hidden_size, num_heads, num_kv_heads, layer_id=layer_id, rope_theta=rope_theta,
                         rope_scaling=rope_scaling, max_position_embeddings=max_position_embeddings, dtype=dtype,
                         head_dim=head_dim, qk_norm_eps=rms_norm_eps)


class Qwen3DecoderLayer(LlamaDecoderLayer):
    """qwen3.py:140-202; ``forward`` is LlamaDecoderLayer's"""

    def __init__(self, config, layer_id: int = 0, dtype=None):
        nn.Module.__init__(self)
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


class Qwen3Model(LlamaModel):
    """Qwen2Model with Qwen3DecoderLayer (qwen3.py:205-217)."""
    layer_class = Qwen3DecoderLayer


class Qwen3ForCausalLM(LlamaForCausalLM):
    """qwen3.py:220-325: the q_norm / k_norm weights, like every norm weight, load whole"""
    model_class = Qwen3Model
