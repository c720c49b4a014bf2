"""Apertus (SwissAI) decoder hosted on the HIP hot path.

Re-hosts nn/models/swissai/apertus.py (SwissAIMLP 31-68, SwissAIAttention 71-176, SwissAIDecoderLayer 179-257,
SwissAIModel 260-308, SwissAIForCausalLM 311-450): the reference's module tree and parameter names -
``attention_layernorm`` / ``feedforward_layernorm`` for the two layer norms, ``self_attn.q_norm`` / ``k_norm``,
``mlp.up_proj`` / ``mlp.down_proj`` and the two raw activation scalars ``mlp.act_fn.alpha_p`` / ``alpha_n`` - so its
checkpoints and state_dicts map 1:1.

The attention block is Qwen3's: per-head RMSNorm of q and k, rotary embedding, KV store - one sp_qk_norm_rotary launch
on the fused path, the reference's order of separate steps on the other.  SwissAIAttention is qwen3.py's class under
the reference's constructor; nothing of it is restated here.  To llama.py's skeleton this file states only what
differs: the names of the two layer norms (LlamaDecoderLayer.forward runs the layer protocol, deferred all-reduce
under tensor parallelism included, over them), the layer class (LlamaModel), and for LlamaForCausalLM no pooler, the
``get_embedding`` refusal and a stacking table of q_proj / k_proj / v_proj alone - up_proj stands alone.

What is new is the MLP: ``up_proj -> xIELU -> down_proj`` with no gate projection (apertus.py:63-68).  up_proj is
column-parallel with a single shard, down_proj row-parallel, and the two activation scalars are replicated on every
tensor-parallel rank.  A step of at most 16 rows runs up_proj and the activation as ONE weight-streaming launch
(sp_gemm_skinny_xielu), bit for bit the skinny projection followed by sp_xielu; above that the projection is the
library GEMM and sp_xielu runs in place on its result (_native.XIELU_CALLS says which ran).

Refused with NotImplementedError: ``attention_bias`` / ``bias`` / ``qkv_bias`` / ``mlp_bias``, a
``partial_rotary_factor`` other than 1, a ``hidden_act`` other than "xielu".  The reference's ``get_embedding`` /
pooler branch (apertus.py:336, 353-354) is not built: ``forward(get_embedding=True)`` raises."""
from typing import Any, Dict, Optional

import torch
from torch import nn

from . import _native
from .forward_info import ForwardBatch
from .layers import RMSNorm, XIELU
from .llama import (LlamaDecoderLayer, LlamaForCausalLM, LlamaModel, LogitsProcessorOutput,
                    MergedColumnParallelLinear, RowParallelLinear)
from .qwen3 import Qwen3Attention


class SwissAIMLP(nn.Module):
    def __init__(self, hidden_size: int, intermediate_size: int, hidden_act: str, bias: bool = False, dtype=None):
        super().__init__()
        if bias:
            raise NotImplementedError("mlp_bias=True (a bias on up_proj / down_proj) is not built")
        if hidden_act != "xielu":
            raise NotImplementedError(f"hidden_act={hidden_act!r} is not built for this architecture: only xielu")
        self.up_proj = MergedColumnParallelLinear(hidden_size, [intermediate_size], dtype)
        self.down_proj = RowParallelLinear(intermediate_size, hidden_size, dtype)
        self.act_fn = XIELU()

    def forward(self, x, reduce_output: bool = True):
        # note: with xielu, there's no gate_proj.  <= 16 rows: projection and activation in one launch
        act = self.act_fn
        x = _native.linear_xielu(x, self.up_proj.weight, act.alpha_p.data, act.alpha_n.data, act.beta, act.eps)
        x, _ = self.down_proj(x, reduce_output)
        return x


class SwissAIAttention(Qwen3Attention):
    """apertus.py:71-176 is Qwen3Attention with the head size and the norm epsilon read from the config"""

    def __init__(self, hidden_size: int, config, num_heads: int, num_kv_heads: int, layer_id: int = 0,
                 rope_theta: float = 10000, rope_scaling: Optional[Dict[str, Any]] = None,
                 max_position_embeddings: int = 8192, bias: bool = False, bias_o_proj: bool = False, dtype=None):
        if getattr(config, "partial_rotary_factor", 1) != 1:
            raise NotImplementedError("partial_rotary_factor != 1 is not built: q_norm / k_norm and the rotation "
                                      "share one fused launch over the whole head")
        super().__init__(hidden_size, num_heads, num_kv_heads, layer_id=layer_id, rope_theta=rope_theta,
                         rope_scaling=rope_scaling, head_dim=getattr(config, "head_dim", None),
                         max_position_embeddings=max_position_embeddings, rms_norm_eps=config.rms_norm_eps,
                         attention_bias=bool(bias or bias_o_proj), dtype=dtype)
        self.layer_id = layer_id


class SwissAIDecoderLayer(LlamaDecoderLayer):
    """apertus.py:179-257; ``forward`` is LlamaDecoderLayer's over this layer's norm names"""
    norm_names = ("attention_layernorm", "feedforward_layernorm")

    def __init__(self, config, layer_id: int = 0, dtype=None):
        nn.Module.__init__(self)
        self.hidden_size = config.hidden_size
        rope_scaling = getattr(config, "rope_scaling", None)
        if rope_scaling is not None and getattr(config, "original_max_position_embeddings", None):
            rope_scaling = dict(rope_scaling,
                                original_max_position_embeddings=config.original_max_position_embeddings)
        attention_bias = getattr(config, "attention_bias", False) or getattr(config, "bias", False)
        bias_o_proj = attention_bias
        if hasattr(config, "qkv_bias"):
            attention_bias = config.qkv_bias
        self.self_attn = SwissAIAttention(
            config=config, hidden_size=self.hidden_size, num_heads=config.num_attention_heads,
            num_kv_heads=config.num_key_value_heads, layer_id=layer_id,
            rope_theta=getattr(config, "rope_theta", 10000), rope_scaling=rope_scaling,
            max_position_embeddings=getattr(config, "max_position_embeddings", 8192), bias=attention_bias,
            bias_o_proj=bias_o_proj, dtype=dtype)
        self.mlp = SwissAIMLP(self.hidden_size, config.intermediate_size, config.hidden_act,
                              bias=getattr(config, "mlp_bias", False), dtype=dtype)
        self.attention_layernorm = RMSNorm(config.hidden_size, eps=config.rms_norm_eps)
        self.feedforward_layernorm = RMSNorm(config.hidden_size, eps=config.rms_norm_eps)


class SwissAIModel(LlamaModel):
    layer_class = SwissAIDecoderLayer


class SwissAIForCausalLM(LlamaForCausalLM):
    model_class = SwissAIModel
    has_pooler = False
    # apertus.py:406-439: the norm weights and the two activation scalars of every layer load whole
    stacked_params = {"qkv_proj": ("q_proj", "k_proj", "v_proj")}

    @torch.no_grad()
    def forward(self, input_ids, positions, forward_batch: ForwardBatch, input_embeds: torch.Tensor = None,
                get_embedding: bool = False) -> LogitsProcessorOutput:
        if get_embedding:
            raise NotImplementedError("get_embedding=True (the reference's Pooler branch) is not built")
        return super().forward(input_ids, positions, forward_batch, input_embeds)
