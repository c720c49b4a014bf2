"""Llama with a mixture-of-experts MLP, hosted on the HIP hot path.

Re-hosts nn/models/llama/llama_moe.py (LlamaMLP 32-67, LlamaMoE 70-120, LlamaDecoderLayer 123-192, LlamaModel 195-240,
LlamaMoEForCausalLM 243-368): the reference's module tree and parameter names - ``moe.gate`` ([E, H], an
``nn.Linear``-shaped weight), ``moe.mlp.{i}.gate_up_proj`` / ``moe.mlp.{i}.down_proj`` - so its checkpoints and
state_dicts map 1:1.  What it adds to llama.py's skeleton is the feed-forward block ``moe`` and the refusals of its
constructors: the layer protocol (LlamaDecoderLayer.forward), the decoder loop (LlamaModel), the causal-LM shell and
the loaders (LlamaForCausalLM) are inherited, and attention, norms, embedding and LM head are llama.py's.

The reference's ``LlamaMoE.forward`` loops over the experts with ``torch.where`` and boolean indexing: a host
synchronisation and a data-dependent shape in every layer, which a HIP-graph replay cannot contain.  Here a 16-bit layer
is the router projection (``F.linear`` through the usual linear path) followed by five launches whose grids depend on
the batch shape alone (csrc/moe.hip: route, grouped gate_up + SiLU-mul, grouped down, combine); the grouping lives in
device memory, so a captured step follows the routing of every replay.  The experts' weights are ONE stacked tensor
per projection (``w13`` [E, 2 I, H], ``w2`` [E, H, I]); the per-expert parameters are views of them, so a checkpoint
loads straight into the stacked storage and nothing is packed per step.

fp32 models route on the device too (sp_moe_route accepts fp32 logits) and then take the reference's formulation - one
library product per expert over its gathered rows, added in ascending expert index: eager only, it raises under graph
capture (``_native.MOE_CALLS`` says which path a step took).

Refused with NotImplementedError at construction: tensor parallelism (TP > 1), ``grouped_topk``, more than 64 experts
or more than 8 experts per token.  LoRA toppings on this model are refused by ModelRunner.  The quantised MoE
variants are llama_quant_moe.py's."""
import torch
from torch import nn

from . import _native, llama
from .distributed import get_tensor_model_parallel_world_size
from .forward_info import ForwardBatch
from .layers import RMSNorm
from .llama import LlamaAttention, LogitsProcessorOutput


class _ExpertLinear(nn.Module):
    """one expert's projection: ``weight`` is a view of its slot of the layer's stacked tensor"""

    def __init__(self, slot: torch.Tensor):
        super().__init__()
        self.weight = nn.Parameter(slot, requires_grad=False)


class LlamaMLP(nn.Module):
    """llama_moe.py:32-67 as the experts hold it: names and shapes only - the arithmetic is the layer's"""

    def __init__(self, w13_slot: torch.Tensor, w2_slot: torch.Tensor, hidden_act: str):
        super().__init__()
        if hidden_act != "silu":
            raise ValueError(f"Unsupported activation: {hidden_act}. Only silu is supported for now.")
        self.gate_up_proj = _ExpertLinear(w13_slot)
        self.down_proj = _ExpertLinear(w2_slot)


class LlamaMoE(nn.Module):
    def __init__(self, hidden_size: int, intermediate_size: int, hidden_act: str, num_experts: int,
                 experts_per_token: int, dtype=None):
        super().__init__()
        if get_tensor_model_parallel_world_size() > 1:
            raise NotImplementedError("Llama-MoE under tensor parallelism (TP > 1) is out of scope")
        if not 0 < num_experts <= _native.MOE_MAX_EXPERTS:
            raise NotImplementedError(f"num_experts={num_experts}: 1 .. {_native.MOE_MAX_EXPERTS} are built")
        if not 0 < experts_per_token <= min(num_experts, _native.MOE_MAX_TOP_K):
            raise NotImplementedError(f"experts_per_token={experts_per_token}: 1 .. min(num_experts, "
                                      f"{_native.MOE_MAX_TOP_K}) are built")
        self.experts_per_token = experts_per_token
        self.num_experts = num_experts
        # the two stacked tensors the kernels read; plain attributes, so state_dict keeps the reference's names
        self.w13 = torch.empty(num_experts, 2 * intermediate_size, hidden_size, dtype=dtype)
        self.w2 = torch.empty(num_experts, hidden_size, intermediate_size, dtype=dtype)
        self.mlp = nn.ModuleList([LlamaMLP(self.w13[i], self.w2[i], hidden_act) for i in range(num_experts)])
        self.gate = nn.Linear(hidden_size, num_experts, bias=False, dtype=dtype)
        self.gate.weight.requires_grad_(False)

    def pack_experts(self) -> None:
        """(Re)build the stacked tensors from the per-expert parameters and make those views of them again: needed
        once after anything that moved or replaced the parameters (``.to(device)``, a dtype cast)."""
        ref = self.mlp[0].gate_up_proj.weight
        w13 = torch.stack([m.gate_up_proj.weight.data for m in self.mlp]).to(ref.device)
        w2 = torch.stack([m.down_proj.weight.data for m in self.mlp]).to(ref.device)
        for i, m in enumerate(self.mlp):
            m.gate_up_proj.weight.data = w13[i]
            m.down_proj.weight.data = w2[i]
        self.w13, self.w2 = w13, w2

    def _packed(self) -> bool:
        a, b = self.mlp[0], self.mlp[-1]
        return (a.gate_up_proj.weight.data_ptr() == self.w13[0].data_ptr()
                and b.down_proj.weight.data_ptr() == self.w2[-1].data_ptr() and self.w13.dtype == a.gate_up_proj.weight.dtype)

    def forward(self, x: torch.Tensor, reduce_output: bool = True) -> torch.Tensor:
        """reduce_output: the layer protocol's keyword; there are no partial sums to leave (TP > 1 is refused)"""
        shape = x.shape
        x = x.reshape(-1, shape[-1])
        if not self._packed():
            self.pack_experts()
        router_logits = _native.linear(x, self.gate.weight)
        if x.dtype == torch.float32:
            out = _native.moe_experts_eager(x, router_logits, self.w13, self.w2, self.experts_per_token)
        else:
            out = _native.moe_experts(x, router_logits, self.w13, self.w2, self.experts_per_token)
        return out.view(shape)


class LlamaDecoderLayer(llama.LlamaDecoderLayer):
    """llama_moe.py:123-192; ``forward`` is llama.py's LlamaDecoderLayer's over ``moe``"""
    feed_forward_name = "moe"

    def __init__(self, config, layer_id: int = 0, dtype=None):
        nn.Module.__init__(self)
        self.hidden_size = config.hidden_size
        if getattr(config, "grouped_topk", False):
            raise NotImplementedError("grouped_topk (fused_moe/patch.py) is not built: plain top-k routing only")
        self.self_attn = LlamaAttention(
            config=config, hidden_size=self.hidden_size, num_heads=config.num_attention_heads,
            num_kv_heads=config.num_key_value_heads, layer_id=layer_id,
            rope_theta=getattr(config, "rope_theta", 10000), rope_scaling=getattr(config, "rope_scaling", None),
            rope_is_neox_style=getattr(config, "rope_is_neox_style", True),
            max_position_embeddings=getattr(config, "max_position_embeddings", 8192), dtype=dtype)
        self.moe = LlamaMoE(self.hidden_size, config.intermediate_size, config.hidden_act, config.num_experts,
                            config.experts_per_token, dtype)
        self.input_layernorm = RMSNorm(config.hidden_size, eps=config.rms_norm_eps)
        self.post_attention_layernorm = RMSNorm(config.hidden_size, eps=config.rms_norm_eps)


class LlamaModel(llama.LlamaModel):
    layer_class = LlamaDecoderLayer


class LlamaMoEForCausalLM(llama.LlamaForCausalLM):
    """llama_moe.py:243-368.  The inherited loaders go by parameter names alone: the per-expert parameters are views
    of the stacked tensors, so ``moe.mlp.{i}.gate_proj`` / ``up_proj`` are stacked into ``gate_up_proj``
    (llama_moe.py:317-358) and copied straight into expert i's slot; ``moe.gate.weight`` is copied whole."""
    model_class = LlamaModel
    has_pooler = False

    def __init__(self, config, dtype=None):
        if get_tensor_model_parallel_world_size() > 1:
            raise NotImplementedError("Llama-MoE under tensor parallelism (TP > 1) is out of scope")
        super().__init__(config, dtype)

    @torch.no_grad()
    def forward(self, input_ids, positions, forward_batch: ForwardBatch,
                input_embeds: torch.Tensor = None) -> LogitsProcessorOutput:
        return super().forward(input_ids, positions, forward_batch, input_embeds)
