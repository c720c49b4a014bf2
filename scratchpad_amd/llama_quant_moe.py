"""Llama with compressed experts over a dense base MLP, hosted on the HIP hot path.

Re-hosts nn/models/llama/llama_quant_moe.py (LlamaMLP 39-74, LLamaSBmm 77-128, LlamaCompressedMLP 131-167, LlamaMoE
170-257, LlamaDecoderLayer 260-330, LlamaModel 333-378, LlamaQuantisedMoEForCausalLM 381-) and
llama_naive_quant_moe.py (LlamaCompressedMLP 71-101, LlamaMoE 104-163, LlamaNaiveQuantisedMoEForCausalLM 286-): Llama
with one extra feed-forward block per layer.  A dense ``moe.base_mlp`` (llama.py's LlamaMLP, fused paths untouched) is
always applied; on top of it the router ``moe.gate`` ([E, H]) picks ``experts_per_token`` of ``num_experts`` experts,
each a gate_up / down pair stored 4-bit and 2:4 sparse with one scale per output row:

    out = sum_k w_k * expert_k(x) + base_mlp(x)

What it adds to llama.py's skeleton is the feed-forward block ``moe``, the packed-expert loaders and the refusals of
its constructors, exactly as llama_moe.py does; attention, norms, embedding and LM head are llama.py's.

The experts are stored in THIS library's packed layout (scratchpad_amd/delta.py: ``codes`` / ``meta`` / ``scales``),
stacked over the experts, as uint8 / dtype BUFFERS (ModelRunner.load_model casts and re-draws parameters):

    sbmm variant    moe.mlp.gate_up_proj.{codes,meta,scales}      [E, 2 I, H / 4], [E, 2 I, H / 8], [E, 2 I]
                    moe.mlp.down_proj.{codes,meta,scales}         [E, H, I / 4],   [E, H, I / 8],   [E, H]
    naive variant   moe.mlp.{i}.gate_up_proj.{codes,meta,scales}  views of expert i's slot of the same stacked storage
                    moe.mlp.{i}.down_proj.{codes,meta,scales}

The reference's ``qweight`` / ``meta`` / ``workspace`` triple is in triteia's Marlin tile order: a state dict that
carries it is refused by name.  A freshly built model holds code 8 / valid meta / scale 1, so its experts add exactly
0; ``init_weights=True`` (ModelRunner) fills them with seeded random valid packed values.

A layer is the base MLP, the router projection and five launches whose grids depend on the batch shape alone
(sp_moe_route's two, then csrc/quant_moe.hip: grouped packed gate_up + SiLU-mul, grouped packed down, combine onto the
base output); a captured step follows the routing of every replay.  The two variants differ in the order the K expert
outputs of a token are added: rank order k = 0 .. K-1 (sbmm) or ascending expert index (naive).  Both route through
sp_moe_route, and the sbmm variant's un-sort is built as intended (DESIGN.md 4.6d states both choices).
``config.sbmm_type`` (naive / multilaunch / forloop) is accepted and ignored: all three are one arithmetic.

Refused with NotImplementedError at construction: tensor parallelism (TP > 1), fp32 (the kernels are 16-bit and there
is no eager form), ``grouped_topk``, more than 64 experts or more than 8 experts per token.  Embedding requests,
toppings and ``expert_layout=None`` are refused by ModelConfig / ModelRunner."""
from typing import Dict, Iterable, Tuple

import torch
from torch import nn

from . import _native, llama
from .delta import ZERO_CODE, ZERO_META, pack_delta
from .distributed import get_tensor_model_parallel_world_size
from .layers import RMSNorm
from .llama import LlamaAttention, LlamaMLP  # noqa: F401  (LlamaMLP: the reference's name for the base MLP)

PACKED_LEAVES = ("codes", "meta", "scales")
_VALID_NIBBLES = (0x4, 0x8, 0xC, 0x9, 0xD, 0xE)          # p0 | p1 << 2 for every p0 < p1


def pack_experts_from_dense(w13: torch.Tensor, w2: torch.Tensor, dtype: torch.dtype):
    """((codes, meta, scales) of gate_up, (codes, meta, scales) of down) stacked over the experts, from dense w13
    [E, 2 I, H] (gate rows first) and w2 [E, H, I]: ``pack_delta`` per expert (round-to-nearest magnitude pruning).  On
    the CPU; for tests and the bench."""
    if w13.dim() != 3 or w2.dim() != 3 or w13.shape[0] != w2.shape[0]:
        raise ValueError("pack_experts_from_dense takes w13 [E, 2 I, H] and w2 [E, H, I]")
    out = []
    for w in (w13, w2):
        parts = [pack_delta(w[e].float(), dtype) for e in range(w.shape[0])]
        out.append(tuple(torch.stack([p[i] for p in parts]).contiguous() for i in range(3)))
    return out[0], out[1]


def _empty_packed(E: int, N: int, K: int, dtype):
    return (torch.full((E, N, K // 4), ZERO_CODE, dtype=torch.uint8),
            torch.full((E, N, K // 8), ZERO_META, dtype=torch.uint8), torch.ones((E, N), dtype=dtype))


class _PackedLinear(nn.Module):
    """packed projection(s): ``codes`` / ``meta`` / ``scales`` buffers (stacked over the experts, or one expert's
    views of the stacked storage)"""

    def __init__(self, codes: torch.Tensor, meta: torch.Tensor, scales: torch.Tensor):
        super().__init__()
        self.register_buffer("codes", codes)
        self.register_buffer("meta", meta)
        self.register_buffer("scales", scales)

    def packed(self):
        return self.codes, self.meta, self.scales


class LLamaSBmm(_PackedLinear):
    """llama_quant_moe.py:77-128: every expert's projection in one module (the reference's spelling)"""


class SparseLowPrecisionLinear(_PackedLinear):
    """what triteia's ``sparse_low_precision_linear`` returns (llama_naive_quant_moe.py:83-91): one expert's"""


class LlamaCompressedMLP(nn.Module):
    """names and shapes only - the arithmetic is the layer's"""

    def __init__(self, gate_up, down, linear_class):
        super().__init__()
        self.gate_up_proj = linear_class(*gate_up)
        self.down_proj = linear_class(*down)


class LlamaMoE(nn.Module):
    order = _native.QMOE_ORDER_RANK        # sbmm: the K outputs of a token are added in rank order
    naive = False

    def __init__(self, hidden_size: int, intermediate_size: int, hidden_act: str, num_experts: int,
                 experts_per_token: int, dtype=None):
        super().__init__()
        if get_tensor_model_parallel_world_size() > 1:
            raise NotImplementedError("Llama-Quant-MoE under tensor parallelism (TP > 1) is out of scope")
        if dtype not in (torch.float16, torch.bfloat16):
            raise NotImplementedError(f"Llama-Quant-MoE in {dtype}: the expert kernels are fp16 / bf16 (there is no "
                                      "eager form)")
        if not 0 < num_experts <= _native.MOE_MAX_EXPERTS:
            raise NotImplementedError(f"num_experts={num_experts}: 1 .. {_native.MOE_MAX_EXPERTS} are built")
        if not 0 < experts_per_token <= min(num_experts, _native.MOE_MAX_TOP_K):
            raise NotImplementedError(f"experts_per_token={experts_per_token}: 1 .. min(num_experts, "
                                      f"{_native.MOE_MAX_TOP_K}) are built")
        if hidden_size % 64 or intermediate_size % 64:
            raise NotImplementedError(f"hidden_size={hidden_size}, intermediate_size={intermediate_size}: the packed "
                                      "expert kernels take multiples of 64")
        self.experts_per_token = experts_per_token
        self.num_experts = num_experts
        self.base_mlp = LlamaMLP(hidden_size, intermediate_size, hidden_act, dtype)
        p13 = _empty_packed(num_experts, 2 * intermediate_size, hidden_size, dtype)
        p2 = _empty_packed(num_experts, hidden_size, intermediate_size, dtype)
        if self.naive:
            # the stacked storage the kernels read: plain attributes, so state_dict keeps the reference's names
            self._p13, self._p2 = p13, p2
            self.mlp = nn.ModuleList([LlamaCompressedMLP([t[i] for t in p13], [t[i] for t in p2],
                                                         SparseLowPrecisionLinear) for i in range(num_experts)])
        else:
            self.mlp = LlamaCompressedMLP(p13, p2, LLamaSBmm)
        self.gate = nn.Linear(hidden_size, num_experts, bias=False, dtype=dtype)
        self.gate.weight.requires_grad_(False)

    # ---- the stacked storage
    def pack_experts(self) -> None:
        """naive variant: (re)build the stacked tensors from the per-expert buffers and make those views of them again;
        needed once after anything that moved or replaced the buffers (``.to(device)``)."""
        if not self.naive:
            return
        for proj, attr in (("gate_up_proj", "_p13"), ("down_proj", "_p2")):
            stacked = tuple(torch.stack([getattr(getattr(m, proj), leaf) for m in self.mlp]) for leaf in PACKED_LEAVES)
            for i, m in enumerate(self.mlp):
                for leaf, t in zip(PACKED_LEAVES, stacked):
                    setattr(getattr(m, proj), leaf, t[i])
            setattr(self, attr, stacked)

    def _packed(self) -> bool:
        if not self.naive:
            return True
        a, b = self.mlp[0], self.mlp[-1]
        return (a.gate_up_proj.codes.data_ptr() == self._p13[0][0].data_ptr()
                and b.down_proj.scales.data_ptr() == self._p2[2][-1].data_ptr())

    def packed(self):
        """((codes, meta, scales) of gate_up, the same of down), stacked over the experts"""
        if self.naive:
            if not self._packed():
                self.pack_experts()
            return self._p13, self._p2
        return self.mlp.gate_up_proj.packed(), self.mlp.down_proj.packed()

    @torch.no_grad()
    def init_expert_weights(self, generator: torch.Generator) -> None:
        """seeded random VALID packed values: codes 0..15, every meta nibble p0 < p1, small positive scales"""
        p13, p2 = self.packed()
        for codes, meta, scales in (p13, p2):
            dev = codes.device
            codes.copy_(torch.randint(0, 256, codes.shape, generator=generator, device=dev, dtype=torch.int32))
            nib = torch.tensor(_VALID_NIBBLES, device=dev, dtype=torch.int32)
            lo = nib[torch.randint(0, 6, meta.shape, generator=generator, device=dev)]
            hi = nib[torch.randint(0, 6, meta.shape, generator=generator, device=dev)]
            meta.copy_(lo | (hi << 4))
            scales.copy_(0.002 + 0.004 * torch.rand(scales.shape, generator=generator, device=dev))

    def forward(self, x: torch.Tensor, reduce_output: bool = True) -> torch.Tensor:
        """reduce_output: the layer protocol's keyword; there are no partial sums to leave (TP > 1 is refused)"""
        shape = x.shape
        x = x.reshape(-1, shape[-1])
        p13, p2 = self.packed()
        base = self.base_mlp(x)
        router_logits = _native.linear(x, self.gate.weight)
        out = _native.qmoe_experts(x, router_logits, p13, p2, self.experts_per_token, self.order, base)
        return out.view(shape)


class LlamaNaiveMoE(LlamaMoE):
    """llama_naive_quant_moe.py:104-163 (there: LlamaMoE): per-expert modules, outputs added in ascending expert index"""
    order = _native.QMOE_ORDER_EXPERT
    naive = True


class LlamaDecoderLayer(llama.LlamaDecoderLayer):
    """llama_quant_moe.py:260-330; ``forward`` is llama.py's LlamaDecoderLayer's over ``moe``"""
    feed_forward_name = "moe"
    moe_class = LlamaMoE

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
        self.moe = self.moe_class(self.hidden_size, config.intermediate_size, config.hidden_act, config.num_experts,
                                  config.experts_per_token, dtype)
        self.input_layernorm = RMSNorm(config.hidden_size, eps=config.rms_norm_eps)
        self.post_attention_layernorm = RMSNorm(config.hidden_size, eps=config.rms_norm_eps)


class LlamaNaiveDecoderLayer(LlamaDecoderLayer):
    moe_class = LlamaNaiveMoE


class LlamaModel(llama.LlamaModel):
    layer_class = LlamaDecoderLayer


class LlamaNaiveModel(llama.LlamaModel):
    layer_class = LlamaNaiveDecoderLayer


class LlamaQuantisedMoEForCausalLM(llama.LlamaForCausalLM):
    """llama_quant_moe.py:381-.  Parameters load through the inherited loaders by name; the packed experts are buffers
    and are filled by name here.  ``gate_proj`` | ``up_proj`` stack by rows (the expert dimension, where a tensor has
    one, stays in front)."""
    model_class = LlamaModel
    has_pooler = False

    def __init__(self, config, dtype=None):
        if get_tensor_model_parallel_world_size() > 1:
            raise NotImplementedError("Llama-Quant-MoE under tensor parallelism (TP > 1) is out of scope")
        super().__init__(config, dtype)

    def moe_blocks(self):
        return [layer.moe for layer in self.model.layers]

    def expert_buffers(self) -> Dict[str, torch.Tensor]:
        """the packed experts by state-dict name"""
        for moe in self.moe_blocks():
            moe.packed()        # (naive variant: the per-expert buffers are views of the stacked storage again)
        return {n: b for n, b in self.named_buffers() if ".moe.mlp." in n and n.rsplit(".", 1)[1] in PACKED_LEAVES}

    def init_expert_weights(self, generator: torch.Generator) -> None:
        for moe in self.moe_blocks():
            moe.init_expert_weights(generator)

    def load_full_state_dict(self, full: Dict[str, torch.Tensor]) -> None:
        for name in full:
            if ".moe." in name and name.rsplit(".", 1)[1] in ("qweight", "workspace"):
                raise NotImplementedError(f"{name}: the reference's qweight / meta / workspace triple is in triteia's "
                                          "Marlin tile order, which is not converted; the experts are read in this "
                                          "library's packed layout (codes / meta / scales, scratchpad_amd/delta.py)")
        super().load_full_state_dict(full)
        for name, buf in self.expert_buffers().items():
            src = full[name]
            if src.shape != buf.shape:
                raise RuntimeError(f"{name}: shape {tuple(src.shape)} != {tuple(buf.shape)}")
            if name.endswith("scales"):
                src = src.to(buf.dtype)
            elif src.dtype != torch.uint8:
                raise RuntimeError(f"{name}: packed bytes are uint8, not {src.dtype}")
            buf.copy_(src)

    def load_weights(self, weights: Iterable[Tuple[str, torch.Tensor]]) -> None:
        """llama.py's load_weights with the stacking dimension of the packed tensors: rows, i.e. the last dimension of
        ``scales`` and the one before the last of ``codes`` / ``meta``"""
        staged: Dict[Tuple[str, str], Dict[str, torch.Tensor]] = {}
        full: Dict[str, torch.Tensor] = {}
        for name, w in weights:
            for merged, tag in ((m, t) for m, tags in self.stacked_params.items() for t in tags):
                if "." + tag + "." in name:
                    staged.setdefault((name.replace(tag, merged), merged), {})[tag] = w
                    break
            else:
                full[name] = w
        for (name, merged), parts in staged.items():
            leaf = name.rsplit(".", 1)[1]
            first = parts[self.stacked_params[merged][0]]
            dim = 0 if leaf not in PACKED_LEAVES else first.dim() - (1 if leaf == "scales" else 2)
            full[name] = torch.cat([parts[t] for t in self.stacked_params[merged]], dim)
        self.load_full_state_dict(full)


class LlamaNaiveQuantisedMoEForCausalLM(LlamaQuantisedMoEForCausalLM):
    """llama_naive_quant_moe.py:286-"""
    model_class = LlamaNaiveModel
