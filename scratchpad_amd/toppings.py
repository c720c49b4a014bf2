"""Toppings: many fine-tuned variants of one base model served from one engine, as LoRA adapters or as compressed
full-model deltas.

Re-hosts nn/toppings/topping_module.py (DeltaAdapter 68-118, LoRAAdapter 121-181), nn/toppings/topping_layer.py
(28-391), memory/topping_pool.py (35-172) and managers/toppings_manager.py (76-592) on Llama at TP = 1.  The reference
hands the arithmetic to triteia.python.ops.ldmm (not part of its tree); here it is

* LoRA: ``sp_lora_shrink`` / ``sp_lora_expand`` (csrc/lora.hip): per projection one shrink and one expand (two for
  qkv), whatever the number of adapters in the batch, every row choosing its adapter by an int32 slot index (-1: base
  model only);
* delta (W_finetuned - W_base stored 4-bit and 2:4 sparse, scratchpad_amd/delta.py): ``sp_delta_group`` once per
  forward (the rows of the index vector sorted by slot, on the device) and ONE ``sp_delta_mm`` per wrapped projection
  over its whole stacked output (csrc/delta.hip): 4 launches per layer.

A manager serves LoRA adapters or delta adapters, not both.  Refused, each with a NotImplementedError that names it:
the two kinds in one manager, a delta topping no DeltaAdapter object was handed in for (loading one from a path), the
reference's triteia-layout (qweight, meta, scales) triple as a raw tuple, compress configs other than 4 bit / 2:4,
delta tensors outside the decoder layers' projections (embedding, LM-head and norm swaps), TP > 1.

Nothing here reads files or the network: an adapter is built from a state dict of tensors.
"""
import re
from typing import Dict, Iterable, List, Optional, Tuple

import torch
from torch import nn

from . import _native
from .delta import ZERO_CODE, ZERO_META, empty_delta
from .llama import MergedColumnParallelLinear, QKVParallelLinear, RowParallelLinear, _ShardedLinear


def get_layer_id(name: str) -> Optional[int]:
    m = re.search(r"layers\.(\d+)\.", name)
    return None if m is None else int(m.group(1))


# config module name -> module name in the model (toppings_manager.py:30-42)
_MODULE_NAME = {"q_proj": "qkv_proj", "k_proj": "qkv_proj", "v_proj": "qkv_proj",
                "gate_proj": "gate_up_proj", "up_proj": "gate_up_proj"}
# config module name -> (buffer name of A, buffer name of B) (toppings_manager.py:64-73)
_STACKED_NAME = {"q_proj": ("qkv_proj", "q_proj"), "k_proj": ("qkv_proj", "kv_proj"), "v_proj": ("qkv_proj", "kv_proj"),
                 "gate_proj": ("gate_up_proj", "gate_up_proj"), "up_proj": ("gate_up_proj", "gate_up_proj")}


def get_module_name(name: str) -> str:
    return _MODULE_NAME.get(name, name)


def get_stacked_name(name: str) -> Tuple[str, str]:
    return _STACKED_NAME.get(name, (name, name))


def get_hidden_dim(module_name: str, config) -> Tuple[int, int]:
    """(input width, output width of ONE stacked slice) of a buffer name (topping_pool.py:9-32), with the head
    width read from the config where it has one"""
    D = getattr(config, "head_dim", None) or config.hidden_size // config.num_attention_heads
    if module_name in ("q_proj", "qkv_proj"):
        return config.hidden_size, config.num_attention_heads * D
    if module_name == "o_proj":
        return config.num_attention_heads * D, config.hidden_size
    if module_name == "kv_proj":
        return config.hidden_size, config.num_key_value_heads * D
    if module_name == "gate_up_proj":
        return config.hidden_size, config.intermediate_size
    if module_name == "down_proj":
        return config.intermediate_size, config.hidden_size
    if module_name in ("lm_head", "logits_processor", "embed_tokens"):
        raise NotImplementedError(f"toppings on {module_name} (embedding / LM-head swaps) are out of scope")
    raise NotImplementedError(f"get_hidden_dim for {module_name} is not implemented")


class ToppingConfig:
    """config/topping_config.py: the adapter's type, its name ('path') and its PEFT config as a dict
    (``r``, ``lora_alpha``, ``target_modules``)"""

    def __init__(self, topping_type: str = "lora", path: str = "", hf_config: Optional[dict] = None):
        self.topping_type = topping_type
        self.path = path
        self.hf_config = dict(hf_config or {})


class ToppingLayer:
    def __init__(self):
        self.weights: Dict[str, torch.Tensor] = {}


class LoRAAdapter:
    """topping_module.py:121-181.  ``initialize_weights(state_dict)`` takes the tensors (PEFT names,
    ``...layers.N.self_attn.q_proj.lora_A.weight`` [r, in] / ``lora_B.weight`` [out, r]) and stacks them as the
    reference does: ``qkv_proj.lora_A`` = q|k|v on dim 0, ``kv_proj.lora_B`` = k|v, ``gate_up_proj`` = gate|up for both.
    A projection of a stacked group the adapter does not target enters the stack as zeros."""

    def __init__(self, uid, config: ToppingConfig, base_hf_config, load_config=None):
        self.uid = uid
        self.config = config
        self.base_hf_config = base_hf_config
        self.load_config = load_config
        self.r = int(config.hf_config["r"])
        self.scaling = config.hf_config["lora_alpha"] / config.hf_config["r"]
        self.layers = [ToppingLayer() for _ in range(base_hf_config.num_hidden_layers)]
        self.weights: Dict[str, torch.Tensor] = {}

    def get_stacked_multiply(self, module_name: str) -> int:
        return {"kv_proj": 2, "gate_up_proj": 2, "qkv_proj": 3}.get(module_name, 1)

    def initialize_weights(self, state_dict: Optional[Dict[str, torch.Tensor]] = None) -> "LoRAAdapter":
        if state_dict is None:
            raise NotImplementedError("LoRAAdapter loads from a state dict of tensors: reading checkpoints from files "
                                      "or the network is out of scope")
        for name, w in state_dict.items():
            lid = get_layer_id(name)
            if lid is None:
                self.weights[name] = w.detach().cpu()
            else:
                self.layers[lid].weights[name] = w.detach().cpu()
        cfg = self.base_hf_config
        for layer in self.layers:
            self._stack(layer, ("q_proj", "k_proj", "v_proj"), "qkv_proj", ("k_proj", "v_proj"), "kv_proj", cfg)
            self._stack(layer, ("gate_proj", "up_proj"), "gate_up_proj", ("gate_proj", "up_proj"), "gate_up_proj", cfg)
        return self

    def _stack(self, layer: ToppingLayer, a_parts, a_name, b_parts, b_name, cfg) -> None:
        D = getattr(cfg, "head_dim", None) or cfg.hidden_size // cfg.num_attention_heads
        kv = cfg.num_key_value_heads * D
        # part -> (input width, output width): the shape of the zeros a part the adapter does not target stands for
        widths = {"q_proj": (cfg.hidden_size, cfg.num_attention_heads * D), "k_proj": (cfg.hidden_size, kv),
                  "v_proj": (cfg.hidden_size, kv), "gate_proj": (cfg.hidden_size, cfg.intermediate_size),
                  "up_proj": (cfg.hidden_size, cfg.intermediate_size)}
        for kind, parts, stacked in (("lora_A", a_parts, a_name), ("lora_B", b_parts, b_name)):
            found = {p: name for p in parts for name in layer.weights if f".{p}.{kind}" in name}
            if not found:
                continue
            first = next(iter(found))
            template, dtype = found[first], layer.weights[found[first]].dtype
            tensors = []
            for p in parts:
                if p in found:
                    tensors.append(layer.weights.pop(found[p]))
                else:
                    shape = (self.r, widths[p][0]) if kind == "lora_A" else (widths[p][1], self.r)
                    tensors.append(torch.zeros(shape, dtype=dtype))
            layer.weights[template.replace(f".{first}.", f".{stacked}.")] = torch.cat(tensors, 0)


class DeltaBuffer:
    """What ``set_topping_info(delta_buffer=...)`` takes: the packed delta slots of ONE projection of one layer in this
    library's layout (scratchpad_amd/delta.py) - codes uint8 [slots, N, K / 4], meta uint8 [slots, N, K / 8], scales
    [slots, N].  Not a tuple on purpose: a raw tuple is the reference's triteia-layout triple, which is refused."""
    __slots__ = ("codes", "meta", "scales")

    def __init__(self, codes: torch.Tensor, meta: torch.Tensor, scales: torch.Tensor):
        if codes.dim() != 3 or meta.dim() != 3 or scales.dim() != 2 or codes.dtype != torch.uint8 \
                or meta.dtype != torch.uint8 or codes.shape[:2] != meta.shape[:2] or codes.shape[:2] != scales.shape \
                or codes.shape[2] != 2 * meta.shape[2]:
            raise ValueError("DeltaBuffer: codes uint8 [slots, N, K / 4], meta uint8 [slots, N, K / 8], scales "
                             f"[slots, N]; got {tuple(codes.shape)}, {tuple(meta.shape)}, {tuple(scales.shape)}")
        self.codes, self.meta, self.scales = codes, meta, scales


_DELTA_PROJ = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
_DELTA_STACKS = {"qkv_proj": ("q_proj", "k_proj", "v_proj"), "gate_up_proj": ("gate_proj", "up_proj")}
_DELTA_MEMBERS = ("codes", "meta", "scales")


def delta_proj_shape(proj: str, cfg) -> Tuple[int, int]:
    """(output rows N, input width K) of one HF projection's dense delta"""
    D = getattr(cfg, "head_dim", None) or cfg.hidden_size // cfg.num_attention_heads
    q, kv = cfg.num_attention_heads * D, cfg.num_key_value_heads * D
    return {"q_proj": (q, cfg.hidden_size), "k_proj": (kv, cfg.hidden_size), "v_proj": (kv, cfg.hidden_size),
            "o_proj": (cfg.hidden_size, q), "gate_proj": (cfg.intermediate_size, cfg.hidden_size),
            "up_proj": (cfg.intermediate_size, cfg.hidden_size),
            "down_proj": (cfg.hidden_size, cfg.intermediate_size)}[proj]


def delta_module_shape(module: str, cfg) -> Tuple[int, int]:
    """(N, K) of a model module's delta: the stacked rows of its projections"""
    parts = _DELTA_STACKS.get(module, (module,))
    return sum(delta_proj_shape(p, cfg)[0] for p in parts), delta_proj_shape(parts[0], cfg)[1]


class DeltaAdapter:
    """topping_module.py:68-118.  ``initialize_weights(state_dict)`` takes the packed tensors of scratchpad_amd/delta.py
    under ``...layers.N.self_attn.q_proj.codes`` / ``.meta`` / ``.scales`` (and k_proj, v_proj, o_proj, mlp.gate_proj,
    up_proj, down_proj) and stacks q|k|v and gate|up by rows - the format is row-local, so stacking is concatenation.
    A projection of a stacked group the adapter does not carry enters the stack as zeros (code 8, scale 1).
    ``layers[i].weights`` is keyed by the name behind ``layers.i.`` with the module name of the model
    (``self_attn.qkv_proj.codes``)."""

    def __init__(self, uid, config: ToppingConfig, base_hf_config, load_config=None):
        self.uid = uid
        self.config = config
        self.base_hf_config = base_hf_config
        self.load_config = load_config
        cc = dict(config.hf_config.get("compress_config") or {"bits": 4, "sparsity": 0.5})
        if cc.get("bits", 4) != 4 or cc.get("sparsity", 0.5) != 0.5:
            raise NotImplementedError(f"delta compress_config {cc}: only bits = 4, sparsity = 0.5 (2:4) deltas are "
                                      "served (2-bit and dense deltas are out of scope)")
        self.pack_factor = 32 // 4
        self.sparse_factor = 2
        self.layers = [ToppingLayer() for _ in range(base_hf_config.num_hidden_layers)]
        self.target_modules: set = set()       # the model modules this adapter carries a delta for

    def get_stacked_multiply_delta(self, module_name: str) -> int:
        return {"kv_proj": 2, "gate_up_proj": 2, "qkv_proj": 3}.get(module_name, 1)

    def get_pack_factor(self) -> int:
        return self.pack_factor

    def get_sparse_factor(self) -> int:
        return self.sparse_factor

    def initialize_weights(self, state_dict: Optional[Dict[str, torch.Tensor]] = None) -> "DeltaAdapter":
        if state_dict is None:
            raise NotImplementedError("DeltaAdapter loads from a state dict of packed tensors: reading deltazip "
                                      "checkpoints from files or the network is out of scope")
        cfg = self.base_hf_config
        found: List[Dict[str, Dict[str, torch.Tensor]]] = [dict() for _ in self.layers]
        for name, w in state_dict.items():
            lid = get_layer_id(name)
            m = re.search(r"layers\.\d+\.((?:self_attn|mlp)\.(\w+))\.(\w+)$", name)
            if lid is None or m is None or m.group(2) not in _DELTA_PROJ:
                raise NotImplementedError(f"delta tensor {name!r}: only the decoder layers' projections {_DELTA_PROJ} "
                                          "take a delta (embed_tokens, lm_head and norm swaps - the reference's "
                                          "outside_layer_modules / uncompressed_delta_target_weights - are out of "
                                          "scope)")
            if m.group(3) not in _DELTA_MEMBERS:
                raise NotImplementedError(f"delta tensor {name!r}: a projection carries codes, meta and scales (the "
                                          "reference's triteia-layout qweight / metas are not converted)")
            if not 0 <= lid < len(self.layers):
                raise ValueError(f"{name}: the model has {len(self.layers)} layers")
            found[lid].setdefault(m.group(2), {})[m.group(3)] = w.detach().cpu()
        for lid, projs in enumerate(found):
            for proj, members in projs.items():
                N, K = delta_proj_shape(proj, cfg)
                want = {"codes": (N, K // 4), "meta": (N, K // 8), "scales": (N,)}
                for k in _DELTA_MEMBERS:
                    if k not in members:
                        raise ValueError(f"layer {lid} {proj}: {k} is missing")
                    if tuple(members[k].shape) != want[k]:
                        raise ValueError(f"layer {lid} {proj}.{k}: {tuple(members[k].shape)}, expected {want[k]}")
                    if k != "scales" and members[k].dtype != torch.uint8:
                        raise ValueError(f"layer {lid} {proj}.{k}: uint8 expected, got {members[k].dtype}")
            for module, block in (("qkv_proj", "self_attn"), ("o_proj", "self_attn"), ("gate_up_proj", "mlp"),
                                  ("down_proj", "mlp")):
                parts = _DELTA_STACKS.get(module, (module,))
                if not any(p in projs for p in parts):
                    continue
                dtype = next(projs[p]["scales"].dtype for p in parts if p in projs)
                stack = [projs[p] if p in projs else dict(zip(_DELTA_MEMBERS, empty_delta(*delta_proj_shape(p, cfg), dtype)))
                         for p in parts]
                for k in _DELTA_MEMBERS:
                    self.layers[lid].weights[f"{block}.{module}.{k}"] = torch.cat([s[k] for s in stack], 0).contiguous()
                self.target_modules.add(module)
        return self


class ToppingMemPool:
    """topping_pool.py:35-124, the LoRA half: ``A_buffer[module][layer]`` is [slots, in, r * c] and
    ``B_buffer[module][layer]`` is [slots, r, out * c] (c = stacked slices of the module), in the model dtype,
    allocated ONCE and zeroed: every address a captured graph holds stays valid, and an unloaded slot adds 0.
    The layers of a module are views of one [layers, slots, ., .] allocation (``A_all`` / ``B_all``), so that
    loading an adapter into a slot is one copy per module.

    topping_pool.py:126-172, the delta half (``deltas`` given): per model module of ``delta_target_weights`` ONE
    allocation each for codes, meta and scales - ``qweight_all[module]`` uint8 [layers, slots, N, K / 4],
    ``meta_all[module]`` uint8 [layers, slots, N, K / 8], ``scales_all[module]`` [layers, slots, N] in the model dtype -
    with per-layer views ``qweight_buffer`` / ``meta_buffer`` / ``scales_buffer`` [module][layer] (the reference's
    names; the layout is this library's, scratchpad_amd/delta.py).  Allocated once; an empty slot holds code 8 and
    scale 1 and adds exactly 0."""

    def __init__(self, args, base_hf_config, loras: List[LoRAAdapter], target_weights, max_toppings_per_batch: int,
                 max_lora_dim: int, base_model=None, lora_dtype: torch.dtype = torch.bfloat16, device="cuda",
                 deltas=None, delta_target_weights=None, uncompressed_delta_target_weights=None):
        if uncompressed_delta_target_weights:
            raise NotImplementedError("uncompressed delta target weights (embedding / LM-head / norm swaps) are out of "
                                      "scope")
        if deltas and loras:
            raise NotImplementedError("LoRA and delta toppings in one pool are out of scope")
        self.args = args
        self.base_model = base_model
        self.base_hf_config = base_hf_config
        self.loras = loras
        self.target_weights = target_weights
        self.max_toppings_per_batch = max_toppings_per_batch
        self.max_lora_dim = max_lora_dim
        self.lora_dtype = lora_dtype
        self.A_buffer: Dict[str, List[torch.Tensor]] = {}
        self.B_buffer: Dict[str, List[torch.Tensor]] = {}
        self.A_all: Dict[str, torch.Tensor] = {}
        self.B_all: Dict[str, torch.Tensor] = {}
        num_layers = base_hf_config.num_hidden_layers
        for module_A, module_B in sorted(self.target_weights):
            dim_A, _ = get_hidden_dim(module_A, base_hf_config)
            c = loras[-1].get_stacked_multiply(module_A)
            if module_A not in self.A_buffer:
                self.A_all[module_A] = torch.zeros((num_layers, max_toppings_per_batch, dim_A, max_lora_dim * c),
                                                   dtype=lora_dtype, device=device)
                self.A_buffer[module_A] = list(self.A_all[module_A].unbind(0))
            _, dim_B = get_hidden_dim(module_B, base_hf_config)
            c = loras[-1].get_stacked_multiply(module_B)
            if module_B not in self.B_buffer:
                self.B_all[module_B] = torch.zeros((num_layers, max_toppings_per_batch, max_lora_dim, dim_B * c),
                                                   dtype=lora_dtype, device=device)
                self.B_buffer[module_B] = list(self.B_all[module_B].unbind(0))
        self.deltas = list(deltas or [])
        self.delta_target_weights = sorted(delta_target_weights or []) if self.deltas else []
        self.qweight_all: Dict[str, torch.Tensor] = {}
        self.meta_all: Dict[str, torch.Tensor] = {}
        self.scales_all: Dict[str, torch.Tensor] = {}
        self.qweight_buffer: Dict[str, List[torch.Tensor]] = {}
        self.meta_buffer: Dict[str, List[torch.Tensor]] = {}
        self.scales_buffer: Dict[str, List[torch.Tensor]] = {}
        for module in self.delta_target_weights:
            N, K = delta_module_shape(module, base_hf_config)
            if K % 64 != 0 or N % 16 != 0:
                raise NotImplementedError(f"delta toppings on {module} [{N}, {K}]: sp_delta_mm serves input widths "
                                          "that are multiples of 64 and output widths that are multiples of 16")
            shape = (num_layers, max_toppings_per_batch, N)
            self.qweight_all[module] = torch.full(shape + (K // 4,), ZERO_CODE, dtype=torch.uint8, device=device)
            self.meta_all[module] = torch.full(shape + (K // 8,), ZERO_META, dtype=torch.uint8, device=device)
            self.scales_all[module] = torch.ones(shape, dtype=lora_dtype, device=device)
            self.qweight_buffer[module] = list(self.qweight_all[module].unbind(0))
            self.meta_buffer[module] = list(self.meta_all[module].unbind(0))
            self.scales_buffer[module] = list(self.scales_all[module].unbind(0))

    def delta_buffer(self, module: str, layer_id: int) -> Optional[DeltaBuffer]:
        if module not in self.qweight_buffer:
            return None
        return DeltaBuffer(self.qweight_buffer[module][layer_id], self.meta_buffer[module][layer_id],
                           self.scales_buffer[module][layer_id])


# --------------------------------------------------------------------------- layers
class BaseLayerWithTopping(nn.Module):
    """topping_layer.py:28-39.  ``has_toppings`` tells the callers that fuse a projection with what follows it
    (LlamaMLP's gate_up + SiLU launch) to keep the projection on its own: the delta lands before the activation."""
    has_toppings = True

    def __init__(self, base_layer, config: Dict):
        super().__init__()
        self.base_layer = base_layer
        self.config = config
        self.set_topping = False
        self.weight_indices = None
        self.scaling = 1.0
        self.delta: Optional[DeltaBuffer] = None
        self.delta_groups = None

    @property
    def weight(self):
        return self.base_layer.weight

    def forward(self, x: torch.Tensor):
        return self.base_layer.forward(x)

    def set_topping_info(self, *args, **kwargs):
        ...

    @staticmethod
    def _delta(name: str, b) -> Optional[DeltaBuffer]:
        if b is None or isinstance(b, DeltaBuffer):
            return b
        raise NotImplementedError(f"delta toppings: {name} must be a DeltaBuffer (codes, meta, scales in this library's "
                                  "layout) or None; a raw tuple is the reference's triteia-layout triple, whose "
                                  "conversion is out of scope")

    def _set_delta(self, delta: Optional[DeltaBuffer], delta_groups) -> None:
        """the packed slots of this projection and the manager's persistent (slot_offsets, sorted_rows)"""
        if delta is not None and delta_groups is None:
            raise ValueError("a delta_buffer goes with delta_groups = (slot_offsets, sorted_rows)")
        self.delta = delta
        self.delta_groups = tuple(delta_groups) if delta is not None else None

    def _add_packed_delta(self, x: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        """out += x . delta[slot of the row]^T over the whole (stacked) output: ONE launch"""
        d = self.delta
        _native.delta_mm(out, x, d.codes, d.meta, d.scales, self.delta_groups[0], self.delta_groups[1])
        return out

    def _tokens(self, x: torch.Tensor) -> torch.Tensor:
        if self.weight_indices is None:
            raise RuntimeError(f"{type(self).__name__}: set_topping_info() has not been called")
        return self.weight_indices[: x.shape[0]] if self.weight_indices.shape[0] != x.shape[0] else self.weight_indices


class ColumnParallelLinearWithTopping(BaseLayerWithTopping):
    """topping_layer.py:73-108: out += (x . A[idx]) . B[idx], one shrink and one expand in place on the base output"""
    num_slices = 1

    def set_topping_info(self, bs, weight_indices, lora_buffer=None, delta_buffer=None, scaling=None,
                         delta_groups=None):
        self._set_delta(self._delta("delta_buffer", delta_buffer), delta_groups)
        self.weight_indices = weight_indices
        self.A_buffer, self.B_buffer = (None, None) if lora_buffer is None else (lora_buffer[0], lora_buffer[1])
        if scaling is not None:
            self.scaling = float(scaling)
        self.set_topping = True

    def _add_delta(self, x: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        if self.delta is not None:
            self._add_packed_delta(x, out)
        if self.A_buffer is None or self.B_buffer is None:
            return out
        idx = self._tokens(x)
        tmp = _native.lora_shrink(x, self.A_buffer, idx, self.scaling)
        _native.lora_expand(out, tmp, self.B_buffer, idx, self.num_slices)
        return out

    def forward(self, input_: torch.Tensor):
        out = self.base_layer(input_)[0]
        return self._add_delta(input_, out), None


class MergedColumnParallelLinearWithTopping(ColumnParallelLinearWithTopping):
    """topping_layer.py:111-155: gate|up - one shrink (R = 2 r) and one expand over both slices"""
    num_slices = 2


class QKVParallelLinearWithToppings(ColumnParallelLinearWithTopping):
    """topping_layer.py:158-241: one shrink over the stacked q|k|v A (R = 3 r), an expand of q and an expand of the
    two kv slices (tmp offset by r, the output offset by the q width)"""

    def set_topping_info(self, bs, weight_indices, lora_buffer=None, delta_buffer_q=None, delta_buffer_kv=None,
                         scaling=None, delta_groups=None):
        """``delta_buffer_q``: the DeltaBuffer of the whole stacked q|k|v output (one launch); the reference's separate
        kv triple has no counterpart, so ``delta_buffer_kv`` stays None"""
        q = self._delta("delta_buffer_q", delta_buffer_q)
        if self._delta("delta_buffer_kv", delta_buffer_kv) is not None:
            raise NotImplementedError("delta toppings: q|k|v is ONE stacked delta_buffer_q here; a separate "
                                      "delta_buffer_kv is not served")
        self._set_delta(q, delta_groups)
        self.weight_indices = weight_indices
        self.A_buffer_qkv, self.B_buffer_q, self.B_buffer_kv = (None, None, None) if lora_buffer is None else lora_buffer
        if scaling is not None:
            self.scaling = float(scaling)
        self.set_topping = True

    def forward(self, input_: torch.Tensor):
        out = self.base_layer(input_)[0]
        if self.delta is not None:
            self._add_packed_delta(input_, out)
        if self.A_buffer_qkv is None:
            return out, None
        idx = self._tokens(input_)
        tmp = _native.lora_shrink(input_, self.A_buffer_qkv, idx, self.scaling)
        r = self.A_buffer_qkv.shape[2] // 3
        q_dim = 0
        if self.B_buffer_q is not None:
            q_dim = self.B_buffer_q.shape[2]
            _native.lora_expand(out[:, :q_dim], tmp[:, :r], self.B_buffer_q, idx, 1)
        else:
            q_dim = out.shape[1] - (self.B_buffer_kv.shape[2] if self.B_buffer_kv is not None else 0)
        if self.B_buffer_kv is not None:
            _native.lora_expand(out[:, q_dim:], tmp[:, r:], self.B_buffer_kv, idx, 2)
        return out, None


class RowParallelLinearWithTopping(ColumnParallelLinearWithTopping):
    """topping_layer.py:244-294, keeping this project's ``reduce_output`` (TP = 1: there is nothing to reduce; the
    delta is added to this rank's output before the base layer would have reduced it, so TP > 1 is refused)"""

    def set_topping_info(self, bs, weight_indices, lora_buffer=None, delta_buffer=None, debug=False, scaling=None,
                         delta_groups=None):
        super().set_topping_info(bs, weight_indices, lora_buffer=lora_buffer, delta_buffer=delta_buffer,
                                 scaling=scaling, delta_groups=delta_groups)

    def forward(self, input_: torch.Tensor, reduce_output: bool = True):
        if getattr(self.base_layer, "tp_size", 1) > 1:
            raise NotImplementedError("toppings under tensor parallelism (TP > 1) are out of scope")
        out = self.base_layer(input_, reduce_output)[0]
        return self._add_delta(input_, out), None


def get_topping_layer(layer: nn.Module) -> BaseLayerWithTopping:
    """topping_layer.py:377-391 over this project's linears (llama.py); the order matters"""
    supported = ((QKVParallelLinear, QKVParallelLinearWithToppings),
                 (MergedColumnParallelLinear, MergedColumnParallelLinearWithTopping),
                 (RowParallelLinear, RowParallelLinearWithTopping),
                 (_ShardedLinear, ColumnParallelLinearWithTopping))
    for src, dst in supported:
        if isinstance(layer, src):
            return dst(layer, {})
    if type(layer).__name__ in ("VocabParallelEmbedding", "ParallelLMHead", "LogitsProcessor"):
        raise NotImplementedError(f"toppings on {type(layer).__name__} (embedding / LM-head swaps) are out of scope")
    raise Exception(f"No corresponding Topping layer supported for {type(layer)}.")


def replace_submodule(model: nn.Module, module_name: str, new_module: nn.Module) -> nn.Module:
    parent = model.get_submodule(".".join(module_name.split(".")[:-1]))
    setattr(parent, module_name.split(".")[-1], new_module)
    return new_module


# --------------------------------------------------------------------------- manager
class ToppingsManager:
    """managers/toppings_manager.py:76-592 for LoRA adapters or for delta adapters (one kind per manager).

    ``adapters``: LoRAAdapter objects, or DeltaAdapter objects, whose weights are loaded (this takes the place of
    ``server_args.init_toppings`` and the checkpoint loader).  Without adapters, or with ``max_toppings_per_batch``
    unset, the manager is disabled and touches nothing.  All registered LoRA adapters share ``r`` and ``scaling``
    (toppings_manager.py:208-213).

    Delta adapters: next to ``weight_indices`` the manager owns the persistent ``slot_offsets`` [slots + 1] and
    ``sorted_rows`` buffers every topping layer holds.  ``group_topping_batch(num_tokens)`` fills them with ONE
    ``sp_delta_group`` launch from the device index buffer alone: eagerly behind ``prepare_topping_batch``, and inside
    the captured region ahead of the first layer under the graph runner, so a replay follows a changed index vector.

    Three deliberate deviations from the reference's ``prepare_topping_batch``:
      * LoRA is not asserted away (the reference: ``assert len_loras == 0, "LoRA is not supported in this version"``);
      * a prefill batch may hold several requests and several adapters (the reference asserts ``bs == 1``): a
        request's slot is repeated ``extend_seq_lens[i]`` times;
      * the indices need not be sorted: the kernels are correct, and batch-invariant, for any order.
    The per-token index vector lives in ONE persistent int32 buffer (``weight_indices``), which is the tensor every
    topping layer holds; a batch is written into it, never into a fresh tensor, so a captured graph follows it."""

    def __init__(self, server_args, base_model, base_hf_config, load_config=None,
                 adapters: Optional[Iterable[LoRAAdapter]] = None, device=None, dtype: Optional[torch.dtype] = None,
                 tp_size: int = 1, max_tokens: Optional[int] = None):
        self.available_toppings: Dict[str, Tuple[str, str]] = {}
        self.base_model = base_model
        self.base_hf_config = base_hf_config
        self.load_config = load_config
        self.toppings_id: Dict[str, int] = {}
        self.max_toppings_per_batch = getattr(server_args, "max_toppings_per_batch", None)
        adapters = list(adapters or [])
        if not adapters or not self.max_toppings_per_batch:
            self.enabled = False
            return
        if tp_size > 1:
            raise NotImplementedError("toppings under tensor parallelism (TP > 1) are out of scope")
        kinds = {isinstance(a, DeltaAdapter) for a in adapters}
        if len(kinds) > 1:
            raise NotImplementedError("LoRA and delta toppings in one manager are out of scope: a manager serves "
                                      "LoRAAdapter objects or DeltaAdapter objects")
        self.kind = "delta" if kinds == {True} else "lora"
        self.enabled = True
        p = next(iter(base_model.parameters()), None)
        self.device = device if device is not None else (p.device if p is not None else "cpu")
        self.dtype = dtype if dtype is not None else (p.dtype if p is not None else torch.bfloat16)
        self._adapters = {a.uid: a for a in adapters}
        self._staged: Dict[object, Dict[Tuple[int, str], torch.Tensor]] = {}
        for a in adapters:
            self.register_topping(a.config.topping_type, a.config.path, a.uid)
        self.init_topping_batch()
        self.init_toppings()
        self.init_topping_mem_pool(server_args)
        # one entry per token of the largest step; -1 = base model only
        n = max_tokens or max(getattr(server_args, "max_prefill_tokens", 16384), 1)
        self.weight_indices = torch.full((n,), -1, dtype=torch.int32, device=self.device)
        # the grouping of the step's rows by slot (delta adapters): rewritten by every group_topping_batch
        self.slot_offsets = self.sorted_rows = None
        if self.kind == "delta":
            self.slot_offsets = torch.zeros((self.max_toppings_per_batch + 1,), dtype=torch.int32, device=self.device)
            self.sorted_rows = torch.zeros((n,), dtype=torch.int32, device=self.device)
        self._wire_modules()

    # ---- set-up
    def register_topping(self, topping_type, topping_path: str, topping_name: str) -> None:
        kind = str(getattr(topping_type, "value", topping_type))
        if kind not in ("lora", "delta"):
            raise NotImplementedError(f"unknown topping type {topping_type!r}")
        adapter = getattr(self, "_adapters", {}).get(topping_name)
        if kind == "delta" and not isinstance(adapter, DeltaAdapter):
            raise NotImplementedError(f"delta topping {topping_name!r}: no DeltaAdapter object was handed to the "
                                      "manager for it; loading a deltazip checkpoint from a path is out of scope")
        if kind != getattr(self, "kind", kind) or (kind == "lora" and isinstance(adapter, DeltaAdapter)):
            raise NotImplementedError(f"topping {topping_name!r} is registered as {kind!r} with a manager of "
                                      f"{getattr(self, 'kind', 'another kind')!r} adapters: LoRA and delta toppings "
                                      "in one manager are out of scope")
        self.available_toppings[topping_name] = (topping_type, topping_path)

    def init_topping_batch(self) -> None:
        self.active_uids = set()      # adapters that hold a slot
        self.buffer_id = {}           # adapter uid -> slot

    def init_toppings(self) -> None:
        self.configs = {name: self._adapters[name].config for name in self.available_toppings}
        self.loras: List[LoRAAdapter] = []
        self.lora_id: Dict[str, int] = {}
        self.deltas: List[DeltaAdapter] = []
        self.delta_id: Dict[str, int] = {}
        if self.kind == "delta":
            for c in self.configs.values():
                for m in c.hf_config.get("target_modules", ()):
                    if m in ("lm_head", "embed_tokens", "logits_processor", "norm"):
                        raise NotImplementedError(f"toppings on {m} (embedding / LM-head / norm swaps) are out of scope")
            for name in self.available_toppings:
                self.delta_id[name] = self.toppings_id[name] = len(self.deltas)
                self.deltas.append(self._adapters[name])
            self.target_modules = set().union(*(a.target_modules for a in self.deltas))
            if not self.target_modules:
                raise ValueError("the delta adapters carry no tensors (initialize_weights(state_dict) first)")
            self.origin_target_modules = set(self.target_modules)
            self.target_weights = set()
            self.max_lora_dim, self.scaling = 0, 1.0
            self.topping_modules = []
            for module_name, module in self.get_target_modules():
                self.topping_modules.append((module_name, self.set_topping_module(module_name, module)))
            return
        self.origin_target_modules = set()
        for c in self.configs.values():
            self.origin_target_modules |= set(c.hf_config["target_modules"])
        for m in self.origin_target_modules:
            if m in ("lm_head", "embed_tokens", "logits_processor"):
                raise NotImplementedError(f"toppings on {m} (embedding / LM-head swaps) are out of scope")
        self.target_modules = {get_module_name(m) for m in self.origin_target_modules}
        self.target_weights = {get_stacked_name(m) for m in self.origin_target_modules}
        for name in self.available_toppings:
            self.lora_id[name] = self.toppings_id[name] = len(self.loras)
            self.loras.append(self._adapters[name])
        self.max_lora_dim = max(a.r for a in self.loras)
        self.scaling = self.loras[0].scaling
        if any(a.r != self.max_lora_dim for a in self.loras):
            raise ValueError("all registered LoRA adapters must share r")
        if any(a.scaling != self.scaling for a in self.loras):
            raise ValueError("all registered LoRA adapters must share lora_alpha / r")
        if self.max_lora_dim not in _native.LORA_RANKS:
            raise NotImplementedError(f"LoRA rank {self.max_lora_dim}: the kernels serve r in {_native.LORA_RANKS}")
        self.topping_modules = []
        for module_name, module in self.get_target_modules():
            self.topping_modules.append((module_name, self.set_topping_module(module_name, module)))

    def init_topping_mem_pool(self, args) -> None:
        self.topping_memory_pool = ToppingMemPool(
            args, base_hf_config=self.base_hf_config, loras=self.loras, target_weights=self.target_weights,
            max_toppings_per_batch=self.max_toppings_per_batch, max_lora_dim=self.max_lora_dim,
            base_model=self.base_model, lora_dtype=self.dtype, device=self.device, deltas=self.deltas,
            delta_target_weights=self.target_modules if self.kind == "delta" else None)

    def set_topping_module(self, module_name: str, module: nn.Module) -> BaseLayerWithTopping:
        return replace_submodule(self.base_model, module_name, get_topping_layer(module))

    def match_target_modules(self, module_name: str) -> bool:
        return module_name.split(".")[-1] in self.target_modules

    def get_target_modules(self):
        return [(n, m) for n, m in self.base_model.named_modules()
                if self.match_target_modules(n) and not isinstance(m, BaseLayerWithTopping)
                and ".base_layer" not in n]

    def get_weight_name(self, name: str, idx: int) -> Optional[str]:
        # longest first: "qkv_proj" before "q_proj", "kv_proj" before "v_proj"-like substrings
        for target in sorted(self.target_weights, key=lambda t: -len(t[idx])):
            if "." + target[idx] + "." in name or name.endswith(target[idx]):
                return target[idx]
        return None

    def _wire_modules(self) -> None:
        """hand every topping layer its buffers and THE index tensor, once: nothing a layer holds changes afterwards"""
        if self.kind == "delta":
            groups = (self.slot_offsets, self.sorted_rows)
            for module_name, module in self.topping_modules:
                buf = self.topping_memory_pool.delta_buffer(module_name.split(".")[-1], get_layer_id(module_name))
                key = "delta_buffer_q" if "qkv_proj" in module_name else "delta_buffer"
                module.set_topping_info(0, self.weight_indices, **{key: buf}, delta_groups=groups)
            return
        A, B = self.A_buffer, self.B_buffer
        for module_name, module in self.topping_modules:
            layer_id = get_layer_id(module_name)
            if "qkv_proj" in module_name:
                module.set_topping_info(
                    0, self.weight_indices,
                    lora_buffer=(A["qkv_proj"][layer_id] if "qkv_proj" in A else None,
                                 B["q_proj"][layer_id] if "q_proj" in B else None,
                                 B["kv_proj"][layer_id] if "kv_proj" in B else None), scaling=self.scaling)
            else:
                w = module_name.split(".")[-1]
                module.set_topping_info(
                    0, self.weight_indices,
                    lora_buffer=(A[w][layer_id] if w in A else None, B[w][layer_id] if w in B else None),
                    scaling=self.scaling)

    # ---- per batch
    def assign_slots(self, topping_paths) -> None:
        """the reference's eviction walk (toppings_manager.py:243-261) over the batch's adapters, in first-use order"""
        cur_uids = list(dict.fromkeys(u for u in topping_paths if u is not None))
        for u in cur_uids:
            if u not in self.available_toppings:
                raise KeyError(f"topping {u!r} is not registered")
        if len(cur_uids) > self.max_toppings_per_batch:
            raise ValueError(f"Got {len(cur_uids)} toppings, but max is {self.max_toppings_per_batch}")
        i, j = 0, len(self.active_uids)
        evictable = sorted(self.active_uids, key=lambda u: self.buffer_id[u])
        for uid in cur_uids:
            if uid in self.active_uids:
                continue
            if j < self.max_toppings_per_batch:
                index = j
                j += 1
            else:
                while i < len(evictable) and evictable[i] in cur_uids:
                    i += 1
                assert i < len(evictable)
                self.active_uids.remove(evictable[i])
                index = self.buffer_id.pop(evictable[i])
                i += 1
            self.load_topping(uid, index)
            self.active_uids.add(uid)
            self.buffer_id[uid] = index

    def prepare_topping_batch(self, forward_batch) -> Optional[torch.Tensor]:
        """Slots for the batch's adapters, then the per-token int32 slot vector written into the persistent buffer
        (the one every layer, eager or captured, holds).  Decode: one entry per request.
        Extend: a request's slot repeated ``extend_seq_lens[i]`` times.  ``None`` -> -1.  Returns the filled view."""
        if not self.enabled:
            return None
        paths = forward_batch.topping_paths
        if paths is None:
            paths = [None] * forward_batch.batch_size
        if len(paths) != forward_batch.batch_size:
            raise ValueError(f"Expected batch size to match topping paths, got (bs={forward_batch.batch_size}) != "
                             f"({len(paths)})")
        self.assign_slots(paths)
        slots = [-1 if p is None else self.buffer_id[p] for p in paths]
        if forward_batch.forward_mode.is_extend():
            lens = forward_batch.extend_seq_lens_cpu
            if lens is None:
                lens = [int(v) for v in forward_batch.extend_seq_lens.tolist()]
            slots = [s for s, n in zip(slots, lens) for _ in range(int(n))]
        buf = self.weight_indices
        if len(slots) > buf.shape[0]:
            raise ValueError(f"{len(slots)} tokens exceed the topping index buffer ({buf.shape[0]} entries: "
                             "ServerArgs.max_prefill_tokens)")
        view = buf[: len(slots)]
        if slots:
            view.copy_(torch.tensor(slots, dtype=torch.int32), non_blocking=True)
        return view

    def group_topping_batch(self, num_tokens: int) -> None:
        """delta adapters: the first ``num_tokens`` rows of the index buffer grouped by slot, on the device (one
        launch, no host read: capturable).  Nothing to do for LoRA adapters, whose kernels read the index vector."""
        if self.enabled and self.kind == "delta":
            _native.delta_group(self.weight_indices, int(num_tokens), self.max_toppings_per_batch, self.slot_offsets,
                                self.sorted_rows)

    # ---- slots
    def load_topping(self, uid, buffer_id: int) -> None:
        if uid is not None and uid not in self.available_toppings:
            raise KeyError(f"topping {uid!r} is not registered")
        if self.kind == "delta":
            self._load_delta(uid, buffer_id)
        else:
            self._load_lora(uid, buffer_id)

    def _delta_pools(self):
        pool = self.topping_memory_pool
        return (("codes", pool.qweight_all), ("meta", pool.meta_all), ("scales", pool.scales_all))

    def _stage_delta(self, uid) -> Dict[Tuple[str, str], torch.Tensor]:
        """adapter ``uid`` as the pool stores it: per module and buffer ONE contiguous [layers, N, .] host tensor
        (pinned where the pool is on a device); a module or layer the adapter carries nothing for is an empty delta"""
        if uid in self._staged:
            return self._staged[uid]
        staged = {}
        fill = {"codes": ZERO_CODE, "meta": ZERO_META, "scales": 1}
        for kind, all_ in self._delta_pools():
            for module, big in all_.items():
                t = torch.full((big.shape[0],) + tuple(big.shape[2:]), fill[kind], dtype=big.dtype)
                staged[(kind, module)] = t.pin_memory() if big.is_cuda else t
        for i, layer in enumerate(self.deltas[self.delta_id[uid]].layers):
            for name, w in layer.weights.items():
                module, kind = name.split(".")[-2:]
                dst = staged[(kind, module)][i]
                if tuple(w.shape) != tuple(dst.shape):
                    raise ValueError(f"layer {i} {name}: {tuple(w.shape)} does not fit the slot {tuple(dst.shape)}")
                if w.dtype != dst.dtype:      # (a scale converted to another dtype is another delta)
                    raise ValueError(f"layer {i} {name}: {w.dtype}, the pool holds {dst.dtype}")
                dst.copy_(w)
        self._staged[uid] = staged
        return staged

    def _load_delta(self, uid, buffer_id: int) -> None:
        """adapter ``uid`` into slot ``buffer_id`` of every layer: one copy per module and buffer from the staged host
        tensors; ``uid`` None leaves the slot empty (code 8, scale 1: it adds exactly 0).  In place: a captured graph
        sees the new contents at its next replay."""
        if not 0 <= buffer_id < self.max_toppings_per_batch:
            raise IndexError(f"slot {buffer_id} outside [0, {self.max_toppings_per_batch})")
        staged = None if uid is None else self._stage_delta(uid)
        fill = {"codes": ZERO_CODE, "meta": ZERO_META, "scales": 1}
        for kind, all_ in self._delta_pools():
            for module, big in all_.items():
                if staged is None:
                    big[:, buffer_id].fill_(fill[kind])
                else:
                    big[:, buffer_id].copy_(staged[(kind, module)], non_blocking=True)

    def _stage(self, uid) -> Dict[Tuple[int, str], torch.Tensor]:
        """adapter ``uid`` as the pool stores it: per module ONE contiguous [layers, in, r c] (A) / [layers, r, out c]
        (B) host tensor in the pool's dtype (pinned where the pool is on a device), transposed once
        (toppings_manager.py:456, 460: ``copy_(weights.T)``); a module the adapter does not target is zeros"""
        if uid in self._staged:
            return self._staged[uid]
        pool = self.topping_memory_pool
        staged = {}
        for side, all_ in ((0, pool.A_all), (1, pool.B_all)):
            for module, big in all_.items():
                t = torch.zeros((big.shape[0],) + tuple(big.shape[2:]), dtype=big.dtype)
                staged[(side, module)] = t.pin_memory() if big.is_cuda else t
        for i, layer in enumerate(self.loras[self.lora_id[uid]].layers):
            for name, w in layer.weights.items():
                side = 0 if "lora_A" in name else 1
                target = self.get_weight_name(name, side)
                if target is None:
                    continue
                dst = staged[(side, target)][i]
                if tuple(w.T.shape) != tuple(dst.shape):
                    raise ValueError(f"{name}: {tuple(w.T.shape)} does not fit the slot {tuple(dst.shape)}")
                dst.copy_(w.T)
        self._staged[uid] = staged
        return staged

    def _load_lora(self, uid, buffer_id: int) -> None:
        """adapter ``uid`` into slot ``buffer_id`` of every layer: one copy per module from the staged host tensors;
        ``uid`` None, and every module the adapter does not target, leaves the slot zero.  In place: a captured graph
        sees the new contents at its next replay."""
        if not 0 <= buffer_id < self.max_toppings_per_batch:
            raise IndexError(f"slot {buffer_id} outside [0, {self.max_toppings_per_batch})")
        pool = self.topping_memory_pool
        staged = None if uid is None else self._stage(uid)
        for side, all_ in ((0, pool.A_all), (1, pool.B_all)):
            for module, big in all_.items():
                if staged is None:
                    big[:, buffer_id].zero_()
                else:
                    big[:, buffer_id].copy_(staged[(side, module)], non_blocking=True)

    @property
    def toppings(self):
        return list(self.available_toppings.keys())

    @property
    def A_buffer(self):
        return self.topping_memory_pool.A_buffer

    @property
    def B_buffer(self):
        return self.topping_memory_pool.B_buffer
