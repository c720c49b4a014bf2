"""Host side of the LoRA toppings (no launch): header / SIGNATURES / exports, the refusals of sp_lora_shrink and
sp_lora_expand through the header binding (every call below carries an argument that is refused BEFORE a launch), the
adapter's weight stacking, the pool's shapes, slot assignment and the per-token index vector on CPU tensors."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

from tests import c_header

STATUS = c_header.enum_values("sp_status")
OK, INVALID, UNSUPPORTED = STATUS["SP_OK"], STATUS["SP_ERR_INVALID_ARG"], STATUS["SP_ERR_UNSUPPORTED"]
DT = c_header.enum_values("sp_dtype")


# --------------------------------------------------------------------------- header and host-side refusals
def test_header_declares_both_entries():
    from scratchpad_amd import _native
    protos = c_header.prototypes()
    assert c_header.abi_version() == 10
    assert [n for n, _ in protos["sp_lora_shrink"][1]] == [
        "tmp", "x", "a", "indices", "num_tokens", "K", "R", "num_slots", "x_stride", "a_slot_stride", "tmp_stride",
        "scale", "dtype", "stream"]
    assert [n for n, _ in protos["sp_lora_expand"][1]] == [
        "y", "tmp", "b", "indices", "num_tokens", "r", "n", "num_slices", "num_slots", "y_stride", "tmp_stride",
        "b_slot_stride", "dtype", "stream"]
    for name in ("sp_lora_shrink", "sp_lora_expand"):
        res, args = protos[name]
        assert _native.SIGNATURES[name] == (res, [t for _, t in args])
    assert set(_native.LORA_CALLS) == {"shrink", "expand"}


@pytest.fixture(scope="module")
def lib():
    from scratchpad_amd import _native, build
    build.build_native(verbose=False)
    return c_header.bind(_native.lib_path())


@pytest.fixture(scope="module")
def addr():
    """a 16-byte-aligned HOST address: no call below reaches a launch"""
    buf = (ctypes.c_char * 4096)()
    a = ctypes.addressof(buf)
    yield a + (-a) % 16
    del buf


def test_both_entries_are_exported(lib):
    assert lib.sp_lora_shrink is not None and lib.sp_lora_expand is not None


def test_shrink_refuses_on_the_host(lib, addr):
    a = addr
    good = dict(tmp=a, x=a, a=a, indices=a, num_tokens=5, K=128, R=48, num_slots=3, x_stride=136,
                a_slot_stride=128 * 48, tmp_stride=52, scale=2.0, dtype=DT["SP_BF16"], stream=None)
    assert set(good) == {p for p, _ in lib.sp_prototypes["sp_lora_shrink"][1]}
    call = lambda **kw: c_header.call(lib, "sp_lora_shrink", **{**good, **kw})
    for p in ("tmp", "x", "a", "indices"):
        assert call(**{p: None}) == INVALID, p
    assert call(num_tokens=-5) == INVALID and call(K=-128) == INVALID and call(R=-48) == INVALID
    assert call(R=256) == UNSUPPORTED and call(R=200) == UNSUPPORTED and call(R=12) == UNSUPPORTED
    assert call(K=100) == UNSUPPORTED
    assert call(dtype=DT["SP_F32"]) == UNSUPPORTED and call(dtype=DT["SP_FP8_E5M2"]) == UNSUPPORTED
    assert call(x_stride=120) == INVALID and call(tmp_stride=40) == INVALID and call(a_slot_stride=128 * 48 - 8) == INVALID
    assert call(x_stride=137) == INVALID, "16-byte vectors of x: the row stride is a multiple of 8"
    assert call(x=a + 2) == INVALID and call(a=a + 8) == INVALID, "16-byte vectors need aligned bases"
    assert call(num_tokens=0) == OK and call(num_tokens=0, x=None) == OK


def test_expand_refuses_on_the_host(lib, addr):
    a = addr
    good = dict(y=a, tmp=a, b=a, indices=a, num_tokens=5, r=16, n=64, num_slices=2, num_slots=3, y_stride=136,
                tmp_stride=36, b_slot_stride=16 * 128, dtype=DT["SP_F16"], stream=None)
    assert set(good) == {p for p, _ in lib.sp_prototypes["sp_lora_expand"][1]}
    call = lambda **kw: c_header.call(lib, "sp_lora_expand", **{**good, **kw})
    for p in ("y", "tmp", "b", "indices"):
        assert call(**{p: None}) == INVALID, p
    assert call(num_tokens=-5) == INVALID and call(n=-64) == INVALID and call(r=-16) == INVALID
    assert call(r=12) == UNSUPPORTED and call(r=128) == UNSUPPORTED and call(r=4) == UNSUPPORTED
    assert call(r=64, num_slices=4) == UNSUPPORTED, "R = num_slices * r above 192"
    assert call(n=60) == UNSUPPORTED
    assert call(dtype=DT["SP_F32"]) == UNSUPPORTED
    assert call(y_stride=120) == INVALID and call(tmp_stride=24) == INVALID and call(b_slot_stride=16 * 128 - 8) == INVALID
    assert call(y=a + 2) == INVALID and call(b=a + 4) == INVALID and call(y_stride=137) == INVALID
    assert call(num_tokens=0) == OK and call(num_tokens=0, y=None) == OK


def test_native_wrappers_refuse_host_tensors_and_bad_layouts():
    from scratchpad_amd import _native
    x, A, B = torch.zeros(2, 64, dtype=torch.bfloat16), torch.zeros(3, 64, 16, dtype=torch.bfloat16), \
        torch.zeros(3, 16, 32, dtype=torch.bfloat16)
    idx = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _native.lora_shrink(x, A, idx, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _native.lora_expand(torch.zeros(2, 32, dtype=torch.bfloat16), torch.zeros(2, 16), B, idx, 1)


# --------------------------------------------------------------------------- adapter, pool, manager
@pytest.fixture()
def tp1():
    from scratchpad_amd import distributed as dist_
    if not dist_.model_parallel_is_initialized():
        dist_.initialize_model_parallel(1)
    return dist_


def tiny_config():
    from scratchpad_amd.model_runner import ModelConfig
    return ModelConfig(64, 96, 2, 4, 2, 32)          # hidden 64, inter 96, 2 layers, 4 q heads, 2 kv heads, D 16


ALL = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")


def peft_state(cfg, r, targets, fill):
    """PEFT names; every tensor is filled with a constant that says which projection (and layer, and side) it is"""
    D = cfg.head_dim
    dims = {"q_proj": (cfg.hidden_size, cfg.num_attention_heads * D), "k_proj": (cfg.hidden_size, cfg.num_key_value_heads * D),
            "v_proj": (cfg.hidden_size, cfg.num_key_value_heads * D), "o_proj": (cfg.num_attention_heads * D, cfg.hidden_size),
            "gate_proj": (cfg.hidden_size, cfg.intermediate_size), "up_proj": (cfg.hidden_size, cfg.intermediate_size),
            "down_proj": (cfg.intermediate_size, cfg.hidden_size)}
    sd = {}
    for layer in range(cfg.num_hidden_layers):
        for t in targets:
            block = "self_attn" if t in ("q_proj", "k_proj", "v_proj", "o_proj") else "mlp"
            base = f"base_model.model.model.layers.{layer}.{block}.{t}"
            k = fill + 10 * layer + ALL.index(t)
            sd[base + ".lora_A.weight"] = torch.full((r, dims[t][0]), float(k))
            sd[base + ".lora_B.weight"] = torch.full((dims[t][1], r), float(-k))
    return sd


def make_adapter(uid, cfg, targets=ALL, r=8, alpha=16, fill=1):
    from scratchpad_amd.toppings import LoRAAdapter, ToppingConfig
    conf = ToppingConfig("lora", uid, {"r": r, "lora_alpha": alpha, "target_modules": list(targets)})
    return LoRAAdapter(uid, conf, cfg).initialize_weights(peft_state(cfg, r, targets, fill))


def test_lora_adapter_stacks_like_the_reference():
    cfg = tiny_config()
    ad = make_adapter("a", cfg)
    assert ad.scaling == 2.0 and ad.get_stacked_multiply("qkv_proj") == 3 and ad.get_stacked_multiply("kv_proj") == 2 \
        and ad.get_stacked_multiply("gate_up_proj") == 2 and ad.get_stacked_multiply("o_proj") == 1
    for layer in range(2):
        w = {n.split(f"layers.{layer}.")[1]: t for n, t in ad.layers[layer].weights.items()}
        assert sorted(w) == sorted([
            "self_attn.qkv_proj.lora_A.weight", "self_attn.q_proj.lora_B.weight", "self_attn.kv_proj.lora_B.weight",
            "self_attn.o_proj.lora_A.weight", "self_attn.o_proj.lora_B.weight",
            "mlp.gate_up_proj.lora_A.weight", "mlp.gate_up_proj.lora_B.weight",
            "mlp.down_proj.lora_A.weight", "mlp.down_proj.lora_B.weight"])
        k = 1 + 10 * layer
        qkv = w["self_attn.qkv_proj.lora_A.weight"]
        assert qkv.shape == (24, 64)
        assert qkv[:8].eq(k + 0).all() and qkv[8:16].eq(k + 1).all() and qkv[16:].eq(k + 2).all(), "q | k | v on dim 0"
        kv = w["self_attn.kv_proj.lora_B.weight"]
        assert kv.shape == (64, 8) and kv[:32].eq(-(k + 1)).all() and kv[32:].eq(-(k + 2)).all(), "k | v"
        assert w["self_attn.q_proj.lora_B.weight"].shape == (64, 8) and w["self_attn.q_proj.lora_B.weight"].eq(-k).all()
        gu_a, gu_b = w["mlp.gate_up_proj.lora_A.weight"], w["mlp.gate_up_proj.lora_B.weight"]
        assert gu_a.shape == (16, 64) and gu_a[:8].eq(k + 4).all() and gu_a[8:].eq(k + 5).all(), "gate | up"
        assert gu_b.shape == (192, 8) and gu_b[:96].eq(-(k + 4)).all() and gu_b[96:].eq(-(k + 5)).all()
        assert w["mlp.down_proj.lora_A.weight"].shape == (8, 96) and w["mlp.down_proj.lora_B.weight"].shape == (64, 8)


def test_missing_projection_of_a_stacked_group_is_zero():
    cfg = tiny_config()
    ad = make_adapter("qv", cfg, targets=("q_proj", "v_proj"))
    w = {n.split("layers.0.")[1]: t for n, t in ad.layers[0].weights.items()}
    qkv = w["self_attn.qkv_proj.lora_A.weight"]
    assert qkv.shape == (24, 64) and qkv[:8].eq(1).all() and qkv[8:16].eq(0).all() and qkv[16:].eq(3).all()
    kv = w["self_attn.kv_proj.lora_B.weight"]
    assert kv.shape == (64, 8) and kv[:32].eq(0).all() and kv[32:].eq(-3).all()
    with pytest.raises(NotImplementedError, match="state dict"):
        make_adapter("x", cfg).initialize_weights(None)


def tiny_model(cfg):
    from scratchpad_amd.llama import LlamaForCausalLM
    m = LlamaForCausalLM(cfg, dtype=torch.bfloat16)
    for p in m.parameters():
        p.data.zero_()
    return m


def make_manager(cfg, adapters, slots=2, **kw):
    from scratchpad_amd.toppings import ToppingsManager
    args = SimpleNamespace(max_toppings_per_batch=slots, max_prefill_tokens=64)
    return ToppingsManager(args, tiny_model(cfg), cfg, None, adapters=adapters, device="cpu", dtype=torch.bfloat16, **kw)


def test_pool_shapes_are_the_references_and_layers_are_wrapped(tp1):
    from scratchpad_amd import toppings as tpg
    cfg = tiny_config()
    tm = make_manager(cfg, [make_adapter("a", cfg), make_adapter("b", cfg, fill=3)], slots=2)
    assert tm.enabled and tm.scaling == 2.0 and tm.max_lora_dim == 8
    A, B = tm.A_buffer, tm.B_buffer
    assert sorted(A) == ["down_proj", "gate_up_proj", "o_proj", "qkv_proj"]
    assert sorted(B) == ["down_proj", "gate_up_proj", "kv_proj", "o_proj", "q_proj"]
    # topping_pool.py:88-124: A [slots, in, r * c], B [slots, r, out * c], one tensor per layer
    want_a = {"qkv_proj": (2, 64, 24), "o_proj": (2, 64, 8), "gate_up_proj": (2, 64, 16), "down_proj": (2, 96, 8)}
    want_b = {"q_proj": (2, 8, 64), "kv_proj": (2, 8, 64), "o_proj": (2, 8, 64), "gate_up_proj": (2, 8, 192),
              "down_proj": (2, 8, 64)}
    for k, shp in want_a.items():
        assert len(A[k]) == 2 and all(tuple(t.shape) == shp and t.dtype == torch.bfloat16 for t in A[k]), k
    for k, shp in want_b.items():
        assert len(B[k]) == 2 and all(tuple(t.shape) == shp and t.dtype == torch.bfloat16 for t in B[k]), k
    layer = tm.base_model.model.layers[1]
    assert isinstance(layer.self_attn.qkv_proj, tpg.QKVParallelLinearWithToppings)
    assert isinstance(layer.self_attn.o_proj, tpg.RowParallelLinearWithTopping)
    assert isinstance(layer.mlp.gate_up_proj, tpg.MergedColumnParallelLinearWithTopping)
    assert isinstance(layer.mlp.down_proj, tpg.RowParallelLinearWithTopping)
    assert layer.mlp.gate_up_proj.has_toppings, "LlamaMLP must not take the fused gate_up + SiLU launch"
    assert layer.mlp.gate_up_proj.weight is layer.mlp.gate_up_proj.base_layer.weight
    # the layers hold THE persistent index tensor and their layer's buffers
    assert layer.self_attn.qkv_proj.weight_indices is tm.weight_indices and tm.weight_indices.dtype == torch.int32
    assert layer.self_attn.qkv_proj.A_buffer_qkv is A["qkv_proj"][1] and layer.self_attn.qkv_proj.B_buffer_kv is B["kv_proj"][1]
    assert layer.mlp.down_proj.A_buffer is A["down_proj"][1] and layer.mlp.down_proj.scaling == 2.0
    with pytest.raises(NotImplementedError, match="delta"):
        layer.mlp.down_proj.set_topping_info(1, tm.weight_indices, lora_buffer=None, delta_buffer=(None, None, None))
    with pytest.raises(NotImplementedError, match="delta"):
        layer.self_attn.qkv_proj.set_topping_info(1, tm.weight_indices, lora_buffer=None, delta_buffer_q=())
    # load: copy_(weights.T) into the slot; uid None zeroes it
    tm.load_topping("b", 1)
    assert A["qkv_proj"][1][1][:, :8].eq(13).all() and A["qkv_proj"][1][1][:, 16:].eq(15).all()
    assert B["kv_proj"][0][1][:, :32].eq(-4).all() and B["kv_proj"][0][1][:, 32:].eq(-5).all()
    assert A["qkv_proj"][1][0].eq(0).all(), "slot 0 was not touched"
    tm.load_topping(None, 1)
    assert all(t[1].eq(0).all() for ts in list(A.values()) + list(B.values()) for t in ts)


def fb(mode, paths, extend_lens=None):
    from scratchpad_amd.forward_info import ForwardBatch, ForwardMode
    n = len(paths)
    z = torch.zeros(n, dtype=torch.int64)
    b = ForwardBatch(forward_mode=getattr(ForwardMode, mode), batch_size=n, input_ids=z, req_pool_indices=z, seq_lens=z,
                     out_cache_loc=z, seq_lens_sum=0, topping_paths=paths)
    if extend_lens is not None:
        b.extend_seq_lens_cpu = extend_lens
        b.extend_seq_lens = torch.tensor(extend_lens, dtype=torch.int32)
    return b


def test_prepare_topping_batch_slots_eviction_and_indices(tp1):
    cfg = tiny_config()
    ads = [make_adapter(u, cfg, fill=i + 1) for i, u in enumerate("abcd")]
    tm = make_manager(cfg, ads, slots=2)
    buf = tm.weight_indices
    v = tm.prepare_topping_batch(fb("DECODE", ["a", None, "b", "a"]))
    assert v.data_ptr() == buf.data_ptr() and v.dtype == torch.int32, "written into the persistent buffer"
    assert v.tolist() == [0, -1, 1, 0] and tm.buffer_id == {"a": 0, "b": 1}
    assert tm.A_buffer["o_proj"][0][0].eq(1 + 3).all() and tm.A_buffer["o_proj"][0][1].eq(2 + 3).all()
    # nothing new: nothing moves
    assert tm.prepare_topping_batch(fb("DECODE", ["b", "b"])).tolist() == [1, 1] and tm.buffer_id == {"a": 0, "b": 1}
    # c arrives, the pool is full: the walk evicts the first resident adapter the batch does not name (a, slot 0)
    assert tm.prepare_topping_batch(fb("DECODE", ["c", "b", None])).tolist() == [0, 1, -1]
    assert tm.buffer_id == {"c": 0, "b": 1} and tm.A_buffer["o_proj"][0][0].eq(3 + 3).all()
    # a and d arrive together: both residents go, in slot order
    assert tm.prepare_topping_batch(fb("DECODE", ["a", "d"])).tolist() == [0, 1]
    assert tm.buffer_id == {"a": 0, "d": 1} and tm.A_buffer["o_proj"][0][1].eq(4 + 3).all()
    # a stays where it is, b takes the slot of d
    assert tm.prepare_topping_batch(fb("DECODE", ["b", "a"])).tolist() == [1, 0]
    # all base model: every row -1, nothing loaded or evicted
    assert tm.prepare_topping_batch(fb("DECODE", [None, None, None])).tolist() == [-1, -1, -1]
    assert tm.buffer_id == {"a": 0, "b": 1}
    # extend: a request's slot is repeated extend_seq_lens[i] times; several requests and adapters, unsorted
    v = tm.prepare_topping_batch(fb("EXTEND", ["b", None, "a"], [3, 2, 1]))
    assert v.tolist() == [1, 1, 1, -1, -1, 0] and v.data_ptr() == buf.data_ptr()
    with pytest.raises(ValueError, match="max is 2"):
        tm.prepare_topping_batch(fb("DECODE", ["a", "b", "c"]))
    with pytest.raises(KeyError, match="not registered"):
        tm.prepare_topping_batch(fb("DECODE", ["zzz"]))


def test_refusals_delta_tp_rank_and_disabled(tp1):
    from scratchpad_amd.toppings import ToppingsManager
    cfg = tiny_config()
    a = make_adapter("a", cfg)
    tm = make_manager(cfg, [a])
    with pytest.raises(NotImplementedError, match="delta"):
        tm.register_topping("delta", "some/path", "d")
    with pytest.raises(NotImplementedError, match="TP > 1"):
        make_manager(cfg, [a], tp_size=2)
    with pytest.raises(ValueError, match="share"):
        make_manager(cfg, [a, make_adapter("b", cfg, alpha=32)])
    with pytest.raises(NotImplementedError, match="rank"):
        make_manager(cfg, [make_adapter("c", cfg, r=4, alpha=8)])
    with pytest.raises(NotImplementedError, match="out of scope"):
        make_manager(cfg, [_with_targets(make_adapter("f", cfg, targets=("q_proj",)), ["q_proj", "lm_head"])])
    # no adapters, or no slots: disabled, the model is left alone
    model = tiny_model(cfg)
    off = ToppingsManager(SimpleNamespace(max_toppings_per_batch=None), model, cfg, None, adapters=[a])
    assert not off.enabled and off.prepare_topping_batch(fb("DECODE", [None])) is None
    assert type(model.model.layers[0].mlp.gate_up_proj).__name__ == "MergedColumnParallelLinear"
    assert not ToppingsManager(SimpleNamespace(max_toppings_per_batch=4), model, cfg, None, adapters=[]).enabled


def _with_targets(adapter, targets):
    adapter.config.hf_config["target_modules"] = targets
    return adapter


def test_model_runner_refuses_what_is_out_of_scope():
    from scratchpad_amd.model_runner import ModelConfig, ModelRunner, ServerArgs
    assert ServerArgs().max_toppings_per_batch is None
    for cfg, tp in ((ModelConfig.llama3_8b(), 2), (ModelConfig.qwen3_8b(), 1), (ModelConfig.apertus_8b(), 1),
                    (ModelConfig.mllama_11b_text(), 1)):
        mr = ModelRunner.__new__(ModelRunner)
        mr.model_config, mr.tp_size, mr.server_args = cfg, tp, ServerArgs(max_toppings_per_batch=2)
        with pytest.raises(NotImplementedError, match="out of scope"):
            mr.init_toppings([object()])


def test_adapters_and_slots_go_together():
    from scratchpad_amd.model_runner import ModelConfig, ModelRunner, ServerArgs
    cfg = tiny_config()
    with pytest.raises(ValueError, match="go together"):
        ModelRunner(cfg, ServerArgs(), toppings=[make_adapter("a", cfg)])
    with pytest.raises(ValueError, match="go together"):
        ModelRunner(cfg, ServerArgs(max_toppings_per_batch=2))
    assert ServerArgs().max_prefill_tokens == 16384


def test_checkpoints_load_through_the_wrapped_projections(tp1):
    """the usual loaders after the manager has wrapped the projections: same checkpoint names, same parameters"""
    from scratchpad_amd.llama import LlamaForCausalLM
    cfg = tiny_config()
    g = torch.Generator().manual_seed(3)
    plain = LlamaForCausalLM(cfg, dtype=torch.bfloat16)
    full = {n: torch.randn(p.shape, generator=g).to(torch.bfloat16) for n, p in plain.named_parameters()}
    plain.load_full_state_dict(full)
    tm = make_manager(cfg, [make_adapter("a", cfg)])
    wrapped = tm.base_model
    assert "model.layers.0.self_attn.qkv_proj.base_layer.weight" in dict(wrapped.named_parameters())
    wrapped.load_full_state_dict(full)
    for n, p in plain.named_parameters():
        q = wrapped.get_parameter(n if ".mlp." not in n and ".self_attn." not in n else
                                  n.replace(".weight", ".base_layer.weight"))
        assert torch.equal(p.data, q.data), n
    # HF names (q_proj / k_proj / v_proj, gate_proj / up_proj) through load_weights
    hf = []
    for n, w in full.items():
        if "qkv_proj" in n:
            q, k, v = w.split([64, 32, 32], 0)
            hf += [(n.replace("qkv_proj", t), x) for t, x in (("q_proj", q), ("k_proj", k), ("v_proj", v))]
        elif "gate_up_proj" in n:
            a, b = w.split([96, 96], 0)
            hf += [(n.replace("gate_up_proj", "gate_proj"), a), (n.replace("gate_up_proj", "up_proj"), b)]
        else:
            hf.append((n, w))
    for p in wrapped.parameters():
        p.data.zero_()
    wrapped.load_weights(hf)
    assert torch.equal(wrapped.model.layers[1].mlp.gate_up_proj.weight.data, full["model.layers.1.mlp.gate_up_proj.weight"])
    assert torch.equal(wrapped.model.layers[0].self_attn.qkv_proj.weight.data,
                       full["model.layers.0.self_attn.qkv_proj.weight"])


def test_prepare_for_decode_with_an_enabled_manager_keeps_the_order(tp1):
    from scratchpad_amd import pool, sampler, schedule_batch
    cfg = tiny_config()
    tm = make_manager(cfg, [make_adapter("a", cfg), make_adapter("b", cfg, fill=2)])
    r2t = pool.ReqToTokenPool(8, 16, "cpu", False)
    alloc = pool.TokenToKVPoolAllocator(64, torch.float32, "cpu", None)
    Req, ScheduleBatch = schedule_batch.Req, schedule_batch.ScheduleBatch
    reqs = [Req(str(i), "", [1, 2, 3 + i], sampler.SamplingParams(max_new_tokens=8), topping_path=p)
            for i, p in enumerate(["b", None, "a", "b"])]
    b = ScheduleBatch.init_new(reqs, r2t, alloc, None, SimpleNamespace(is_encoder_decoder=False, vocab_size=32),
                               False, None, False)
    b.req_pool_indices = torch.arange(4)
    b.seq_lens = torch.tensor([3, 3, 3, 3])
    b.seq_lens_sum = 12
    b.output_ids = torch.tensor([7, 8, 9, 10])
    b.prepare_for_decode(tm)
    assert b.forward_mode.is_decode() and [r.rid for r in b.reqs] == ["0", "1", "2", "3"]
    assert b.input_ids.tolist() == [7, 8, 9, 10] and b.seq_lens.tolist() == [4, 4, 4, 4]
    assert [r.topping_path for r in b.reqs] == ["b", None, "a", "b"]
