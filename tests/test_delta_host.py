"""Host side of the delta toppings (no launch): the packed format (pack_delta / unpack_delta), the adapter's stacking, the
pool's shapes and empty-slot contents, slot assignment and eviction, the typed DeltaBuffer, and every refusal, on CPU
tensors."""
from types import SimpleNamespace

import pytest
import torch

from tests import delta_oracle

ALL = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")


# --------------------------------------------------------------------------- the format
def dense_cases():
    g = torch.Generator().manual_seed(11)
    D = torch.randn(24, 64, generator=g)
    D[:4] = 0                                              # row 0: all zero, scale 1
    D[1, :8] = torch.tensor([3.0, 0, 0, 0, 0, 0, 0, -2.0])  # groups with one non-zero
    D[2, :4] = torch.tensor([1.5, -1.5, 1.5, 1.5])          # ties: the lower columns win
    D[3, :4] = torch.tensor([4.0, 0.0, 0.01, 0.0])          # a kept value that rounds to code 8
    D[4] *= 1e-3
    return D


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_unpack_of_pack_keeps_the_two_largest_within_half_a_step(dtype):
    from scratchpad_amd.delta import pack_delta, unpack_delta
    D = dense_cases()
    codes, meta, scales = pack_delta(D, dtype)
    N, K = D.shape
    assert codes.dtype == torch.uint8 and tuple(codes.shape) == (N, K // 4)
    assert meta.dtype == torch.uint8 and tuple(meta.shape) == (N, K // 8)
    assert scales.dtype == dtype and tuple(scales.shape) == (N,)
    U = unpack_delta(codes, meta, scales)
    assert U.dtype == torch.float32 and tuple(U.shape) == (N, K)
    g = D.double().view(N, K // 4, 4)
    order = torch.sort(g.abs(), dim=-1, descending=True, stable=True).indices
    keep = torch.zeros_like(g, dtype=torch.bool).scatter_(-1, order[..., :2], True)
    u = U.double().view(N, K // 4, 4)
    assert bool((u[~keep] == 0).all()), "only the two largest of a group survive"
    half = (scales.double() / 2).view(N, 1, 1).expand_as(g)
    assert bool(((u - g).abs()[keep] <= half[keep]).all()), "a kept value is within scale / 2 of the original"
    # the scale: max |kept| / 7 in the dtype, 1 for the all-zero row
    kept_max = (g.abs() * keep).amax(dim=(1, 2))
    assert scales[0] == 1 and torch.equal(scales[1:], (kept_max[1:] / 7).to(dtype))
    # ties go to the lower column; fewer than two non-zeros: code 8 at the unused position
    assert U[2, 0] > 0 > U[2, 1] and U[2, 2] == 0 and U[2, 3] == 0
    assert codes[1, 0] == ((8 << 4) | 15) and meta[1, 0] & 15 == (0 | 1 << 2), "3.0 = 7 scale at column 0, code 8 next"
    assert codes[1, 1] >> 4 != 8 and codes[1, 1] & 15 == 8 and meta[1, 0] >> 4 == (0 | 3 << 2)
    assert codes[0].eq(0x88).all() and meta[0].eq(0x44).all()
    # the independent restatement of the format (the GPU tests' oracle) reads the same matrix
    q = delta_oracle.dense_codes(codes, meta)
    assert torch.equal((q * scales.double().view(N, 1)).float(), U)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_pack_of_unpack_is_the_identity_on_packed_tensors(dtype):
    from scratchpad_amd.delta import empty_delta, pack_delta, unpack_delta
    packed = pack_delta(dense_cases(), dtype)
    again = pack_delta(unpack_delta(*packed), dtype)
    for a, b, what in zip(packed, again, ("codes", "meta", "scales")):
        assert torch.equal(a, b), what
    empty = empty_delta(16, 64, dtype)
    assert all(torch.equal(a, b) for a, b in zip(empty, pack_delta(torch.zeros(16, 64), dtype)))
    assert unpack_delta(*empty).eq(0).all()


def test_format_refusals():
    from scratchpad_amd.delta import pack_delta, unpack_delta
    with pytest.raises(ValueError, match="multiple of 8"):
        pack_delta(torch.zeros(4, 12))
    with pytest.raises(ValueError, match="fp16 or bf16"):
        pack_delta(torch.zeros(4, 16), torch.float32)
    c, m, s = pack_delta(torch.ones(4, 16), torch.float16)
    with pytest.raises(ValueError, match="p0 < p1"):
        unpack_delta(c, torch.zeros_like(m), s)
    with pytest.raises(ValueError, match="one matrix"):
        unpack_delta(c, m[:, :1], s)


# --------------------------------------------------------------------------- adapter, pool, manager
@pytest.fixture()
def tp1():
    from scratchpad_amd import distributed as dist_
    if not dist_.model_parallel_is_initialized():
        dist_.initialize_model_parallel(1)
    return dist_


def tiny_config(inter=128):
    from scratchpad_amd.model_runner import ModelConfig
    return ModelConfig(64, inter, 2, 4, 2, 32)          # hidden 64, 2 layers, 4 q heads, 2 kv heads, D 16


def packed_state(cfg, targets, fill, dtype=torch.bfloat16):
    """every projection's dense delta is 7 k in columns 0 and 1 of every group, k a constant that says which projection
    and layer it is (scale k, code 15: exact in bf16), packed"""
    from scratchpad_amd.delta import pack_delta
    from scratchpad_amd.toppings import delta_proj_shape
    sd, dense = {}, {}
    for layer in range(cfg.num_hidden_layers):
        for t in targets:
            N, K = delta_proj_shape(t, cfg)
            D = torch.zeros(N, K)
            D[:, 0::4] = D[:, 1::4] = 7.0 * (fill + 10 * layer + ALL.index(t))
            block = "self_attn" if t in ALL[:4] else "mlp"
            base = f"model.layers.{layer}.{block}.{t}"
            for k, v in zip(("codes", "meta", "scales"), pack_delta(D, dtype)):
                sd[f"{base}.{k}"] = v
            dense[(layer, t)] = D
    return sd, dense


def make_adapter(uid, cfg, targets=ALL, fill=1, hf_config=None):
    from scratchpad_amd.toppings import DeltaAdapter, ToppingConfig
    conf = ToppingConfig("delta", uid, hf_config or {})
    return DeltaAdapter(uid, conf, cfg).initialize_weights(packed_state(cfg, targets, fill)[0])


def test_delta_adapter_stacks_by_rows():
    from scratchpad_amd.delta import unpack_delta
    cfg = tiny_config()
    ad = make_adapter("a", cfg)
    assert ad.target_modules == {"qkv_proj", "o_proj", "gate_up_proj", "down_proj"}
    assert ad.get_pack_factor() == 8 and ad.get_sparse_factor() == 2
    for layer in range(2):
        w = ad.layers[layer].weights
        assert sorted(w) == sorted(f"{b}.{m}.{k}" for b, m in (("self_attn", "qkv_proj"), ("self_attn", "o_proj"),
                                                               ("mlp", "gate_up_proj"), ("mlp", "down_proj"))
                                   for k in ("codes", "meta", "scales"))
        k = 1 + 10 * layer
        qkv = unpack_delta(*(w[f"self_attn.qkv_proj.{m}"] for m in ("codes", "meta", "scales")))
        assert tuple(qkv.shape) == (128, 64)
        assert qkv[:64, 0].eq(7 * k).all() and qkv[64:96, 0].eq(7 * k + 7).all() and qkv[96:, 0].eq(7 * k + 14).all(), "q | k | v"
        gu = unpack_delta(*(w[f"mlp.gate_up_proj.{m}"] for m in ("codes", "meta", "scales")))
        assert tuple(gu.shape) == (256, 64) and gu[:128, 1].eq(7 * k + 28).all() and gu[128:, 1].eq(7 * k + 35).all(), "gate | up"
        assert tuple(w["mlp.down_proj.codes"].shape) == (64, 32) and tuple(w["mlp.down_proj.meta"].shape) == (64, 16)
        assert tuple(w["self_attn.o_proj.scales"].shape) == (64,)


def test_missing_member_of_a_stacked_group_is_an_empty_delta():
    from scratchpad_amd.delta import unpack_delta
    cfg = tiny_config()
    ad = make_adapter("qv", cfg, targets=("q_proj", "v_proj"))
    assert ad.target_modules == {"qkv_proj"}
    w = ad.layers[0].weights
    assert w["self_attn.qkv_proj.codes"][64:96].eq(0x88).all() and w["self_attn.qkv_proj.meta"][64:96].eq(0x44).all()
    assert w["self_attn.qkv_proj.scales"][64:96].eq(1).all()
    qkv = unpack_delta(*(w[f"self_attn.qkv_proj.{m}"] for m in ("codes", "meta", "scales")))
    assert qkv[:64, 0].eq(7).all() and qkv[64:96].eq(0).all() and qkv[96:, 0].eq(21).all()


def test_delta_adapter_refusals():
    from scratchpad_amd.toppings import DeltaAdapter, ToppingConfig
    cfg = tiny_config()
    with pytest.raises(NotImplementedError, match="state dict"):
        DeltaAdapter("x", ToppingConfig("delta", "x"), cfg).initialize_weights(None)
    sd, _ = packed_state(cfg, ("q_proj",), 1)
    for name in ("model.embed_tokens.codes", "lm_head.codes", "model.norm.weight",
                 "model.layers.0.input_layernorm.weight", "model.layers.0.self_attn.rotary.codes"):
        with pytest.raises(NotImplementedError, match="out of scope") as e:
            DeltaAdapter("x", ToppingConfig("delta", "x"), cfg).initialize_weights({**sd, name: torch.zeros(4)})
        assert name in str(e.value)
    with pytest.raises(NotImplementedError, match="qweight"):
        DeltaAdapter("x", ToppingConfig("delta", "x"), cfg).initialize_weights(
            {"model.layers.0.self_attn.q_proj.qweight": torch.zeros(4)})
    for cc in ({"bits": 2, "sparsity": 0.5}, {"bits": 4, "sparsity": 1.0}, {"bits": 4, "sparsity": 0.25}):
        with pytest.raises(NotImplementedError, match="compress_config"):
            DeltaAdapter("x", ToppingConfig("delta", "x", {"compress_config": cc}), cfg)
    DeltaAdapter("x", ToppingConfig("delta", "x", {"compress_config": {"bits": 4, "sparsity": 0.5}}), cfg)
    bad = dict(sd)
    bad["model.layers.0.self_attn.q_proj.codes"] = bad["model.layers.0.self_attn.q_proj.codes"][:, :8]
    with pytest.raises(ValueError, match="expected"):
        DeltaAdapter("x", ToppingConfig("delta", "x"), cfg).initialize_weights(bad)
    del bad["model.layers.0.self_attn.q_proj.codes"]
    with pytest.raises(ValueError, match="missing"):
        DeltaAdapter("x", ToppingConfig("delta", "x"), cfg).initialize_weights(bad)


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


def test_pool_shapes_empty_slots_and_wiring(tp1):
    from scratchpad_amd import toppings as tpg
    from scratchpad_amd.delta import unpack_delta
    cfg = tiny_config()
    tm = make_manager(cfg, [make_adapter("a", cfg), make_adapter("b", cfg, fill=3)], slots=2)
    assert tm.enabled and tm.kind == "delta" and tm.A_buffer == {} and tm.B_buffer == {}
    pool = tm.topping_memory_pool
    want = {"qkv_proj": (128, 64), "o_proj": (64, 64), "gate_up_proj": (256, 64), "down_proj": (64, 128)}
    assert sorted(pool.qweight_buffer) == sorted(want) == sorted(pool.meta_buffer) == sorted(pool.scales_buffer)
    for m, (N, K) in want.items():
        # ONE [layers, slots, ...] allocation per module and buffer, the layers are views of it
        assert tuple(pool.qweight_all[m].shape) == (2, 2, N, K // 4) and pool.qweight_all[m].dtype == torch.uint8
        assert tuple(pool.meta_all[m].shape) == (2, 2, N, K // 8) and pool.meta_all[m].dtype == torch.uint8
        assert tuple(pool.scales_all[m].shape) == (2, 2, N) and pool.scales_all[m].dtype == torch.bfloat16
        for layer in range(2):
            assert pool.qweight_buffer[m][layer].data_ptr() == pool.qweight_all[m][layer].data_ptr()
            assert tuple(pool.meta_buffer[m][layer].shape) == (2, N, K // 8)
            assert tuple(pool.scales_buffer[m][layer].shape) == (2, N)
        # an empty slot: code 8, scale 1 - the zero matrix
        assert pool.qweight_all[m].eq(0x88).all() and pool.meta_all[m].eq(0x44).all() and pool.scales_all[m].eq(1).all()
        assert unpack_delta(pool.qweight_buffer[m][0][1], pool.meta_buffer[m][0][1], pool.scales_buffer[m][0][1]).eq(0).all()
    layer = tm.base_model.model.layers[1]
    assert isinstance(layer.self_attn.qkv_proj, tpg.QKVParallelLinearWithToppings)
    assert isinstance(layer.self_attn.o_proj, tpg.RowParallelLinearWithTopping)
    assert isinstance(layer.mlp.gate_up_proj, tpg.MergedColumnParallelLinearWithTopping)
    assert isinstance(layer.mlp.down_proj, tpg.RowParallelLinearWithTopping)
    assert layer.mlp.gate_up_proj.has_toppings, "LlamaMLP must not take the fused gate_up + SiLU launch"
    # the layers hold THE persistent index / grouping tensors and their layer's views
    assert tm.slot_offsets.dtype == torch.int32 and tuple(tm.slot_offsets.shape) == (3,)
    assert tm.sorted_rows.dtype == torch.int32 and tm.sorted_rows.shape[0] == tm.weight_indices.shape[0] == 64
    for mod, name in ((layer.self_attn.qkv_proj, "qkv_proj"), (layer.mlp.down_proj, "down_proj")):
        assert isinstance(mod.delta, tpg.DeltaBuffer) and mod.weight_indices is tm.weight_indices
        assert mod.delta.codes is pool.qweight_buffer[name][1] and mod.delta.meta is pool.meta_buffer[name][1]
        assert mod.delta.scales is pool.scales_buffer[name][1]
        assert mod.delta_groups[0] is tm.slot_offsets and mod.delta_groups[1] is tm.sorted_rows
    assert layer.self_attn.qkv_proj.A_buffer_qkv is None and layer.mlp.down_proj.A_buffer is None
    # load: the staged tensors into the slot, every layer and module; uid None empties it
    tm.load_topping("b", 1)
    got = unpack_delta(pool.qweight_buffer["qkv_proj"][1][1], pool.meta_buffer["qkv_proj"][1][1],
                       pool.scales_buffer["qkv_proj"][1][1])
    assert got[:64, 0].eq(91).all() and got[64:96, 1].eq(98).all() and got[96:, 0].eq(105).all() and got[:, 2].eq(0).all()
    got = unpack_delta(pool.qweight_buffer["down_proj"][0][1], pool.meta_buffer["down_proj"][0][1],
                       pool.scales_buffer["down_proj"][0][1])
    assert got[:, 0].eq(7 * (3 + 6)).all()
    assert pool.qweight_all["qkv_proj"][:, 0].eq(0x88).all(), "slot 0 was not touched"
    tm.load_topping(None, 1)
    for m in want:
        assert pool.qweight_all[m].eq(0x88).all() and pool.meta_all[m].eq(0x44).all() and pool.scales_all[m].eq(1).all()
    with pytest.raises(IndexError):
        tm.load_topping("a", 2)
    # scales in another dtype than the pool's are not converted silently
    from scratchpad_amd.toppings import DeltaAdapter, ToppingConfig
    half = DeltaAdapter("h", ToppingConfig("delta", "h"), cfg).initialize_weights(
        packed_state(cfg, ("o_proj",), 1, dtype=torch.float16)[0])
    tm16 = make_manager(cfg, [half])
    with pytest.raises(ValueError, match="the pool holds"):
        tm16.load_topping("h", 0)


def test_a_partial_adapter_leaves_the_other_modules_empty(tp1):
    cfg = tiny_config()
    tm = make_manager(cfg, [make_adapter("o", cfg, targets=("o_proj",)), make_adapter("d", cfg, targets=("down_proj",))])
    pool = tm.topping_memory_pool
    assert sorted(pool.qweight_buffer) == ["down_proj", "o_proj"]
    tm.load_topping("o", 0)
    assert not pool.qweight_all["o_proj"][:, 0].eq(0x88).all() and pool.qweight_all["down_proj"][:, 0].eq(0x88).all()
    assert type(tm.base_model.model.layers[0].self_attn.qkv_proj).__name__ == "QKVParallelLinear"


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


def test_slot_assignment_and_eviction(tp1):
    cfg = tiny_config()
    tm = make_manager(cfg, [make_adapter(u, cfg, targets=("o_proj",), fill=i + 1) for i, u in enumerate("abc")], slots=2)
    codes = tm.topping_memory_pool.qweight_all["o_proj"]
    scales = tm.topping_memory_pool.scales_all["o_proj"]
    v = tm.prepare_topping_batch(fb("DECODE", ["a", None, "b", "a"]))
    assert v.data_ptr() == tm.weight_indices.data_ptr() and v.tolist() == [0, -1, 1, 0]
    assert tm.buffer_id == {"a": 0, "b": 1}
    # the slots' scales (fill + 3) tell the adapters apart
    assert scales[0, 0, 0] == 4 and scales[0, 1, 0] == 5
    before = codes.data_ptr()
    assert tm.prepare_topping_batch(fb("DECODE", ["c", "b", None])).tolist() == [0, 1, -1]
    assert tm.buffer_id == {"c": 0, "b": 1} and scales[0, 0, 0] == 6
    assert codes.data_ptr() == before, "loaded in place: the addresses a captured graph holds stay valid"
    v = tm.prepare_topping_batch(fb("EXTEND", ["b", None, "a"], [3, 2, 1]))
    assert v.tolist() == [1, 1, 1, -1, -1, 0] and tm.buffer_id == {"a": 0, "b": 1}
    with pytest.raises(ValueError, match="max is 2"):
        tm.prepare_topping_batch(fb("DECODE", ["a", "b", "c"]))
    with pytest.raises(KeyError, match="not registered"):
        tm.prepare_topping_batch(fb("DECODE", ["zzz"]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tm.group_topping_batch(4)


def test_manager_and_layer_refusals(tp1):
    from scratchpad_amd import toppings as tpg
    from tests.test_lora_host import make_adapter as make_lora
    cfg = tiny_config()
    a = make_adapter("a", cfg)
    tm = make_manager(cfg, [a])
    # a delta topping nobody handed a DeltaAdapter in for: loading from a path is out of scope
    with pytest.raises(NotImplementedError, match="delta"):
        tm.register_topping("delta", "some/path", "d")
    tm.register_topping("delta", "a", "a")
    with pytest.raises(NotImplementedError, match="one manager"):
        tm.register_topping("lora", "some/path", "l")
    with pytest.raises(NotImplementedError, match="unknown"):
        tm.register_topping("ia3", "some/path", "x")
    with pytest.raises(NotImplementedError, match="one manager"):
        make_manager(cfg, [a, make_lora("l", cfg)])
    with pytest.raises(NotImplementedError, match="TP > 1"):
        make_manager(cfg, [a], tp_size=2)
    with pytest.raises(NotImplementedError, match="out of scope"):
        make_manager(cfg, [make_adapter("h", cfg, hf_config={"target_modules": ["q_proj", "lm_head"]})])
    with pytest.raises(NotImplementedError, match="multiples of 64"):
        make_manager(tiny_config(inter=96), [make_adapter("w", tiny_config(inter=96), targets=("down_proj",))])
    with pytest.raises(NotImplementedError, match="out of scope"):
        tpg.ToppingMemPool(None, cfg, [], set(), 2, 0, deltas=[a], delta_target_weights={"o_proj"}, device="cpu",
                           uncompressed_delta_target_weights={"lm_head"})
    # the layers: a DeltaBuffer or None; a raw tuple is the reference's triteia-layout triple
    layer = tm.base_model.model.layers[0]
    buf = tm.topping_memory_pool.delta_buffer("down_proj", 0)
    groups = (tm.slot_offsets, tm.sorted_rows)
    layer.mlp.down_proj.set_topping_info(1, tm.weight_indices, delta_buffer=buf, delta_groups=groups)
    for raw in ((None, None, None), (), (buf.codes, buf.meta, buf.scales)):
        with pytest.raises(NotImplementedError, match="delta"):
            layer.mlp.down_proj.set_topping_info(1, tm.weight_indices, delta_buffer=raw, delta_groups=groups)
        with pytest.raises(NotImplementedError, match="delta"):
            layer.self_attn.qkv_proj.set_topping_info(1, tm.weight_indices, delta_buffer_q=raw, delta_groups=groups)
    with pytest.raises(NotImplementedError, match="delta_buffer_kv"):
        layer.self_attn.qkv_proj.set_topping_info(1, tm.weight_indices, delta_buffer_kv=buf, delta_groups=groups)
    with pytest.raises(ValueError, match="delta_groups"):
        layer.mlp.down_proj.set_topping_info(1, tm.weight_indices, delta_buffer=buf)
    with pytest.raises(ValueError, match="DeltaBuffer"):
        tpg.DeltaBuffer(buf.codes, buf.meta[:, :, :1], buf.scales)
    # no slots: disabled, the model is left alone
    model = tiny_model(cfg)
    off = tpg.ToppingsManager(SimpleNamespace(max_toppings_per_batch=None), model, cfg, None, adapters=[a])
    assert not off.enabled and off.prepare_topping_batch(fb("DECODE", [None])) is None
    assert type(model.model.layers[0].mlp.gate_up_proj).__name__ == "MergedColumnParallelLinear"


def test_model_runner_refuses_delta_adapters_where_it_refuses_lora():
    from scratchpad_amd.model_runner import ModelConfig, ModelRunner, ServerArgs
    cfg = tiny_config()
    for mc, tp in ((ModelConfig.llama3_8b(), 2), (ModelConfig.qwen3_8b(), 1)):
        mr = ModelRunner.__new__(ModelRunner)
        mr.model_config, mr.tp_size, mr.server_args = mc, tp, ServerArgs(max_toppings_per_batch=2)
        with pytest.raises(NotImplementedError, match="out of scope"):
            mr.init_toppings([make_adapter("a", cfg)])
    with pytest.raises(ValueError, match="go together"):
        ModelRunner(cfg, ServerArgs(), toppings=[make_adapter("a", cfg)])
