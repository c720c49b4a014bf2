"""Host side of Llama-Quant-MoE without a GPU: tests/quant_moe_oracle.py against the package's own unpack and against
itself (it must notice a wrong accumulation order and exchanged experts), ModelConfig's layouts, refusals and preset,
and the module tree, packed-expert storage and checkpoint loaders of scratchpad_amd/llama_quant_moe.py."""
import pytest
import torch

from tests import moe_oracle, quant_moe_oracle as qo

ARCHS = ("llama_quant_moe", "llama_naive_quant_moe")


@pytest.fixture()
def tp1():
    from scratchpad_amd import distributed as dist_
    if not dist_.model_parallel_is_initialized():
        dist_.initialize_model_parallel(1)
    return dist_


# --------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_oracle_unpack_matches_unpack_delta(dtype):
    from scratchpad_amd.delta import pack_delta, unpack_delta
    g = torch.Generator().manual_seed(3)
    packs = [pack_delta(torch.randn(24, 64, generator=g) * 0.1, dtype) for _ in range(3)]
    packed = tuple(torch.stack([p[i] for p in packs]) for i in range(3))
    q, s = qo.unpack(packed)
    for e in range(3):
        assert torch.equal(q[e] * s[e][:, None], unpack_delta(*packs[e]).double())
    codes, meta, scales = qo.random_packed(2, 16, 64, dtype, seed=4)
    q, s = qo.unpack((codes, meta, scales))
    for e in range(2):
        assert torch.equal(q[e] * s[e][:, None], unpack_delta(codes[e], meta[e], scales[e]).double())
    assert int(q.min()) == -8 and int(q.max()) == 7 and float((q == 0).double().mean()) >= 0.5


def small_problem(dtype, T=9, H=64, inter=64, E=4, K=3, seed=5):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, H, generator=g).to(dtype)
    p13, p2 = qo.random_packed(E, 2 * inter, H, dtype, seed + 1), qo.random_packed(E, H, inter, dtype, seed + 2)
    logits = (torch.randn(T, E, generator=g) * 2).to(dtype)
    ids, wts = moe_oracle.route(logits, K)
    base = torch.randn(T, H, generator=g).to(dtype)
    return x, p13, p2, ids, wts, base


def test_oracle_notices_a_wrong_accumulation_order_at_k3():
    dtype = torch.bfloat16
    x, p13, p2, ids, wts, base = small_problem(dtype)
    assert any(r != sorted(r) for r in ids.tolist()), "rank order and expert order differ for some token"
    by_expert, b0 = qo.experts(x, p13, p2, ids, wts, base, qo.ORDER_EXPERT)
    by_rank, b1 = qo.experts(x, p13, p2, ids, wts, base, qo.ORDER_RANK)
    moved = (by_expert - by_rank).abs() > b0 + b1
    assert bool(moved.any()), "the two orders agree everywhere within the bounds: the oracle cannot tell them apart"
    # ... while tokens whose ranks are already ascending in expert index agree exactly
    same = [t for t, r in enumerate(ids.tolist()) if r == sorted(r)]
    assert same and torch.equal(by_expert[same], by_rank[same])
    assert float((b0 > 0).double().mean()) < 0.5, "the bound is zero away from rounding boundaries"


def test_oracle_skips_ids_outside_the_experts_and_counts_duplicates():
    dtype = torch.float16
    tmp = torch.tensor([[1.0], [2.0], [4.0], [8.0], [16.0], [32.0]], dtype=dtype)      # T = 2, K = 3
    base = torch.tensor([[0.5], [0.25]], dtype=dtype)
    ids = torch.tensor([[2, 7, 2], [-1, 0, 0]])
    for order in (qo.ORDER_EXPERT, qo.ORDER_RANK):
        out, bound = qo.combine(tmp, ids, 4, base, order, dtype)
        assert out.flatten().tolist() == [5.5, 48.25] and float(bound.max()) == 0.0
    assert qo.combine_order([3, 1, 3, 0], 4, qo.ORDER_EXPERT) == [3, 1, 0, 2]
    assert qo.combine_order([3, 1, 9, 0], 4, qo.ORDER_RANK) == [0, 1, 3]


def test_model_oracle_is_sensitive_to_exchanged_experts_and_holds_the_gap():
    g, pfx, shape, w0 = moe_oracle.load_case("a")
    assert (shape.hidden, shape.inter, shape.layers, shape.E, shape.K) == (128, 64, 2, 4, 2)
    swapped = qo.swap_experts(qo.quant_weights(w0, shape))
    for arch in ARCHS:
        l1, l2, t1, t2 = qo.oracle_run(arch)
        assert qo.router_gap(t1, shape.K) >= 0.125 and qo.router_gap(t2, shape.K) >= 0.125
        s1 = qo.oracle_run(arch, w=swapped)[0]
        assert float((s1 - l1).abs().max() / l1.abs().max()) > 1e-3
    a, b = qo.oracle_run(ARCHS[0]), qo.oracle_run(ARCHS[1])
    assert float((a[0] - b[0]).abs().max()) <= 1e-5 * float(a[0].abs().max()), "fp32: the variants differ by round-off"


# --------------------------------------------------------------------------- ModelConfig
BASE = (128, 64, 2, 4, 2, 32)


def test_model_config_layouts_refusals_and_preset():
    from scratchpad_amd.model_runner import ModelConfig, ModelRunner, ServerArgs
    for arch in ARCHS:
        with pytest.raises(NotImplementedError, match="quantised MoE"):
            ModelConfig(*BASE, architecture=arch, num_experts=4, experts_per_token=2)
        cfg = ModelConfig(*BASE, architecture=arch, num_experts=4, experts_per_token=2, expert_layout="sp_delta",
                          sbmm_type="multilaunch")
        assert cfg.expert_layout == "sp_delta" and cfg.is_generation
        kw = dict(architecture=arch, expert_layout="sp_delta")
        with pytest.raises(ValueError, match="num_experts"):
            ModelConfig(*BASE, **kw)
        with pytest.raises(NotImplementedError, match="grouped_topk"):
            ModelConfig(*BASE, num_experts=4, experts_per_token=2, grouped_topk=True, **kw)
        with pytest.raises(NotImplementedError, match="64 experts"):
            ModelConfig(*BASE, num_experts=65, experts_per_token=2, **kw)
        with pytest.raises(NotImplementedError, match="top-8"):
            ModelConfig(*BASE, num_experts=16, experts_per_token=9, **kw)
        with pytest.raises(NotImplementedError, match="embedding requests"):
            ModelConfig(*BASE, num_experts=4, experts_per_token=2, is_embedding=True, **kw)
        with pytest.raises(ValueError, match="expert_layout"):
            ModelConfig(*BASE, architecture=arch, num_experts=4, experts_per_token=2, expert_layout="marlin")
    with pytest.raises(ValueError, match="expert_layout"):
        ModelConfig(*BASE, architecture="llama_moe", num_experts=4, experts_per_token=2, expert_layout="sp_delta")
    cfg = ModelConfig.llama3_8b_quant_moe()
    ref = ModelConfig.llama3_8b()
    fields = ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "num_key_value_heads",
              "vocab_size", "head_dim", "rope_theta")
    assert all(getattr(cfg, f) == getattr(ref, f) for f in fields)
    assert (cfg.architecture, cfg.num_experts, cfg.experts_per_token, cfg.expert_layout) == \
        ("llama_quant_moe", 8, 2, "sp_delta")
    assert ModelConfig.llama3_8b_quant_moe(16, 4).num_experts == 16
    assert "SYNTHETIC" in ModelConfig.llama3_8b_quant_moe.__doc__
    # toppings, TP > 1 and fp32 at the model runner
    mr = ModelRunner.__new__(ModelRunner)
    mr.model_config, mr.tp_size, mr.server_args = cfg, 1, ServerArgs(max_toppings_per_batch=2)
    with pytest.raises(NotImplementedError, match="Llama only"):
        mr.init_toppings([object()])
    mr.tp_size, mr.device, mr.dtype = 2, "cpu", torch.bfloat16
    with pytest.raises(NotImplementedError, match="TP > 1"):
        mr.load_model(0, False)
    mr.tp_size, mr.dtype = 1, torch.float32
    with pytest.raises(NotImplementedError, match="fp16 / bf16"):
        mr.load_model(0, False)


def test_layer_refuses_tp_fp32_grouped_topk_and_widths(tp1, monkeypatch):
    from types import SimpleNamespace
    from scratchpad_amd import llama_quant_moe as lq
    cfg = qo.model_config(moe_oracle.load_case("a")[2], ARCHS[0])
    with pytest.raises(NotImplementedError, match="grouped_topk"):
        lq.LlamaDecoderLayer(SimpleNamespace(**{**cfg.__dict__, "grouped_topk": True}), 0, torch.float16)
    with pytest.raises(NotImplementedError, match="fp16 / bf16"):
        lq.LlamaMoE(64, 64, "silu", 4, 2, torch.float32)
    with pytest.raises(NotImplementedError, match="multiples of 64"):
        lq.LlamaMoE(128, 32, "silu", 4, 2, torch.float16)
    with pytest.raises(NotImplementedError, match="num_experts"):
        lq.LlamaMoE(64, 64, "silu", 65, 2, torch.float16)
    with pytest.raises(NotImplementedError, match="experts_per_token"):
        lq.LlamaNaiveMoE(64, 64, "silu", 4, 5, torch.float16)
    monkeypatch.setattr(lq, "get_tensor_model_parallel_world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="TP > 1"):
        lq.LlamaMoE(64, 64, "silu", 4, 2, torch.float16)
    with pytest.raises(NotImplementedError, match="TP > 1"):
        lq.LlamaQuantisedMoEForCausalLM(cfg, torch.float16)


# --------------------------------------------------------------------------- the model
def build(arch, dtype=torch.float16):
    from scratchpad_amd import llama_quant_moe as lq
    shape = moe_oracle.load_case("a")[2]
    cls = lq.LlamaQuantisedMoEForCausalLM if arch == ARCHS[0] else lq.LlamaNaiveQuantisedMoEForCausalLM
    return cls(qo.model_config(shape, arch), dtype), shape


def dense_experts(moe):
    from scratchpad_amd.delta import unpack_delta
    p13, p2 = moe.packed()
    return [torch.stack([unpack_delta(c[e], m[e], s[e]) for e in range(c.shape[0])]) for c, m, s in (p13, p2)]


@pytest.mark.parametrize("arch", ARCHS)
def test_module_tree_names_and_a_fresh_model_adds_zero(tp1, arch):
    model, shape = build(arch)
    names = set(model.state_dict())
    E, H, I = shape.E, shape.hidden, shape.inter
    p = "model.layers.1.moe."
    assert {p + "gate.weight", p + "base_mlp.gate_up_proj.weight", p + "base_mlp.down_proj.weight"} <= names
    mid = [""] if arch == ARCHS[0] else [f"{e}." for e in range(E)]
    lead = (E,) if arch == ARCHS[0] else ()
    sd = model.state_dict()
    for m in mid:
        for proj, (N, K) in (("gate_up_proj", (2 * I, H)), ("down_proj", (H, I))):
            c, me, s = (sd[p + f"mlp.{m}{proj}.{leaf}"] for leaf in ("codes", "meta", "scales"))
            assert tuple(c.shape) == lead + (N, K // 4) and c.dtype == torch.uint8
            assert tuple(me.shape) == lead + (N, K // 8) and me.dtype == torch.uint8
            assert tuple(s.shape) == lead + (N,) and s.dtype == torch.float16
    assert not any("qweight" in n or "workspace" in n for n in names)
    params = dict(model.named_parameters())
    assert not any(n.endswith(("codes", "meta", "scales")) for n in params), "packed experts are buffers"
    assert tuple(params[p + "gate.weight"].shape) == (E, H)
    moe = model.model.layers[0].moe
    assert type(moe.base_mlp).__module__ == "scratchpad_amd.llama"
    assert type(model.model.layers[0]).feed_forward_name == "moe"
    w13, w2 = dense_experts(moe)
    assert float(w13.abs().max()) == 0.0 and float(w2.abs().max()) == 0.0, "a fresh model's experts add exactly 0"
    assert bool((moe.packed()[0][2] == 1).all())


@pytest.mark.parametrize("arch", ARCHS)
def test_init_weights_produces_valid_packed_experts(tp1, arch):
    model, shape = build(arch, torch.bfloat16)
    model.init_expert_weights(torch.Generator().manual_seed(0))
    seen = set()
    for moe in model.moe_blocks():
        for codes, meta, scales in moe.packed():
            for nib in (meta & 15, meta >> 4):
                assert bool(((nib & 3) < (nib >> 2)).all()), "every meta nibble names p0 < p1"
            seen |= set((codes & 15).unique().tolist())
            assert bool((scales > 0).all()) and float(scales.float().max()) < 0.01
        w13, _ = dense_experts(moe)                  # unpack_delta checks the meta once more
        assert float(w13.abs().max()) > 0
    assert seen == set(range(16))
    a = model.model.layers[0].moe.packed()[0][0].clone()
    model.init_expert_weights(torch.Generator().manual_seed(0))
    assert torch.equal(a, model.model.layers[0].moe.packed()[0][0]), "seeded"
    if arch == ARCHS[1]:        # the per-expert buffers are views of the stacked storage
        moe = model.model.layers[0].moe
        assert moe.mlp[2].down_proj.codes.data_ptr() == moe.packed()[1][0][2].data_ptr()
        assert torch.equal(model.state_dict()["model.layers.0.moe.mlp.2.down_proj.codes"], moe.packed()[1][0][2])


@pytest.mark.parametrize("arch", ARCHS)
def test_state_dicts_and_checkpoints_load_into_the_stacked_buffers(tp1, arch):
    model, shape = build(arch)
    g, pfx, _, w0 = moe_oracle.load_case("a")
    wq = qo.quant_weights(w0, shape)
    named = wq if arch == ARCHS[0] else qo.naive_names(wq, shape.E)
    model.load_full_state_dict(named)
    I = shape.inter
    for i, moe in enumerate(model.moe_blocks()):
        p13, p2 = moe.packed()
        for leaf, t13, t2 in zip(("codes", "meta", "scales"), p13, p2):
            assert torch.equal(t13, wq[f"model.layers.{i}.moe.mlp.gate_up_proj.{leaf}"])
            assert torch.equal(t2, wq[f"model.layers.{i}.moe.mlp.down_proj.{leaf}"])
        assert torch.equal(moe.base_mlp.gate_up_proj.weight, wq[f"model.layers.{i}.moe.base_mlp.gate_up_proj.weight"])
        assert torch.equal(moe.gate.weight, w0[f"model.layers.{i}.moe.gate.weight"].half())
    # an HF-style checkpoint: q / k / v and gate / up apart, the packed gate_proj | up_proj stacked by rows
    other, _ = build(arch)
    ckpt = []
    for k, v in named.items():
        if "gate_up_proj" in k:
            rows = 0 if k.endswith("weight") else v.dim() - (1 if k.endswith("scales") else 2)
            a, b = v.split(I, dim=rows)
            ckpt += [(k.replace("gate_up_proj", "up_proj"), b), (k.replace("gate_up_proj", "gate_proj"), a)]
        elif "qkv_proj" in k:
            D = shape.D
            q, kk, vv = v.split([shape.Hq * D, shape.Hkv * D, shape.Hkv * D], 0)
            ckpt += [(k.replace("qkv_proj", "q_proj"), q), (k.replace("qkv_proj", "k_proj"), kk),
                     (k.replace("qkv_proj", "v_proj"), vv)]
        else:
            ckpt.append((k, v))
    other.load_weights(ckpt)
    sa, sb = model.state_dict(), other.state_dict()
    assert set(sa) == set(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    # the reference's own triple is refused by name
    marlin = dict(named)
    key = next(k for k in named if k.endswith("gate_up_proj.codes"))
    marlin[key.replace("codes", "qweight")] = marlin.pop(key)
    with pytest.raises(NotImplementedError, match="Marlin"):
        model.load_full_state_dict(marlin)
    with pytest.raises(NotImplementedError, match="Marlin"):
        model.load_full_state_dict({**named, key.replace("codes", "workspace"): torch.zeros(4)})
    bad = dict(named)
    bad[key] = named[key].float()
    with pytest.raises(RuntimeError, match="uint8"):
        model.load_full_state_dict(bad)


def test_pack_experts_from_dense_and_the_native_wrappers_refuse_host_tensors():
    from scratchpad_amd import _native
    from scratchpad_amd.delta import unpack_delta
    from scratchpad_amd.llama_quant_moe import pack_experts_from_dense
    g = torch.Generator().manual_seed(9)
    w13, w2 = torch.randn(3, 128, 64, generator=g) * 0.05, torch.randn(3, 64, 64, generator=g) * 0.05
    p13, p2 = pack_experts_from_dense(w13, w2, torch.bfloat16)
    assert tuple(p13[0].shape) == (3, 128, 16) and tuple(p13[1].shape) == (3, 128, 8) and tuple(p13[2].shape) == (3, 128)
    assert tuple(p2[0].shape) == (3, 64, 16) and p2[2].dtype == torch.bfloat16
    d = unpack_delta(p13[0][1], p13[1][1], p13[2][1])
    kept = d != 0
    assert float((d - w13[1])[kept].abs().max()) <= 0.51 * float(p13[2][1].float().max())
    assert set(_native.QMOE_CALLS) == {"gate_up", "down", "combine"}
    x = torch.zeros(2, 64, dtype=torch.bfloat16)
    off, pos = torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="device tensors"):
        _native.qmoe_gate_up(x, p13, off, pos, 2)
    with pytest.raises(RuntimeError, match="device tensors"):
        _native.qmoe_down(torch.zeros(4, 64, dtype=torch.bfloat16), p2, torch.zeros(2, 2), off, pos, 2)
    with pytest.raises(RuntimeError, match="device tensors"):
        _native.qmoe_combine(torch.zeros(4, 64, dtype=torch.bfloat16), torch.zeros(2, 2, dtype=torch.int32), 3, x, 0)
