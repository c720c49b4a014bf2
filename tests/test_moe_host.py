"""Host side of the Llama-MoE work (no launch): header / SIGNATURES / exports, the refusals of the four sp_moe_* entries
through the header binding (every call below carries an argument that is refused BEFORE a launch), the oracle against
the reference's recorded run (logits, selected experts, the fixture's router-gap condition in fp32, bf16 and fp16), the
stacked expert storage and the checkpoint loader of scratchpad_amd/llama_moe.py, ModelConfig's refusals and preset."""
import ctypes

import numpy as np
import pytest
import torch

from tests import c_header, moe_oracle

STATUS = c_header.enum_values("sp_status")
OK, INVALID, UNSUPPORTED = STATUS["SP_OK"], STATUS["SP_ERR_INVALID_ARG"], STATUS["SP_ERR_UNSUPPORTED"]
DT = c_header.enum_values("sp_dtype")
ENTRIES = ("sp_moe_route", "sp_moe_gate_up", "sp_moe_down", "sp_moe_combine", "sp_moe_block_rows", "sp_moe_max_tokens")


# --------------------------------------------------------------------------- header and host-side refusals
def test_header_declares_the_entries():
    from scratchpad_amd import _native
    protos = c_header.prototypes()
    assert c_header.abi_version() == 10
    assert [n for n, _ in protos["sp_moe_route"][1]] == [
        "topk_ids", "topk_weights", "expert_offsets", "sorted_pos", "router_logits", "num_tokens", "num_experts",
        "top_k", "logits_stride", "dtype", "stream"]
    assert [n for n, _ in protos["sp_moe_gate_up"][1]] == [
        "h", "x", "w13", "expert_offsets", "sorted_pos", "num_tokens", "top_k", "num_experts", "hidden", "inter",
        "x_stride", "h_stride", "w_expert_stride", "dtype", "stream"]
    assert [n for n, _ in protos["sp_moe_down"][1]] == [
        "tmp", "h", "w2", "topk_weights", "expert_offsets", "sorted_pos", "num_tokens", "top_k", "num_experts",
        "hidden", "inter", "h_stride", "tmp_stride", "w_expert_stride", "dtype", "stream"]
    assert [n for n, _ in protos["sp_moe_combine"][1]] == [
        "out", "tmp", "topk_ids", "num_tokens", "top_k", "num_experts", "hidden", "tmp_stride", "out_stride", "dtype",
        "stream"]
    for name in ENTRIES:
        res, args = protos[name]
        assert _native.SIGNATURES[name] == (res, [t for _, t in args])
    assert set(_native.MOE_CALLS) == {"route", "gate_up", "down", "combine", "fallback"}


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


def test_entries_are_exported_and_the_constants_agree(lib):
    from scratchpad_amd import _native
    for name in ENTRIES:
        assert getattr(lib, name) is not None
    assert c_header.call(lib, "sp_moe_block_rows") == _native.MOE_BLOCK_ROWS == 32
    assert c_header.call(lib, "sp_moe_max_tokens") == _native.MOE_MAX_TOKENS == 16384
    assert (_native.MOE_MAX_EXPERTS, _native.MOE_MAX_TOP_K) == (64, 8)


def test_route_refuses_on_the_host(lib, addr):
    a = addr
    good = dict(topk_ids=a, topk_weights=a, expert_offsets=a, sorted_pos=a, router_logits=a, num_tokens=5,
                num_experts=8, top_k=2, logits_stride=12, dtype=DT["SP_BF16"], stream=None)
    assert set(good) == {p for p, _ in lib.sp_prototypes["sp_moe_route"][1]}
    call = lambda **kw: c_header.call(lib, "sp_moe_route", **{**good, **kw})
    for p in ("topk_ids", "topk_weights", "expert_offsets", "sorted_pos", "router_logits"):
        assert call(**{p: None}) == INVALID, p
    assert call(num_tokens=-5) == INVALID and call(num_experts=-8) == INVALID and call(top_k=-2) == INVALID
    assert call(num_experts=65, logits_stride=65) == UNSUPPORTED, "E > 64"
    assert call(top_k=9, num_experts=16, logits_stride=16) == UNSUPPORTED, "K > 8"
    assert call(top_k=5, num_experts=4) == UNSUPPORTED, "K > E"
    assert call(top_k=0) == UNSUPPORTED and call(num_experts=0, top_k=0) == UNSUPPORTED
    assert call(num_tokens=16385) == UNSUPPORTED, "T above sp_moe_max_tokens()"
    assert call(dtype=DT["SP_FP8_E5M2"]) == UNSUPPORTED
    assert call(logits_stride=7) == INVALID
    assert call(num_tokens=0) == OK and call(num_tokens=0, router_logits=None) == OK


def test_gate_up_refuses_on_the_host(lib, addr):
    a = addr
    good = dict(h=a, x=a, w13=a, expert_offsets=a, sorted_pos=a, num_tokens=5, top_k=2, num_experts=4, hidden=128,
                inter=64, x_stride=136, h_stride=72, w_expert_stride=2 * 64 * 128, dtype=DT["SP_BF16"], stream=None)
    assert set(good) == {p for p, _ in lib.sp_prototypes["sp_moe_gate_up"][1]}
    call = lambda **kw: c_header.call(lib, "sp_moe_gate_up", **{**good, **kw})
    for p in ("h", "x", "w13", "expert_offsets", "sorted_pos"):
        assert call(**{p: None}) == INVALID, p
    assert call(num_tokens=-5) == INVALID and call(hidden=-128) == INVALID and call(inter=-64) == INVALID
    assert call(dtype=DT["SP_F32"]) == UNSUPPORTED, "the MFMA entries are 16-bit"
    assert call(num_experts=65) == UNSUPPORTED and call(top_k=9, num_experts=16) == UNSUPPORTED
    assert call(top_k=5) == UNSUPPORTED, "K > E"
    assert call(num_tokens=16385) == UNSUPPORTED
    assert call(hidden=100, x_stride=104) == UNSUPPORTED, "H % 32"
    assert call(inter=40) == UNSUPPORTED, "I % 32"
    assert call(x_stride=120) == INVALID and call(h_stride=56) == INVALID
    assert call(w_expert_stride=2 * 64 * 128 - 8) == INVALID
    assert call(x_stride=137) == INVALID and call(x=a + 2) == INVALID and call(w13=a + 8) == INVALID
    assert call(num_tokens=0) == OK and call(num_tokens=0, x=None) == OK


def test_down_refuses_on_the_host(lib, addr):
    a = addr
    good = dict(tmp=a, h=a, w2=a, topk_weights=a, expert_offsets=a, sorted_pos=a, num_tokens=5, top_k=2,
                num_experts=4, hidden=128, inter=64, h_stride=72, tmp_stride=136, w_expert_stride=64 * 128,
                dtype=DT["SP_F16"], stream=None)
    assert set(good) == {p for p, _ in lib.sp_prototypes["sp_moe_down"][1]}
    call = lambda **kw: c_header.call(lib, "sp_moe_down", **{**good, **kw})
    for p in ("tmp", "h", "w2", "topk_weights", "expert_offsets", "sorted_pos"):
        assert call(**{p: None}) == INVALID, p
    assert call(num_tokens=-5) == INVALID and call(top_k=-2) == INVALID
    assert call(dtype=DT["SP_F32"]) == UNSUPPORTED
    assert call(num_experts=65) == UNSUPPORTED and call(top_k=9, num_experts=16) == UNSUPPORTED
    assert call(top_k=5) == UNSUPPORTED and call(num_tokens=16385) == UNSUPPORTED
    assert call(hidden=100) == UNSUPPORTED and call(inter=40, h_stride=40) == UNSUPPORTED
    assert call(h_stride=56) == INVALID and call(tmp_stride=120) == INVALID
    assert call(w_expert_stride=64 * 128 - 8) == INVALID
    assert call(h_stride=73) == INVALID and call(h=a + 2) == INVALID and call(w2=a + 4) == INVALID
    assert call(num_tokens=0) == OK


def test_combine_refuses_on_the_host(lib, addr):
    a = addr
    good = dict(out=a, tmp=a, topk_ids=a, num_tokens=5, top_k=2, num_experts=4, hidden=128, tmp_stride=136,
                out_stride=144, dtype=DT["SP_BF16"], stream=None)
    assert set(good) == {p for p, _ in lib.sp_prototypes["sp_moe_combine"][1]}
    call = lambda **kw: c_header.call(lib, "sp_moe_combine", **{**good, **kw})
    for p in ("out", "tmp", "topk_ids"):
        assert call(**{p: None}) == INVALID, p
    assert call(num_tokens=-5) == INVALID and call(hidden=-128) == INVALID
    assert call(dtype=DT["SP_F32"]) == UNSUPPORTED
    assert call(num_experts=65) == UNSUPPORTED and call(top_k=9, num_experts=16) == UNSUPPORTED
    assert call(top_k=5) == UNSUPPORTED and call(num_tokens=16385) == UNSUPPORTED
    assert call(hidden=100) == UNSUPPORTED
    assert call(tmp_stride=120) == INVALID and call(out_stride=120) == INVALID and call(out_stride=145) == INVALID
    assert call(out=a + 2) == INVALID and call(tmp=a + 8) == INVALID
    assert call(num_tokens=0) == OK


def test_native_wrappers_refuse_host_tensors():
    from scratchpad_amd import _native
    x = torch.zeros(2, 64, dtype=torch.bfloat16)
    w13, w2 = torch.zeros(4, 64, 64, dtype=torch.bfloat16), torch.zeros(4, 64, 32, dtype=torch.bfloat16)
    idx = torch.zeros(5, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _native.moe_route(torch.zeros(2, 4), 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _native.moe_gate_up(x, w13, idx, idx, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _native.moe_down(torch.zeros(4, 32, dtype=torch.bfloat16), w2, torch.zeros(2, 2), idx, idx, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _native.moe_combine(torch.zeros(4, 64, dtype=torch.bfloat16), torch.zeros(2, 2, dtype=torch.int32), 4)


def test_the_per_expert_loop_refuses_graph_capture(monkeypatch):
    from scratchpad_amd import _native
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    x = torch.zeros(2, 64)
    with pytest.raises(RuntimeError, match="cannot be captured"):
        _native.moe_experts_eager(x, torch.zeros(2, 4), torch.zeros(4, 64, 64), torch.zeros(4, 64, 32), 2)


# --------------------------------------------------------------------------- the oracle's own statements
def test_oracle_route_ties_order_and_weights():
    ids, w = moe_oracle.route(torch.tensor([[1.0, 1.0, 1.0, 1.0], [0.0, 2.0, 2.0, -1.0]], dtype=torch.bfloat16), 3)
    assert ids.tolist() == [[0, 1, 2], [1, 2, 0]]
    assert torch.equal(w[0], torch.tensor([1 / 3] * 3).bfloat16().float())
    want = torch.softmax(torch.tensor([2.0, 2.0, 0.0]), 0).bfloat16().float()
    assert torch.equal(w[1], want)
    off, pos = moe_oracle.sort_pairs(torch.tensor([[2, 0], [0, 2], [1, 2]]), 4)
    assert off.tolist() == [0, 2, 3, 6, 6] and pos.tolist() == [1, 2, 4, 0, 3, 5]


def test_oracle_experts_bound_is_zero_away_from_rounding_boundaries():
    """the derived bound is an interval carried through the roundings: small next to the values, and the statement
    itself equals the plain-torch block on the same inputs up to that bound"""
    g = torch.Generator().manual_seed(11)
    T, H, inter, E, K = 6, 64, 32, 4, 2
    x = (torch.randn(T, H, generator=g)).bfloat16()
    w13 = (torch.randn(E, 2 * inter, H, generator=g) * 0.1).bfloat16()
    w2 = (torch.randn(E, H, inter, generator=g) * 0.1).bfloat16()
    gate = (torch.randn(E, H, generator=g) * 0.5).bfloat16()
    ids, wts = moe_oracle.route(torch.nn.functional.linear(x, gate), K)
    out, bound = moe_oracle.experts(x, w13, w2, ids, wts)
    assert float((bound == 0).double().mean()) > 0.5, "most elements sit away from every rounding boundary"
    assert float(bound.max()) <= 2.0 ** -6 * float(out.abs().max())
    blk, _, sel = moe_oracle.moe_block(x, gate, list(w13), list(w2), K)
    assert torch.equal(sel.sort(-1).values, ids.sort(-1).values)
    assert bool(((blk.double() - out).abs() <= bound + 1e-30).all())


# --------------------------------------------------------------------------- oracle vs the reference's run
CASES = {"a": (2, 1, 64, 64, 64, False, 4, 2), "b": (2, 1, 128, 32, 96, True, 8, 3)}


@pytest.mark.parametrize("name", ["a", "b"])
def test_oracle_reproduces_the_reference_logits_and_experts(name):
    g, pfx, shape, w = moe_oracle.load_case(name)
    assert (shape.Hq, shape.Hkv, shape.D, shape.inter, shape.vocab, shape.tie, shape.E, shape.K) == CASES[name]
    assert shape.layers == 2
    l1, l2, kv, t1, t2 = moe_oracle.oracle_run(name)
    for got, key in ((l1, "prefill_logits"), (l2, "decode_logits")):
        want = torch.from_numpy(g[pfx + key])
        dev = float((got - want).abs().max() / want.abs().max())
        assert dev <= 1e-4, f"{name} {key}: relative deviation {dev:.2e}"
    assert np.array_equal(l1.argmax(-1).numpy(), g[pfx + "next_ids"])
    for step, trace in (("prefill", t1), ("decode", t2)):
        for i, (_, sel) in enumerate(trace):
            assert np.array_equal(sel.numpy(), g[pfx + f"{step}_selected_experts{i}"]), (step, i)
    used = np.unique(np.concatenate([g[pfx + f"prefill_selected_experts{i}"].ravel() for i in range(2)]))
    assert len(used) >= 3, "the fixture exercises several experts"


@pytest.mark.parametrize("name", ["a", "b"])
def test_fixture_condition_router_gaps(name):
    """the smallest distance between the K-th and (K+1)-th router logit of the reference's fp32 run is >= 0.125, as
    recorded, and a 16-bit run of the oracle takes the same decision everywhere"""
    g, pfx, shape, _ = moe_oracle.load_case(name)
    ref = [(torch.from_numpy(g[pfx + f"{s}_router_logits{i}"]), None) for s in ("prefill", "decode") for i in range(2)]
    gap = moe_oracle.min_gap(ref, shape.K)
    assert gap >= 0.125 and abs(gap - float(g[pfx + "min_gap"])) < 1e-9
    for dtype in (torch.bfloat16, torch.float16):
        _, _, _, t1, t2 = moe_oracle.oracle_run(name, dtype)
        for step, trace in (("prefill", t1), ("decode", t2)):
            for i, (_, sel) in enumerate(trace):
                want = np.sort(g[pfx + f"{step}_selected_experts{i}"], -1)
                assert np.array_equal(np.sort(sel.numpy(), -1), want), (dtype, step, i)


# --------------------------------------------------------------------------- module tree, loader, config
@pytest.fixture()
def tp1():
    from scratchpad_amd import distributed as dist_
    if not dist_.model_parallel_is_initialized():
        dist_.initialize_model_parallel(1)
    return dist_


def test_module_tree_names_and_stacked_storage(tp1):
    from scratchpad_amd.llama_moe import LlamaMoEForCausalLM
    _, _, shape, w = moe_oracle.load_case("a")
    model = LlamaMoEForCausalLM(moe_oracle.model_config(shape), dtype=torch.float32)
    assert sorted(n for n, _ in model.named_parameters()) == sorted(w), "the reference's parameter names"
    model.load_full_state_dict(w)
    moe = model.model.layers[1].moe
    assert tuple(moe.w13.shape) == (4, 128, 128) and tuple(moe.w2.shape) == (4, 128, 64)
    for e in range(4):
        assert moe.mlp[e].gate_up_proj.weight.data_ptr() == moe.w13[e].data_ptr(), "a view of the stacked tensor"
        assert torch.equal(moe.w13[e], w[f"model.layers.1.moe.mlp.{e}.gate_up_proj.weight"])
        assert torch.equal(moe.w2[e], w[f"model.layers.1.moe.mlp.{e}.down_proj.weight"])
    assert torch.equal(moe.gate.weight.data, w["model.layers.1.moe.gate.weight"])
    # parameters that were moved or replaced are packed again
    moe.mlp[2].down_proj.weight.data = moe.mlp[2].down_proj.weight.data.clone() + 1
    assert not moe._packed() or moe.mlp[2].down_proj.weight.data_ptr() != moe.w2[2].data_ptr()
    moe.mlp[0].gate_up_proj.weight.data = moe.mlp[0].gate_up_proj.weight.data.clone()
    assert not moe._packed()
    moe.pack_experts()
    assert moe._packed() and torch.equal(moe.w2[2], w["model.layers.1.moe.mlp.2.down_proj.weight"] + 1)


def test_loader_stacks_gate_and_up_and_follows_exchanged_experts(tp1):
    from scratchpad_amd.llama_moe import LlamaMoEForCausalLM
    _, _, shape, w = moe_oracle.load_case("a")
    swapped = moe_oracle.swap_experts(w, layer=0, a=0, b=1)
    hf = []
    for n, t in swapped.items():
        if "qkv_proj" in n:
            q, k, v = t.split([shape.Hq * shape.D, shape.Hkv * shape.D, shape.Hkv * shape.D], 0)
            hf += [(n.replace("qkv_proj", p), x) for p, x in (("q_proj", q), ("k_proj", k), ("v_proj", v))]
        elif "gate_up_proj" in n:
            a, b = t.split([shape.inter, shape.inter], 0)
            hf += [(n.replace("gate_up_proj", "gate_proj"), a), (n.replace("gate_up_proj", "up_proj"), b)]
        else:
            hf.append((n, t))
    model = LlamaMoEForCausalLM(moe_oracle.model_config(shape), dtype=torch.float32)
    model.load_weights(hf)
    m0, m1 = model.model.layers[0].moe, model.model.layers[1].moe
    assert torch.equal(m0.w13[0], w["model.layers.0.moe.mlp.1.gate_up_proj.weight"])
    assert torch.equal(m0.w13[1], w["model.layers.0.moe.mlp.0.gate_up_proj.weight"])
    assert torch.equal(m0.w2[0], w["model.layers.0.moe.mlp.1.down_proj.weight"])
    assert torch.equal(m0.w2[1], w["model.layers.0.moe.mlp.0.down_proj.weight"])
    assert torch.equal(m0.w13[2], w["model.layers.0.moe.mlp.2.gate_up_proj.weight"])
    assert torch.equal(m1.w13[0], w["model.layers.1.moe.mlp.0.gate_up_proj.weight"]), "layer 1 is left alone"
    assert torch.equal(m0.gate.weight.data, w["model.layers.0.moe.gate.weight"]), "gate rows are left alone"
    assert torch.equal(model.model.layers[0].self_attn.qkv_proj.weight.data,
                       w["model.layers.0.self_attn.qkv_proj.weight"])


def test_exchanged_experts_move_the_oracle():
    _, _, _, w = moe_oracle.load_case("a")
    l1 = moe_oracle.oracle_run("a")[0]
    s1 = moe_oracle.oracle_run("a", w=moe_oracle.swap_experts(w))[0]
    assert float((l1 - s1).abs().max()) > 1e-3 * float(l1.abs().max())


def test_model_config_refusals_and_preset():
    from scratchpad_amd.model_runner import ModelConfig, ModelRunner, ServerArgs
    base = (64, 96, 2, 4, 2, 32)
    for arch in ("llama_quant_moe", "llama_naive_quant_moe"):
        with pytest.raises(NotImplementedError, match="quantised MoE"):
            ModelConfig(*base, architecture=arch, num_experts=4, experts_per_token=2)
    with pytest.raises(ValueError, match="llama_moe"):
        ModelConfig(*base, architecture="mixtral")
    with pytest.raises(ValueError, match="num_experts"):
        ModelConfig(*base, architecture="llama_moe")
    with pytest.raises(NotImplementedError, match="grouped_topk"):
        ModelConfig(*base, architecture="llama_moe", num_experts=4, experts_per_token=2, grouped_topk=True)
    with pytest.raises(NotImplementedError, match="64 experts"):
        ModelConfig(*base, architecture="llama_moe", num_experts=128, experts_per_token=2)
    with pytest.raises(NotImplementedError, match="top-8"):
        ModelConfig(*base, architecture="llama_moe", num_experts=16, experts_per_token=9)
    cfg = ModelConfig.llama_moe_8x7b()
    assert (cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.num_attention_heads,
            cfg.num_key_value_heads, cfg.vocab_size, cfg.head_dim) == (4096, 14336, 32, 32, 8, 32000, 128)
    assert (cfg.num_experts, cfg.experts_per_token, cfg.rope_theta, cfg.architecture) == (8, 2, 1000000.0, "llama_moe")
    assert ModelConfig.llama3_8b().num_experts is None
    # LoRA toppings on an MoE model, and TP > 1
    mr = ModelRunner.__new__(ModelRunner)
    mr.model_config, mr.tp_size, mr.server_args = cfg, 1, ServerArgs(max_toppings_per_batch=2)
    with pytest.raises(NotImplementedError, match="out of scope"):
        mr.init_toppings([object()])
    mr.tp_size, mr.device, mr.dtype = 2, "cpu", torch.bfloat16
    with pytest.raises(NotImplementedError, match="TP > 1"):
        mr.load_model(0, False)


def test_moe_layer_refuses_tp_and_grouped_topk(tp1, monkeypatch):
    from types import SimpleNamespace
    from scratchpad_amd import llama_moe
    cfg = moe_oracle.model_config(moe_oracle.load_case("a")[2])
    with pytest.raises(NotImplementedError, match="grouped_topk"):
        llama_moe.LlamaDecoderLayer(SimpleNamespace(**{**cfg.__dict__, "grouped_topk": True}), 0, torch.float32)
    monkeypatch.setattr(llama_moe, "get_tensor_model_parallel_world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="TP > 1"):
        llama_moe.LlamaMoE(64, 32, "silu", 4, 2, torch.float32)
    with pytest.raises(NotImplementedError, match="TP > 1"):
        llama_moe.LlamaMoEForCausalLM(cfg, torch.float32)
