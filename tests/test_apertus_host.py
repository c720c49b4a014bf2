"""CPU checks of the Apertus work: the oracle against the reference's recorded logits, the header and host-side
refusals of sp_xielu / sp_gemm_skinny_xielu, the XIELU module's parameters, the ModelConfig preset, and the module
tree / weight loading of scratchpad_amd/apertus.py."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import apertus_oracle, c_header

STATUS = c_header.enum_values("sp_status")
OK, INVALID, UNSUPPORTED = STATUS["SP_OK"], STATUS["SP_ERR_INVALID_ARG"], STATUS["SP_ERR_UNSUPPORTED"]
DT = c_header.enum_values("sp_dtype")


def close(got, want, atol, rtol=0.0):
    want = torch.as_tensor(np.asarray(want))
    assert got.shape == want.shape
    assert torch.allclose(got.float(), want.float(), atol=atol, rtol=rtol), float((got.float() - want.float()).abs().max())


# --------------------------------------------------------------------------- oracle vs the reference's run
@pytest.mark.parametrize("name", ["a", "b"])
def test_oracle_reproduces_the_reference_logits(name):
    g, pfx, shape, w = apertus_oracle.load_case(name)
    assert (shape.Hq, shape.Hkv, shape.D, shape.inter, shape.vocab, shape.tie) == \
        {"a": (4, 2, 64, 96, 64, False), "b": (2, 1, 128, 160, 96, True)}[name]
    assert np.isfinite(g[pfx + "prefill_logits"]).all() and np.isfinite(g[pfx + "decode_logits"]).all()
    l1, l2, kv = apertus_oracle.oracle_run(name)
    for got, key in ((l1, "prefill_logits"), (l2, "decode_logits")):
        want = torch.from_numpy(g[pfx + key])
        dev = float((got - want).abs().max() / want.abs().max())
        assert dev <= 1e-5, f"{name} {key}: relative deviation {dev:.2e}"
    assert np.array_equal(l1.argmax(-1).numpy(), g[pfx + "next_ids"])
    close(kv.k[0], g[pfx + "k_buffer0_after"], atol=1e-5)
    close(kv.v[1], g[pfx + "v_buffer1_after"], atol=1e-5)


def test_fixture_scalars_differ_per_layer_and_move_the_logits():
    """the raw activation scalars are off their initial values, exact in bf16 and distinct per layer; exchanging the
    two layers' scalars moves the oracle's logits, so an ignored or swapped scalar cannot hide"""
    g, pfx, shape, w = apertus_oracle.load_case("a")
    names = [f"model.layers.{i}.mlp.act_fn.{s}" for s in ("alpha_p", "alpha_n") for i in (0, 1)]
    vals = [float(w[n]) for n in names]
    assert vals == [0.25, -0.75, -1.0, 0.5]
    for n in names:
        assert w[n].shape == (1,) and torch.equal(w[n].bfloat16().float(), w[n].float())
    swapped = dict(w)
    swapped[names[0]], swapped[names[1]] = w[names[1]], w[names[0]]
    swapped[names[2]], swapped[names[3]] = w[names[3]], w[names[2]]
    l1, _, _ = apertus_oracle.oracle_run("a")
    s1, _, _ = apertus_oracle.oracle_run("a", w=swapped)
    assert float((l1 - s1).abs().max()) > 1e-3 * float(l1.abs().max())


def test_oracle_xielu_at_zero_and_initial_parameters():
    """x == 0 takes the second branch: an * expm1(eps), about -8e-7 at the initial parameters, and never +0"""
    from scratchpad_amd.layers import XIELU
    act = XIELU()
    y = apertus_oracle.xielu(torch.tensor([0.0, -0.0]), act.alpha_p.data, act.alpha_n.data)
    assert torch.all(y < 0) and abs(float(y[0]) + 0.8 * 9.98377799987793e-07) < 1e-9
    assert apertus_oracle.XIELU_EPS == -9.98377799987793e-07


# --------------------------------------------------------------------------- header and host-side refusals
def test_header_declares_both_entries():
    from scratchpad_amd import _native
    protos = c_header.prototypes()
    assert c_header.abi_version() == 10
    assert [n for n, _ in protos["sp_xielu"][1]] == ["out", "x", "alpha_p_raw", "alpha_n_raw", "beta", "eps",
                                                     "num_tokens", "d", "x_stride", "out_stride", "dtype", "stream"]
    skinny = [n for n, _ in protos["sp_gemm_skinny"][1]]
    i = skinny.index("epilogue")
    assert [n for n, _ in protos["sp_gemm_skinny_xielu"][1]] == \
        skinny[:i] + ["alpha_p_raw", "alpha_n_raw", "beta", "eps"] + skinny[i + 1:]
    for name in ("sp_xielu", "sp_gemm_skinny_xielu"):
        res, args = protos[name]
        assert _native.SIGNATURES[name] == (res, [t for _, t in args])


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


def test_xielu_refuses_on_the_host(lib, addr):
    a = addr
    good = dict(out=a, x=a, alpha_p_raw=a, alpha_n_raw=a, beta=0.5, eps=apertus_oracle.XIELU_EPS, num_tokens=3, d=64,
                x_stride=72, out_stride=80, dtype=DT["SP_BF16"], stream=None)
    assert set(good) == {p for p, _ in lib.sp_prototypes["sp_xielu"][1]}
    call = lambda **kw: c_header.call(lib, "sp_xielu", **{**good, **kw})
    for p in ("out", "x", "alpha_p_raw", "alpha_n_raw"):
        assert call(**{p: None}) == INVALID, p
    assert call(d=0) == INVALID and call(d=-64) == INVALID and call(num_tokens=-3) == INVALID
    assert call(x_stride=63) == INVALID and call(out_stride=63) == INVALID
    # every size and stride is in order and the dtype is looked at next ...
    assert call(dtype=DT["SP_FP8_E5M2"]) == UNSUPPORTED
    # ... and only then the pointers: host memory is refused, whichever argument carries it
    assert call() == INVALID, "host pointers must be refused before any launch"
    assert call(num_tokens=0) == OK and call(num_tokens=0, out=None) == OK


def test_gemm_skinny_xielu_refuses_on_the_host(lib, addr):
    a = addr
    good = dict(out=a, x=a, w=a, M=4, N=64, K=128, x_stride=136, w_stride=144, out_stride=72, alpha_p_raw=a,
                alpha_n_raw=a, beta=0.5, eps=apertus_oracle.XIELU_EPS, dtype=DT["SP_BF16"], stream=None)
    assert set(good) == {p for p, _ in lib.sp_prototypes["sp_gemm_skinny_xielu"][1]}
    call = lambda **kw: c_header.call(lib, "sp_gemm_skinny_xielu", **{**good, **kw})
    for p in ("out", "x", "w", "alpha_p_raw", "alpha_n_raw"):
        assert call(**{p: None}) == INVALID, p
    assert call(M=-4) == INVALID and call(N=-64) == INVALID and call(K=-128) == INVALID
    assert call(x_stride=132) == INVALID and call(out_stride=63) == INVALID
    # the shapes epilogue 0 refuses are refused here, before any launch: the caller issues the two calls
    assert call(M=17) == UNSUPPORTED and call(K=48) == UNSUPPORTED and call(dtype=DT["SP_F32"]) == UNSUPPORTED
    assert call(M=0) == OK and call(N=0) == OK


def test_native_wrappers_refuse_host_tensors():
    from scratchpad_amd import _native
    from scratchpad_amd.layers import XIELU
    x, s = torch.zeros(2, 64), torch.zeros(1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _native.xielu(x, s, s, 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _native.gemm_skinny_xielu(x, torch.zeros(32, 64), s, s, 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        XIELU()(x)
    assert set(_native.XIELU_CALLS) == {"xielu", "gemm_skinny_xielu", "two_call"}
    assert _native.XIELU_EPS == apertus_oracle.XIELU_EPS


# --------------------------------------------------------------------------- XIELU module
def test_xielu_module_has_the_references_parameters():
    from scratchpad_amd.layers import XIELU
    act = XIELU()
    assert [n for n, _ in act.named_parameters()] == ["alpha_p", "alpha_n"]
    assert act.alpha_p.shape == (1,) and act.alpha_n.shape == (1,) and act.alpha_p.dtype == torch.float32
    assert float(act.alpha_p.data) == pytest.approx(math.log(math.exp(0.8) - 1.0), rel=1e-6)
    assert float(act.alpha_n.data) == pytest.approx(math.log(math.exp(0.3) - 1.0), rel=1e-6)
    # the reference's own expressions, bit for bit
    assert torch.equal(act.alpha_p.data, torch.log(torch.exp(torch.tensor(0.8)) - 1.0).unsqueeze(0))
    assert torch.equal(act.alpha_n.data, torch.log(torch.exp(torch.tensor(0.8 - 0.5)) - 1.0).unsqueeze(0))
    assert act.beta == 0.5 and act.eps == apertus_oracle.XIELU_EPS
    other = XIELU(alpha_p_init=1.0, alpha_n_init=2.0, beta=0.25, eps=-1e-3)
    assert float(torch.nn.functional.softplus(other.alpha_p.data)) == pytest.approx(1.0, rel=1e-6)
    assert 0.25 + float(torch.nn.functional.softplus(other.alpha_n.data)) == pytest.approx(2.0, rel=1e-6)
    assert other.eps == float(torch.tensor(-1e-3, dtype=torch.bfloat16))


# --------------------------------------------------------------------------- ModelConfig
def test_model_config_accepts_apertus():
    from scratchpad_amd import _native
    from scratchpad_amd.model_runner import ModelConfig
    cfg = ModelConfig(256, 96, 2, 4, 2, 64, architecture="apertus", hidden_act="xielu")
    assert cfg.architecture == "apertus" and cfg.head_dim == 64
    with pytest.raises(ValueError, match="architecture"):
        ModelConfig(256, 96, 2, 4, 2, 64, architecture="olmo2")
    big = ModelConfig.apertus_8b()
    assert big.architecture == "apertus" and big.hidden_act == "xielu" and not big.tie_word_embeddings
    # shapes the fused q/k norm (head sizes 64 / 128 / 256) and the skinny kernel (K % 32 == 0, 16-byte rows) accept
    assert big.head_dim in (64, 128, 256) and big.num_attention_heads % big.num_key_value_heads == 0
    assert big.hidden_size % 32 == 0 and big.intermediate_size % 32 == 0
    assert big.hidden_size % 8 == 0 and big.intermediate_size % 8 == 0 and _native.SKINNY_MAX_ROWS == 16
    assert ModelConfig.apertus_8b(context_len=100000).max_position_embeddings >= 100000
    for other in (ModelConfig.llama3_8b(), ModelConfig.qwen3_8b()):
        assert other.hidden_act == "silu" and other.architecture != "apertus"


# --------------------------------------------------------------------------- module tree and loading
@pytest.fixture()
def tp1():
    from scratchpad_amd import distributed as dist_
    if not dist_.model_parallel_is_initialized():
        dist_.initialize_model_parallel(1)
    return dist_


@pytest.mark.parametrize("name", ["a", "b"])
def test_parameter_names_are_the_references(tp1, name):
    from scratchpad_amd.apertus import SwissAIForCausalLM
    g, pfx, shape, w = apertus_oracle.load_case(name)
    with torch.device("meta"):
        model = SwissAIForCausalLM(apertus_oracle.model_config(shape))
    own = dict(model.state_dict())
    assert sorted(own) == sorted(w), sorted(set(own) ^ set(w))
    assert {k: tuple(v.shape) for k, v in own.items()} == {k: tuple(v.shape) for k, v in w.items()}
    for n in ("attention_layernorm.weight", "feedforward_layernorm.weight", "self_attn.q_norm.weight",
              "self_attn.k_norm.weight", "mlp.up_proj.weight", "mlp.down_proj.weight", "mlp.act_fn.alpha_p",
              "mlp.act_fn.alpha_n"):
        assert "model.layers.1." + n in own, n
    assert not any("gate" in k for k in own)


def test_load_weights_stacks_qkv_only(tp1):
    """q_proj / k_proj / v_proj of an HF checkpoint land in qkv_proj; up_proj, down_proj and the scalars load as named"""
    from scratchpad_amd.apertus import SwissAIForCausalLM
    g, pfx, shape, w = apertus_oracle.load_case("b")
    D, Hq, Hkv = shape.D, shape.Hq, shape.Hkv
    hf = []
    for k, v in w.items():
        if "qkv_proj" in k:
            q, kk, vv = v.split([Hq * D, Hkv * D, Hkv * D], 0)
            hf += [(k.replace("qkv_proj", "q_proj"), q), (k.replace("qkv_proj", "k_proj"), kk),
                   (k.replace("qkv_proj", "v_proj"), vv)]
        else:
            hf.append((k, v))
    hf.append(("lm_head.weight", w["model.embed_tokens.weight"]))          # tied checkpoints may carry it
    hf.append(("model.layers.0.self_attn.rotary_emb.inv_freq", torch.zeros(D // 2)))
    model = SwissAIForCausalLM(apertus_oracle.model_config(shape), dtype=torch.float32)
    model.load_weights(hf)
    for k, p in model.named_parameters():
        assert torch.equal(p.data, w[k]), k
    assert model.lm_head is model.model.embed_tokens
    assert float(model.model.layers[1].mlp.act_fn.alpha_p.data) == -0.75


def test_unbuilt_branches_are_refused(tp1):
    from scratchpad_amd.apertus import SwissAIForCausalLM, SwissAIMLP
    g, pfx, shape, w = apertus_oracle.load_case("b")
    for field, value, match in (("attention_bias", True, "attention_bias"), ("mlp_bias", True, "mlp_bias"),
                                ("partial_rotary_factor", 0.5, "partial_rotary_factor"),
                                ("hidden_act", "silu", "hidden_act")):
        cfg = apertus_oracle.model_config(shape)
        setattr(cfg, field, value)
        with pytest.raises(NotImplementedError, match=match), torch.device("meta"):
            SwissAIForCausalLM(cfg)
    with pytest.raises(NotImplementedError, match="hidden_act"):
        SwissAIMLP(256, 96, "gelu")
    with torch.device("meta"):
        model = SwissAIForCausalLM(apertus_oracle.model_config(shape))
    with pytest.raises(NotImplementedError, match="get_embedding"):
        model(None, None, None, get_embedding=True)
