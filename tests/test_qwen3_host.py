"""CPU checks of the Qwen3 work: the oracle against the reference's recorded logits, the host-side refusals of
sp_qk_norm_rotary, the ModelConfig presets, and the module tree / weight loading of scratchpad_amd/qwen3.py."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import c_header, qwen3_oracle

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
    """the bar tests/test_oracle_golden.py holds the Llama oracle to"""
    g, pfx, shape, w = qwen3_oracle.load_case(name)
    assert shape.D == {"a": 128, "b": 64}[name] and (shape.Hq * shape.D != shape.hidden) == (name == "a")
    assert np.isfinite(g[pfx + "prefill_logits"]).all() and np.isfinite(g[pfx + "decode_logits"]).all()
    l1, l2, kv = qwen3_oracle.oracle_run(name)
    close(l1, g[pfx + "prefill_logits"], atol=2e-5, rtol=1e-5)
    assert np.array_equal(l1.argmax(-1).numpy(), g[pfx + "next_ids"])
    close(l2, g[pfx + "decode_logits"], atol=2e-5, rtol=1e-5)
    close(kv.k[0], g[pfx + "k_buffer0_after"], atol=1e-5)
    close(kv.v[1], g[pfx + "v_buffer1_after"], atol=1e-5)


def test_oracle_sees_the_per_head_weights():
    """q_norm and k_norm of the fixture differ, and swapping them moves the oracle's logits: all-ones weights would
    have hidden a swapped or missing weight"""
    g, pfx, shape, w = qwen3_oracle.load_case("a")
    qn, kn = "model.layers.0.self_attn.q_norm.weight", "model.layers.0.self_attn.k_norm.weight"
    assert not torch.equal(w[qn], w[kn]) and float((w[qn] - 1).abs().max()) > 0.05
    swapped = dict(w)
    swapped[qn], swapped[kn] = w[kn], w[qn]
    l1, _, _ = qwen3_oracle.oracle_run("a")
    s1, _, _ = qwen3_oracle.oracle_run("a", w=swapped)
    assert float((l1 - s1).abs().max()) > 1e-3 * float(l1.abs().max())


# --------------------------------------------------------------------------- host-side refusals
@pytest.fixture(scope="module")
def lib():
    from scratchpad_amd import _native, build
    build.build_native(verbose=False)
    return c_header.bind(_native.lib_path())


@pytest.fixture(scope="module")
def addr():
    """a 16-byte-aligned host address standing for every non-NULL buffer: no call below reaches a launch"""
    buf = (ctypes.c_char * 4096)()
    a = ctypes.addressof(buf)
    yield a + (-a) % 16
    del buf


def test_qk_norm_rotary_refuses_on_the_host(lib, addr):
    a = addr
    good = dict(positions=a, q=a, k=a, q_norm_weight=a, k_norm_weight=a, eps=1e-6, cos_sin_cache=a, num_tokens=5,
                num_q_heads=4, num_kv_heads=2, head_size=128, rotary_dim=128, q_stride=1024, k_stride=1024, is_neox=1,
                v=a, v_stride=1024, k_buffer=a, v_buffer=a, out_cache_loc=a, kv_buffer_stride=256,
                dtype=DT["SP_BF16"], stream=None)
    assert set(good) == {p for p, _ in lib.sp_prototypes["sp_qk_norm_rotary"][1]}
    call = lambda **kw: c_header.call(lib, "sp_qk_norm_rotary", **{**good, **kw})
    for p in ("positions", "q", "k", "q_norm_weight", "k_norm_weight", "cos_sin_cache"):
        assert call(**{p: None}) == INVALID, p
    for k in ("num_tokens", "num_q_heads", "num_kv_heads", "head_size"):
        assert call(**{k: -good[k]}) == INVALID, k
    assert call(rotary_dim=127) == INVALID, "odd rotary_dim"
    assert call(rotary_dim=130) == INVALID, "rotary_dim > head_size"
    assert call(rotary_dim=-128) == INVALID
    # the store is all NULL or all set
    for p in ("v", "k_buffer", "v_buffer", "out_cache_loc"):
        assert call(**{p: None}) == INVALID, p
    assert call(kv_buffer_stride=-256) == INVALID
    # shapes the kernel is not built for are refused before any launch: the caller issues the three launches
    assert call(head_size=80, rotary_dim=80) == UNSUPPORTED
    assert call(rotary_dim=32) == UNSUPPORTED
    assert call(q_stride=1028) == UNSUPPORTED
    assert call(q=a + 4) == UNSUPPORTED
    assert call(dtype=DT["SP_FP8_E5M2"]) == UNSUPPORTED
    assert call(num_tokens=0) == OK


def test_native_wrapper_refuses_host_tensors():
    from scratchpad_amd import _native
    t = torch.zeros(2, 128)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _native.qk_norm_rotary(torch.zeros(2, dtype=torch.int64), t, t.clone(), torch.ones(128), torch.ones(128), 1e-6,
                               128, torch.zeros(8, 128), True)


# --------------------------------------------------------------------------- ModelConfig
def test_model_config_presets():
    from scratchpad_amd.model_runner import ModelConfig
    small = ModelConfig.qwen3_0_6b()
    assert small.architecture == "qwen3" and small.head_dim == 128 != small.hidden_size // small.num_attention_heads
    assert (small.hidden_size, small.intermediate_size, small.num_hidden_layers, small.num_attention_heads,
            small.num_key_value_heads, small.tie_word_embeddings) == (1024, 3072, 28, 16, 8, True)
    big = ModelConfig.qwen3_8b()
    assert (big.hidden_size, big.intermediate_size, big.num_hidden_layers, big.num_attention_heads,
            big.num_key_value_heads, big.head_dim, big.vocab_size, big.rope_theta, big.rms_norm_eps,
            big.tie_word_embeddings, big.architecture) == (4096, 12288, 36, 32, 8, 128, 151936, 1e6, 1e-6, False, "qwen3")
    # existing presets and plain constructions are untouched
    for cfg in (ModelConfig.llama3_8b(), ModelConfig.llama32_1b(), ModelConfig.llama3_70b(),
                ModelConfig.mllama_11b_text(), ModelConfig(256, 256, 2, 4, 1, 256)):
        assert cfg.architecture == "llama" and cfg.attention_bias is False
    l8 = ModelConfig.llama3_8b()
    assert (l8.hidden_size, l8.intermediate_size, l8.num_hidden_layers, l8.head_dim, l8.rope_theta,
            l8.rms_norm_eps) == (4096, 14336, 32, 128, 500000.0, 1e-5)
    with pytest.raises(ValueError, match="architecture"):
        ModelConfig(256, 256, 2, 4, 1, 256, architecture="qwen2")


# --------------------------------------------------------------------------- module tree and loading
@pytest.fixture()
def tp1():
    from scratchpad_amd import distributed as dist_
    if not dist_.model_parallel_is_initialized():
        dist_.initialize_model_parallel(1)
    return dist_


@pytest.mark.parametrize("name", ["a", "b"])
def test_parameter_names_are_the_references(tp1, name):
    from scratchpad_amd.qwen3 import Qwen3ForCausalLM
    g, pfx, shape, w = qwen3_oracle.load_case(name)
    with torch.device("meta"):
        model = Qwen3ForCausalLM(qwen3_oracle.model_config(shape))
    own = dict(model.named_parameters(remove_duplicate=False))
    assert sorted(own) == sorted(w), sorted(set(own) ^ set(w))
    assert {k: tuple(v.shape) for k, v in own.items()} == {k: tuple(v.shape) for k, v in w.items()}
    assert "model.layers.1.self_attn.q_norm.weight" in own and "model.layers.1.self_attn.k_norm.weight" in own


def test_load_weights_maps_hf_names(tp1):
    """q_proj / k_proj / v_proj and gate_proj / up_proj of an HF checkpoint land in the merged parameters"""
    from scratchpad_amd.qwen3 import Qwen3ForCausalLM
    g, pfx, shape, w = qwen3_oracle.load_case("b")
    D, Hq, Hkv = shape.D, shape.Hq, shape.Hkv
    hf = []
    for k, v in w.items():
        if "qkv_proj" in k:
            q, kk, vv = v.split([Hq * D, Hkv * D, Hkv * D], 0)
            hf += [(k.replace("qkv_proj", "q_proj"), q), (k.replace("qkv_proj", "k_proj"), kk),
                   (k.replace("qkv_proj", "v_proj"), vv)]
        elif "gate_up_proj" in k:
            gate, up = v.chunk(2, 0)
            hf += [(k.replace("gate_up_proj", "gate_proj"), gate), (k.replace("gate_up_proj", "up_proj"), up)]
        else:
            hf.append((k, v))
    hf.append(("lm_head.weight", w["model.embed_tokens.weight"]))          # tied checkpoints may carry it
    hf.append(("model.layers.0.self_attn.rotary_emb.inv_freq", torch.zeros(D // 2)))
    model = Qwen3ForCausalLM(qwen3_oracle.model_config(shape), dtype=torch.float32)
    model.load_weights(hf)
    for k, p in model.named_parameters():
        assert torch.equal(p.data, w[k]), k
    assert model.lm_head is model.model.embed_tokens


def test_attention_bias_is_refused(tp1):
    from scratchpad_amd.qwen3 import Qwen3Attention, Qwen3ForCausalLM
    with pytest.raises(NotImplementedError, match="attention_bias"):
        Qwen3Attention(256, 4, 2, head_dim=128, attention_bias=True)
    g, pfx, shape, w = qwen3_oracle.load_case("b")
    cfg = qwen3_oracle.model_config(shape)
    cfg.attention_bias = True
    with pytest.raises(NotImplementedError, match="attention_bias"), torch.device("meta"):
        Qwen3ForCausalLM(cfg)
