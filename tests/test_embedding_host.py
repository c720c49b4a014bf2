"""Host side of embedding requests (no GPU): ModelConfig.is_generation and the llama_embedding architecture, the module
tree and weight loading of scratchpad_amd/llama_embedding.py against the fixture the reference's LlamaEmbeddingModel
wrote, and the refusals - a decode batch, return_logprob, sampling on a non-generative runner, Apertus and Llama-MoE."""
import inspect
from types import SimpleNamespace

import pytest
import torch

from tests import embedding_cases as cases


@pytest.fixture()
def tp1():
    from scratchpad_amd import distributed as dist_
    if not dist_.model_parallel_is_initialized():
        dist_.initialize_model_parallel(1)
    return dist_


@pytest.mark.parametrize("arch,is_embedding,want", [
    ("llama", False, True), ("llama", True, False), ("qwen3", False, True), ("qwen3", True, False),
    ("llama_embedding", False, False), ("llama_embedding", True, False)])
def test_is_generation_truth_table(arch, is_embedding, want):
    from scratchpad_amd.model_runner import ModelConfig
    cfg = ModelConfig(256, 256, 2, 4, 1, 256, architecture=arch, is_embedding=is_embedding)
    assert cfg.is_generation is want


def test_model_config_refusals_and_presets():
    import dataclasses
    from scratchpad_amd.model_runner import ModelConfig, ServerArgs
    with pytest.raises(ValueError, match="architecture"):
        ModelConfig(256, 256, 2, 4, 1, 256, architecture="qwen2")
    with pytest.raises(NotImplementedError, match="embedding"):
        ModelConfig(256, 256, 2, 4, 1, 256, architecture="apertus", hidden_act="xielu", is_embedding=True)
    with pytest.raises(NotImplementedError, match="embedding"):
        ModelConfig(256, 256, 2, 4, 1, 256, architecture="llama_moe", num_experts=4, experts_per_token=2,
                    is_embedding=True)
    fields = [f.name for f in dataclasses.fields(ModelConfig)]
    assert fields[-1] == "is_embedding" and fields.index("grouped_topk") == len(fields) - 2, "behind the existing fields"
    assert [f.name for f in dataclasses.fields(ServerArgs)][-1] == "is_embedding" and ServerArgs().is_embedding is False
    e5 = ModelConfig.e5_mistral_7b()
    assert (e5.architecture, e5.hidden_size, e5.intermediate_size, e5.num_hidden_layers, e5.num_attention_heads,
            e5.num_key_value_heads, e5.vocab_size, e5.head_dim) == ("llama_embedding", 4096, 14336, 32, 32, 8, 32000, 128)
    assert not e5.is_generation and "UNVERIFIED" in ModelConfig.e5_mistral_7b.__doc__
    # the existing presets are what they were
    l8, q8, a8, moe = ModelConfig.llama3_8b(), ModelConfig.qwen3_8b(), ModelConfig.apertus_8b(), ModelConfig.llama_moe_8x7b()
    assert (l8.architecture, l8.hidden_size, l8.intermediate_size, l8.num_hidden_layers, l8.vocab_size, l8.rope_theta,
            l8.rms_norm_eps) == ("llama", 4096, 14336, 32, 128256, 500000.0, 1e-5)
    assert (q8.architecture, q8.hidden_size, q8.intermediate_size, q8.num_hidden_layers, q8.vocab_size,
            q8.head_dim) == ("qwen3", 4096, 12288, 36, 151936, 128)
    assert (a8.architecture, a8.intermediate_size, a8.hidden_act) == ("apertus", 21504, "xielu")
    assert (moe.architecture, moe.num_experts, moe.experts_per_token) == ("llama_moe", 8, 2)
    for cfg in (l8, q8, a8, moe, ModelConfig.llama32_1b(), ModelConfig.llama3_70b(), ModelConfig.qwen3_0_6b()):
        assert cfg.is_generation and cfg.is_embedding is False


def test_parameter_names_are_the_references(tp1):
    from scratchpad_amd.llama_embedding import EntryClass, LlamaEmbeddingModel
    g, pfx, cfg, w = cases.model_case("llama")
    with torch.device("meta"):
        model = LlamaEmbeddingModel(cfg)
    own = dict(model.named_parameters(remove_duplicate=False))
    assert sorted(own) == sorted(w), sorted(set(own) ^ set(w))
    assert {k: tuple(v.shape) for k, v in own.items()} == {k: tuple(v.shape) for k, v in w.items()}
    assert not any(k.startswith("lm_head") for k in own) and not hasattr(model, "logits_processor")
    assert list(model.pooler.parameters()) == [] and EntryClass == [LlamaEmbeddingModel]


def test_causal_lms_carry_a_pooler_without_parameters(tp1):
    from scratchpad_amd.layers import Pooler, PoolingType
    from scratchpad_amd.llama import LlamaForCausalLM
    from scratchpad_amd.qwen3 import Qwen3ForCausalLM
    g, pfx, cfg, w = cases.model_case("qwen3")
    with torch.device("meta"):
        for cls in (LlamaForCausalLM, Qwen3ForCausalLM):
            m = cls(cfg)
            assert isinstance(m.pooler, Pooler) and m.pooler.pooling_type == PoolingType.LAST and m.pooler.normalize
            assert not any("pooler" in k for k, _ in m.named_parameters())
            sig = inspect.signature(cls.forward)
            assert list(sig.parameters)[-1] == "get_embedding" and sig.parameters["get_embedding"].default is False
            assert inspect.signature(type(m.model).forward).parameters["before_final_norm"].default is False
    with torch.device("meta"):
        own = dict(Qwen3ForCausalLM(cfg).named_parameters(remove_duplicate=False))
    assert sorted(own) == sorted(w)


def test_load_weights_maps_hf_names_and_drops_lm_head(tp1):
    from scratchpad_amd.llama_embedding import LlamaEmbeddingModel
    g, pfx, cfg, w = cases.model_case("llama")
    D, Hq, Hkv = cfg.head_dim, cfg.num_attention_heads, cfg.num_key_value_heads
    for bare in (False, True):
        hf = []
        for k, v in w.items():
            name = k[len("model."):] if bare else k          # an e5-mistral checkpoint is the bare decoder
            if "qkv_proj" in k:
                q, kk, vv = v.split([Hq * D, Hkv * D, Hkv * D], 0)
                hf += [(name.replace("qkv_proj", "q_proj"), q), (name.replace("qkv_proj", "k_proj"), kk),
                       (name.replace("qkv_proj", "v_proj"), vv)]
            elif "gate_up_proj" in k:
                gate, up = v.chunk(2, 0)
                hf += [(name.replace("gate_up_proj", "gate_proj"), gate), (name.replace("gate_up_proj", "up_proj"), up)]
            else:
                hf.append((name, v))
        hf.append(("lm_head.weight", torch.full((cfg.vocab_size, cfg.hidden_size), 3.0)))
        model = LlamaEmbeddingModel(cfg, dtype=torch.float32)
        model.load_weights(hf)
        for k, p in model.named_parameters():
            assert torch.equal(p.data, w[k]), k
    model.load_full_state_dict(dict(w, **{"lm_head.weight": torch.zeros(1)}))


def _fb(mode, return_logprob=False):
    from scratchpad_amd.forward_info import ForwardMode
    return SimpleNamespace(forward_mode=getattr(ForwardMode, mode), return_logprob=return_logprob,
                           extend_seq_lens=None)


def test_model_refusals(tp1):
    from scratchpad_amd.layers import Pooler, PoolingType
    from scratchpad_amd.llama import LlamaForCausalLM
    from scratchpad_amd.llama_embedding import LlamaEmbeddingModel
    from scratchpad_amd.qwen3 import Qwen3ForCausalLM
    g, pfx, cfg, w = cases.model_case("qwen3")
    with torch.device("meta"):
        models = [LlamaForCausalLM(cfg), Qwen3ForCausalLM(cfg), LlamaEmbeddingModel(cfg)]
    for m in models:
        with pytest.raises(ValueError, match="decode batch"):
            m(None, None, _fb("DECODE"), get_embedding=True)
        with pytest.raises(NotImplementedError, match="return_logprob"):
            m(None, None, _fb("EXTEND", return_logprob=True), get_embedding=True)
    with pytest.raises(AssertionError, match="only used for embedding"):
        models[2](None, None, _fb("EXTEND"), get_embedding=False)
    with pytest.raises(ValueError, match="Invalid pooling type"):
        Pooler(7, True)(torch.zeros(1, 8), SimpleNamespace(extend_seq_lens=torch.ones(1, dtype=torch.int32)))
    assert [m.name for m in PoolingType] == ["LAST"] and int(PoolingType.LAST) == 0
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Pooler(PoolingType.LAST, True)(torch.zeros(1, 8), SimpleNamespace(extend_seq_lens=torch.ones(1, dtype=torch.int32)))


def test_apertus_and_llama_moe_still_refuse(tp1):
    from scratchpad_amd.apertus import SwissAIForCausalLM
    from scratchpad_amd.model_runner import ModelConfig
    cfg = ModelConfig(256, 256, 2, 4, 1, 256, architecture="apertus", hidden_act="xielu", head_dim=64)
    with torch.device("meta"):
        model = SwissAIForCausalLM(cfg)
    with pytest.raises(NotImplementedError, match="get_embedding"):
        model(None, None, None, get_embedding=True)
    from scratchpad_amd.llama_moe import LlamaMoEForCausalLM
    assert "get_embedding" not in inspect.signature(LlamaMoEForCausalLM.forward).parameters


def test_runner_and_worker_refusals_without_a_device():
    """the checks a non-generative runner makes before anything reaches the device"""
    from scratchpad_amd.model_runner import ModelRunner, TpModelWorker
    mr = ModelRunner.__new__(ModelRunner)
    mr.is_generation = False
    mr.server_args = SimpleNamespace(disable_cuda_graph=False)
    mr.graph_runner = None
    mr.init_cuda_graphs()
    assert mr.graph_runner is None
    with pytest.raises(ValueError, match="non-generative"):
        mr.sample(None, None)
    with pytest.raises(ValueError, match="non-generative"):
        mr.forward_decode(None)
    with pytest.raises(NotImplementedError, match="return_logprob"):
        mr.forward_extend(SimpleNamespace(return_logprob=True))
    worker = TpModelWorker.__new__(TpModelWorker)
    worker.model_runner = SimpleNamespace(is_generation=True)
    with pytest.raises(ValueError, match="generative runner"):
        worker.forward_batch_embedding(None)
    from scratchpad_amd.tp_worker_client import TpModelWorkerClient
    assert not hasattr(TpModelWorkerClient, "forward_batch_embedding"), "the overlap client has none upstream either"
