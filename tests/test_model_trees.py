"""The parameter tree of every served model class, pinned (no GPU).

``ModelRunner.load_model(init_weights=True)`` walks ``named_parameters()`` with ONE generator, so the order of that
list - not only its names and shapes - decides every random-init model the benchmark and the tests build: a refactor
of the model files that registers a module earlier or later changes all of them without failing any fixture test
(fixtures load by name).  tests/golden/model_trees.json holds, per class, the ordered ``[name, shape]`` list of
``named_parameters(remove_duplicate=False)`` and the sorted ``named_modules()`` names, built on the meta device from
the tiny fixture configurations the host tests use.

The file was recorded from the commit BEFORE the decoder skeleton was shared (each of llama.py, qwen3.py, apertus.py
and llama_moe.py still carrying its own layer, model and causal-LM class), by running ``model_trees()`` of this module
there and dumping its result with ``json.dump(..., indent=0, sort_keys=True)``.  It is never to be re-recorded from
the code under test: a difference is a finding."""
import json
import os

import pytest
import torch

from tests import apertus_oracle, embedding_cases, golden, moe_oracle, qwen3_oracle, smoke_impl

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_trees.json")


def _configs():
    """(class, tiny fixture config) of the six served model classes"""
    from scratchpad_amd.apertus import SwissAIForCausalLM
    from scratchpad_amd.llama import LlamaForCausalLM
    from scratchpad_amd.llama_embedding import LlamaEmbeddingModel
    from scratchpad_amd.llama_moe import LlamaMoEForCausalLM
    from scratchpad_amd.mllama import MllamaForConditionalGeneration
    from scratchpad_amd.model_runner import ModelConfig
    from scratchpad_amd.qwen3 import Qwen3ForCausalLM
    sh = smoke_impl.load_case("a")[2]
    llama = ModelConfig(sh.hidden, sh.inter, sh.layers, sh.Hq, sh.Hkv, sh.vocab, context_len=60,
                        rms_norm_eps=sh.rms_eps, rope_theta=sh.rope_theta, max_position_embeddings=sh.max_pos,
                        tie_word_embeddings=sh.tie)
    g = golden.load("tiny_mllama")
    hidden, inter, nl, Hq, Hkv, vocab = (int(x) for x in g["cfg"])
    mllama = ModelConfig(hidden, inter, nl, Hq, Hkv, vocab, context_len=60, rms_norm_eps=1e-5, rope_theta=500000.0,
                         max_position_embeddings=128, cross_attention_layers=[int(x) for x in g["cross_layers"]])
    return [(LlamaForCausalLM, llama),
            (Qwen3ForCausalLM, qwen3_oracle.model_config(qwen3_oracle.load_case("a")[2])),
            (SwissAIForCausalLM, apertus_oracle.model_config(apertus_oracle.load_case("a")[2])),
            (LlamaMoEForCausalLM, moe_oracle.model_config(moe_oracle.load_case("a")[2])),
            (LlamaEmbeddingModel, embedding_cases.model_case("llama")[2]),
            (MllamaForConditionalGeneration, mllama)]


def model_trees():
    from scratchpad_amd import distributed as dist_
    if not dist_.model_parallel_is_initialized():
        dist_.initialize_model_parallel(1)
    trees = {}
    for cls, cfg in _configs():
        with torch.device("meta"):
            model = cls(cfg)
        trees[cls.__name__] = {
            "parameters": [[n, list(p.shape)] for n, p in model.named_parameters(remove_duplicate=False)],
            "modules": sorted(n for n, _ in model.named_modules())}
    return trees


@pytest.fixture(scope="module")
def trees():
    return model_trees()


@pytest.mark.parametrize("cls", ["LlamaForCausalLM", "Qwen3ForCausalLM", "SwissAIForCausalLM", "LlamaMoEForCausalLM",
                                 "LlamaEmbeddingModel", "MllamaForConditionalGeneration"])
def test_parameter_order_and_module_names_are_the_recorded_ones(trees, cls):
    with open(GOLDEN) as f:
        want = json.load(f)[cls]
    got = trees[cls]
    assert len(want["parameters"]) > 4
    assert got["parameters"] == want["parameters"], "named_parameters(): names, shapes or ORDER moved"
    assert got["modules"] == want["modules"], sorted(set(got["modules"]) ^ set(want["modules"]))
