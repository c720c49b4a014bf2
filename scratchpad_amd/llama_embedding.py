"""Llama / Mistral decoder served as an embedding model.

Re-hosts nn/models/llama/llama_embedding.py (LlamaEmbeddingModel 14-77): ``self.model`` is a LlamaModel and
``self.pooler`` a Pooler(LAST, normalize=True); there is no LM head and no logits processor, so the parameter names
are LlamaModel's under ``model.`` and a checkpoint's ``lm_head.*`` is skipped.  ``forward`` is the decoder followed by
the pooler (llama.pooled_embedding: at TP = 1 the final norm, the last-token gather and the L2 normalisation are one
sp_embedding_pool launch) and returns an EmbeddingPoolerOutput of [B, hidden] rows in the model dtype."""
from typing import Dict, Iterable, Tuple

import torch
from torch import nn

from .forward_info import ForwardBatch
from .layers import EmbeddingPoolerOutput, Pooler, PoolingType
from .llama import LlamaForCausalLM, LlamaModel, pooled_embedding


class LlamaEmbeddingModel(nn.Module):
    def __init__(self, config, dtype=None):
        super().__init__()
        self.config = config
        self.model = LlamaModel(config, dtype)
        self.pooler = Pooler(pooling_type=PoolingType.LAST, normalize=True)

    @torch.no_grad()
    def forward(self, input_ids, positions, forward_batch: ForwardBatch, input_embeds: torch.Tensor = None,
                get_embedding: bool = True) -> EmbeddingPoolerOutput:
        assert get_embedding, "LlamaEmbeddingModel / MistralModel is only used for embedding"
        return pooled_embedding(self.model, self.pooler, input_ids, positions, forward_batch, input_embeds)

    # ---- weights: LlamaForCausalLM's loaders (they go by parameter names and ``shard_from_full`` alone)
    def load_full_state_dict(self, full: Dict[str, torch.Tensor]) -> None:
        """a tp=1 state_dict in the reference's naming; ``lm_head.*`` entries, if any, are not read"""
        LlamaForCausalLM.load_full_state_dict(self, full)

    def load_weights(self, weights: Iterable[Tuple[str, torch.Tensor]]) -> None:
        """HF checkpoint names -> merged parameters (llama_embedding.py:39-77); ``lm_head.*`` is skipped.  A
        checkpoint saved from the bare decoder names its tensors without the ``model.`` prefix: it is added."""
        def named():
            for name, w in weights:
                if name.startswith("lm_head."):
                    continue
                yield (name if name.startswith("model.") else "model." + name), w
        LlamaForCausalLM.load_weights(self, named())


EntryClass = [LlamaEmbeddingModel]
