"""Llama / Mistral decoder served as an embedding model.

Re-hosts nn/models/llama/llama_embedding.py (LlamaEmbeddingModel 14-77): ``self.model`` is a LlamaModel and
``self.pooler`` a Pooler(LAST, normalize=True); there is no LM head and no logits processor, so the parameter names
are LlamaModel's under ``model.`` and a checkpoint's ``lm_head.*`` is skipped.  ``forward`` is the decoder followed by
the pooler (llama.pooled_embedding: at TP = 1 the final norm, the last-token gather and the L2 normalisation are one
sp_embedding_pool launch) and returns an EmbeddingPoolerOutput of [B, hidden] rows in the model dtype."""
from typing import Iterable, Tuple

import torch
from torch import nn

from .forward_info import ForwardBatch
from .layers import EmbeddingPoolerOutput, Pooler, PoolingType
from .llama import LlamaForCausalLM, LlamaModel, pooled_embedding


class LlamaEmbeddingModel(LlamaForCausalLM):
    """LlamaForCausalLM for its loaders alone (they read only the names a model owns, so a checkpoint's ``lm_head.*``
    is never read): this constructor builds neither an LM head nor a logits processor"""

    def __init__(self, config, dtype=None):
        nn.Module.__init__(self)
        self.config = config
        self.model = LlamaModel(config, dtype)
        self.pooler = Pooler(pooling_type=PoolingType.LAST, normalize=True)

    @torch.no_grad()
    def forward(self, input_ids, positions, forward_batch: ForwardBatch, input_embeds: torch.Tensor = None,
                get_embedding: bool = True) -> EmbeddingPoolerOutput:
        assert get_embedding, "LlamaEmbeddingModel / MistralModel is only used for embedding"
        return pooled_embedding(self.model, self.pooler, input_ids, positions, forward_batch, input_embeds)

    def load_weights(self, weights: Iterable[Tuple[str, torch.Tensor]]) -> None:
        """HF checkpoint names -> merged parameters (llama_embedding.py:39-77).  A checkpoint saved from the bare
        decoder names its tensors without the ``model.`` prefix: it is added."""
        super().load_weights((n if n.startswith("model.") else "model." + n, w) for n, w in weights)


EntryClass = [LlamaEmbeddingModel]
