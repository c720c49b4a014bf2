#!/usr/bin/env python3
"""Regenerate ``tests/golden/tiny_embedding.npz`` by RUNNING the upstream reference's ``Pooler``,
``LlamaEmbeddingModel`` and ``Qwen3ForCausalLM(get_embedding=True)`` on the CPU (needs the reference tree, see
_ref_loader.py).  Data only: seeded weights and inputs, and what the reference's own code made of them - nothing of
its source text is stored.

  pool_<dtype>_<H>_*   Pooler(PoolingType.LAST, normalize=True) on [T, H] rows in fp32 / fp16 / bf16 at H = 100 and 256:
                       ragged lengths [3, 1, 4, 2, 2]; the second sequence's last row is all zeros (fp16: NaN, since
                       1e-12 is 0 there), the third one's is scaled so that its 2-norm leaves the fp16 range (fp16: the
                       norm is inf and the row comes out as zeros).  The fixture records what the reference makes of them.
  llama_* / qwen3_*    the models on the ragged prefill of [5, 9, 1] tokens of ``tiny_qwen3`` (gen_golden_qwen3.py: same
                       Probe backend over the reference's in-tree Triton extend kernel under the Triton interpreter,
                       ``_to_torch`` so that every CustomOp runs its ``forward_native``), once in fp32 and once in bf16,
                       and ``d16`` = max |bf16 embedding - fp32 embedding| of the reference itself.  (In the bf16 run
                       the attention kernel alone is handed fp32 copies of its bf16 operands: see Probe.)

Weights sit on the coarse 1/64 grid of the Qwen3 generator (exact in 16 bits, so both dtypes see the same weights),
norm weights on ``1 + 0.1 * randn``.

Usage: python tests/golden/gen_golden_embedding.py
"""
import os
import sys
import types

os.environ["TRITON_INTERPRET"] = "1"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_loader  # noqa: E402

_ref_loader.install()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gen_golden import _grid, _save  # noqa: E402

torch.set_grad_enabled(False)

MAX_POS = 128
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


def _bits(t):
    """16-bit results are stored as their bit patterns (numpy has no bfloat16)"""
    return t.view(torch.int16) if t.dtype in (torch.float16, torch.bfloat16) else t


def gen_pooler(out):
    from scratchpad.nn.layers.pooler import Pooler, PoolingType
    pooler = Pooler(PoolingType.LAST, normalize=True)
    lens = torch.tensor([3, 1, 4, 2, 2], dtype=torch.int32)
    g = torch.Generator().manual_seed(311)
    for H in (100, 256):
        x = _grid(torch.randn(int(lens.sum()), H, generator=g))
        x[3] = 0.0                       # last row of sequence 1
        x[7] *= 8192.0                   # last row of sequence 2: multiples of 128, exact in fp16, norm beyond 65504
        out[f"pool_{H}_x"] = x
        for name, dt in DTYPES.items():
            fb = types.SimpleNamespace(extend_seq_lens=lens)
            res = pooler(x.to(dt), fb).embeddings
            assert res.dtype == dt
            out[f"pool_{name}_{H}_out"] = _bits(res)
    out["pool_lens"] = lens


def gen_models(out):
    import transformers
    import scratchpad.nn.models.qwen.qwen3 as Q
    from scratchpad.distributed import init_distributed_environment, initialize_model_parallel
    from scratchpad.memory.pool import MHATokenToKVPool, ReqToTokenPool
    from scratchpad.model_executor.cuda_graph_runner import _to_torch
    from scratchpad.model_executor.forward_info import (CaptureHiddenMode, ForwardBatch, ForwardMode,
                                                        compute_position_torch)
    from scratchpad.nn.attention.backend import AttentionBackend
    from scratchpad.nn.attention.triton_attn.extend_attention import extend_attention_fwd
    from scratchpad.nn.layers import rotary_embedding as _re
    from scratchpad.nn.models.llama.llama_embedding import LlamaEmbeddingModel

    init_distributed_environment(world_size=1, rank=0, distributed_init_method="tcp://127.0.0.1:29523",
                                 local_rank=0, backend="gloo")
    initialize_model_parallel(1)

    class Probe(AttentionBackend):
        def init_forward_metadata(self, fb):
            pass

        def forward_extend(self, q, k, v, layer, fb, save_kv_cache=True):
            q = q.reshape(-1, layer.tp_q_head_num * layer.qk_head_dim)
            o = torch.empty_like(q)
            fb.token_to_kv_pool.set_kv_buffer(layer, fb.out_cache_loc, k, v)
            kb, vb = fb.token_to_kv_pool.get_kv_buffer(layer.layer_id)
            # the Triton interpreter computes on numpy arrays, which have no bfloat16 (its bf16 results are garbage):
            # a bf16 run hands the kernel exact fp32 copies of its bf16 q / k / v and pool, and rounds the output to
            # bf16 once.  Everything outside the attention kernel runs in bf16 as it stands.
            up = (lambda t: t.float()) if q.dtype == torch.bfloat16 else (lambda t: t)
            o_k = up(o)
            extend_attention_fwd(
                up(q).view(-1, layer.tp_q_head_num, layer.qk_head_dim), up(k.contiguous()), up(v.contiguous()),
                o_k.view(-1, layer.tp_q_head_num, layer.v_head_dim), up(kb), up(vb),
                fb.req_to_token_pool.req_to_token, fb.req_pool_indices, fb.seq_lens,
                fb.extend_seq_lens, fb.extend_start_loc, int(fb.extend_seq_lens.max()),
                layer.scaling, layer.logit_cap)
            if o_k is not o:
                o.copy_(o_k)
            return o

    variants = [
        # name, hidden, inter, layers, Hq, Hkv, head_dim, vocab, theta, eps
        ("llama", 128, 64, 2, 2, 1, 64, 64, 10000.0, 1e-5),
        ("qwen3", 128, 64, 2, 4, 2, 64, 64, 1000000.0, 1e-6),
    ]
    for name, hidden, inter, nl, Hq, Hkv, D, vocab, theta, eps in variants:
        torch.manual_seed(312)
        if name == "llama":
            cfg = transformers.LlamaConfig(
                vocab_size=vocab, hidden_size=hidden, intermediate_size=inter, num_hidden_layers=nl,
                num_attention_heads=Hq, num_key_value_heads=Hkv, max_position_embeddings=MAX_POS, rms_norm_eps=eps,
                tie_word_embeddings=False, attention_bias=False)
        else:
            cfg = transformers.Qwen3Config(
                vocab_size=vocab, hidden_size=hidden, intermediate_size=inter, num_hidden_layers=nl,
                num_attention_heads=Hq, num_key_value_heads=Hkv, head_dim=D, max_position_embeddings=MAX_POS,
                rms_norm_eps=eps, tie_word_embeddings=False, attention_bias=False)
        cfg.rope_theta = theta
        cfg.rope_scaling = None
        model = (LlamaEmbeddingModel(cfg) if name == "llama" else Q.Qwen3ForCausalLM(cfg)).eval()
        for pname, p in model.named_parameters():
            if "norm" in pname:
                p.data = _grid(1.0 + 0.1 * torch.randn_like(p))
            else:
                p.data = _grid(torch.randn_like(p) * 0.05)
        weights = {k: v.clone() for k, v in model.state_dict().items()}
        _to_torch(model, reverse=False, num_tokens=2)  # CustomOp -> forward_native
        g = torch.Generator().manual_seed(313)
        ext = [5, 9, 1]
        bs = len(ext)
        ids = torch.randint(0, vocab, (sum(ext),), generator=g)
        req_idx = torch.tensor([2, 0, 3], dtype=torch.int64)
        slots = (torch.randperm(90, generator=g) + 1).to(torch.int64)
        out_loc = slots[: sum(ext)]
        emb = {}
        for dname in ("fp32", "bf16"):
            dt = DTYPES[dname]
            model.to(dt)
            _re._ROPE_DICT.clear()
            kv = MHATokenToKVPool(96, 1, dt, Hkv, D, nl, "cpu", False)
            r2t = ReqToTokenPool(4, 64, "cpu", False)
            off = 0
            for b in range(bs):
                r2t.req_to_token[req_idx[b], : ext[b]] = out_loc[off: off + ext[b]].to(torch.int32)
                off += ext[b]
            pre_t = torch.zeros(bs, dtype=torch.int32)
            ext_t = torch.tensor(ext, dtype=torch.int32)
            positions, start_loc = compute_position_torch(pre_t, ext_t)
            seq = torch.tensor(ext, dtype=torch.int64)
            fb = ForwardBatch(
                forward_mode=ForwardMode.EXTEND, batch_size=bs, input_ids=ids, req_pool_indices=req_idx,
                seq_lens=seq, out_cache_loc=out_loc, seq_lens_sum=int(seq.sum()), positions=positions,
                extend_num_tokens=sum(ext), extend_seq_lens=ext_t, extend_prefix_lens=pre_t,
                extend_start_loc=start_loc, extend_prefix_lens_cpu=[0] * bs, extend_seq_lens_cpu=ext,
                req_to_token_pool=r2t, token_to_kv_pool=kv, attn_backend=Probe(),
                capture_hidden_mode=CaptureHiddenMode.NULL)
            res = model.forward(ids, positions, fb, get_embedding=True).embeddings
            assert res.dtype == dt and res.shape == (bs, hidden), (res.dtype, res.shape)
            emb[dname] = res.clone()
        pfx = f"{name}_"
        out.update({pfx + "w::" + k: v for k, v in weights.items()})
        out.update({
            pfx + "cfg": np.array([hidden, inter, nl, Hq, Hkv, vocab, 0, D], np.int64),
            pfx + "rope_theta": np.float64(theta), pfx + "rms_eps": np.float64(eps), pfx + "max_pos": np.int64(MAX_POS),
            pfx + "input_ids": ids, pfx + "extend_lens": ext_t, pfx + "req_pool_indices": req_idx,
            pfx + "out_cache_loc": out_loc, pfx + "positions": positions,
            pfx + "emb_fp32": emb["fp32"], pfx + "emb_bf16": _bits(emb["bf16"]),
            pfx + "d16": np.float64((emb["bf16"].double() - emb["fp32"].double()).abs().max()),
        })
        print(name, "d16 =", float(out[pfx + "d16"]), "norms", emb["fp32"].norm(dim=1).tolist())


def gen_tiny_embedding():
    out = {}
    gen_pooler(out)
    gen_models(out)
    _save("tiny_embedding", **out)


if __name__ == "__main__":
    gen_tiny_embedding()
