#!/usr/bin/env python3
"""Regenerate ``tests/golden/tiny_qwen3.npz`` by RUNNING the upstream reference's ``Qwen3ForCausalLM`` on the CPU
(needs the reference tree, see _ref_loader.py).  Data only: seeded weights and inputs, and what the reference's own
code made of them - nothing of its source text is stored.

Same flow and same recorded keys as ``tiny_llama`` (gen_golden.py, gen_tiny_llama): a ragged prefill of [5, 9, 1]
tokens, then one decode step; the reference's in-tree Triton extend / decode kernels run under the Triton interpreter
behind a ``Probe`` attention backend, and ``_to_torch(model, reverse=False, ...)`` makes every CustomOp (RMSNorm, the
per-head q_norm / k_norm among them, SiluAndMul, the rotary embedding) run its ``forward_native``.

Norm weights - q_norm and k_norm included - sit on the ``1 + 0.1 * randn`` grid, so a swapped or missing per-head
weight shows in the logits.  Every other weight sits on the exact-in-16-bit grid of the Llama generator, drawn at
its coarse step (multiples of 1/64, std 0.05): the explicit head_dim makes the attention projections of variant a alone
786k weights, and at the 1/1024 step the fixture would be about 3 MiB; this keeps it under 1 MiB.  For the same
reason the MLP and the vocabulary are small (64 and 64 / 96).

  a   hidden 256, 4 q / 2 kv heads, explicit head_dim 128 (q_size 512 != hidden), untied head, rope_theta 1e6
  b   hidden 256, 4 q / 1 kv heads, head_dim 64, tied head

Usage: python tests/golden/gen_golden_qwen3.py
"""
import os
import sys

os.environ["TRITON_INTERPRET"] = "1"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_loader  # noqa: E402

_ref_loader.install()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gen_golden import _grid, _save  # noqa: E402

torch.set_grad_enabled(False)

RMS_EPS = 1e-6
MAX_POS = 128


def gen_tiny_qwen3():
    import transformers
    import scratchpad.nn.models.qwen.qwen3 as Q
    from scratchpad.distributed import init_distributed_environment, initialize_model_parallel
    from scratchpad.memory.pool import MHATokenToKVPool, ReqToTokenPool
    from scratchpad.model_executor.cuda_graph_runner import _to_torch
    from scratchpad.model_executor.forward_info import (CaptureHiddenMode, ForwardBatch, ForwardMode,
                                                        compute_position_torch)
    from scratchpad.nn.attention.backend import AttentionBackend
    from scratchpad.nn.attention.triton_attn.decode_attention import decode_attention_fwd
    from scratchpad.nn.attention.triton_attn.extend_attention import extend_attention_fwd
    from scratchpad.nn.layers import rotary_embedding as _re

    init_distributed_environment(world_size=1, rank=0, distributed_init_method="tcp://127.0.0.1:29519",
                                 local_rank=0, backend="gloo")
    initialize_model_parallel(1)

    class Probe(AttentionBackend):
        def init_forward_metadata(self, fb):
            pass

        def forward_extend(self, q, k, v, layer, fb, save_kv_cache=True):
            q = q.reshape(-1, layer.tp_q_head_num * layer.qk_head_dim)
            o = torch.empty_like(q)
            fb.token_to_kv_pool.set_kv_buffer(layer, fb.out_cache_loc, k, v)
            extend_attention_fwd(
                q.view(-1, layer.tp_q_head_num, layer.qk_head_dim), k.contiguous(), v.contiguous(),
                o.view(-1, layer.tp_q_head_num, layer.v_head_dim),
                *fb.token_to_kv_pool.get_kv_buffer(layer.layer_id),
                fb.req_to_token_pool.req_to_token, fb.req_pool_indices, fb.seq_lens,
                fb.extend_seq_lens, fb.extend_start_loc, int(fb.extend_seq_lens.max()),
                layer.scaling, layer.logit_cap)
            return o

        def forward_decode(self, q, k, v, layer, fb, save_kv_cache=True):
            q = q.reshape(-1, layer.tp_q_head_num * layer.qk_head_dim)
            o = torch.empty_like(q)
            fb.token_to_kv_pool.set_kv_buffer(layer, fb.out_cache_loc, k, v)
            start = torch.zeros_like(fb.seq_lens)
            start[1:] = torch.cumsum(fb.seq_lens[:-1], 0)
            logits = torch.empty(layer.tp_q_head_num, int(fb.seq_lens.sum()))
            decode_attention_fwd(
                q.view(-1, layer.tp_q_head_num, layer.qk_head_dim),
                *fb.token_to_kv_pool.get_kv_buffer(layer.layer_id),
                o.view(-1, layer.tp_q_head_num, layer.v_head_dim),
                fb.req_to_token_pool.req_to_token, fb.req_pool_indices, start, fb.seq_lens,
                logits, int(fb.seq_lens.max()), layer.scaling, layer.logit_cap)
            return o

    out = {}
    variants = [
        # name, hidden, inter, layers, Hq, Hkv, head_dim, vocab, theta, tie
        ("a", 256, 64, 2, 4, 2, 128, 64, 1000000.0, False),
        ("b", 256, 64, 2, 4, 1, 64, 96, 1000000.0, True),
    ]
    for name, hidden, inter, nl, Hq, Hkv, D, vocab, theta, tie in variants:
        torch.manual_seed(208)
        cfg = transformers.Qwen3Config(
            vocab_size=vocab, hidden_size=hidden, intermediate_size=inter, num_hidden_layers=nl,
            num_attention_heads=Hq, num_key_value_heads=Hkv, head_dim=D, max_position_embeddings=MAX_POS,
            rms_norm_eps=RMS_EPS, tie_word_embeddings=tie, attention_bias=False)
        # transformers>=5 keeps RoPE params only in cfg.rope_parameters; the reference reads attributes
        cfg.rope_theta = theta
        cfg.rope_scaling = None
        model = Q.Qwen3ForCausalLM(cfg).eval()
        for pname, p in model.named_parameters():
            if "norm" in pname:
                p.data = _grid(1.0 + 0.1 * torch.randn_like(p))
            else:
                # multiples of 1/64, |k| <= 255: exact in bf16/fp16 (std 0.05)
                p.data = _grid(torch.randn_like(p) * 0.05)
        _to_torch(model, reverse=False, num_tokens=2)  # CustomOp -> forward_native
        kv = MHATokenToKVPool(96, 1, torch.float32, Hkv, D, nl, "cpu", False)
        r2t = ReqToTokenPool(4, 64, "cpu", False)
        backend = Probe()
        g = torch.Generator().manual_seed(209)
        ext = [5, 9, 1]
        bs = len(ext)
        ids = torch.randint(0, vocab, (sum(ext),), generator=g)
        req_idx = torch.tensor([2, 0, 3], dtype=torch.int64)
        slots = (torch.randperm(90, generator=g) + 1).to(torch.int64)
        out_loc = slots[: sum(ext)]
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
            req_to_token_pool=r2t, token_to_kv_pool=kv, attn_backend=backend,
            capture_hidden_mode=CaptureHiddenMode.NULL)
        res = model.forward(ids, positions, fb)
        prefill_logits = res.next_token_logits.clone()
        next_ids = torch.argmax(prefill_logits, dim=-1)

        # decode step (ScheduleBatch.prepare_for_decode: seq_lens += 1, alloc, write req_to_token)
        dec_loc = slots[sum(ext): sum(ext) + bs]
        seq2 = seq + 1
        for b in range(bs):
            r2t.req_to_token[req_idx[b], int(seq[b])] = int(dec_loc[b])
        fb2 = ForwardBatch(
            forward_mode=ForwardMode.DECODE, batch_size=bs, input_ids=next_ids, req_pool_indices=req_idx,
            seq_lens=seq2, out_cache_loc=dec_loc, seq_lens_sum=int(seq2.sum()),
            positions=torch.clamp(seq2 - 1, min=0).to(torch.int64),
            req_to_token_pool=r2t, token_to_kv_pool=kv, attn_backend=backend,
            capture_hidden_mode=CaptureHiddenMode.NULL)
        res2 = model.forward(next_ids, fb2.positions, fb2)
        decode_logits = res2.next_token_logits.clone()

        pfx = f"{name}_"
        out.update({pfx + "w::" + k: v for k, v in model.state_dict().items()})
        out.update({
            pfx + "cfg": np.array([hidden, inter, nl, Hq, Hkv, vocab, int(tie), D], np.int64),
            pfx + "rope_theta": np.float64(theta), pfx + "rms_eps": np.float64(RMS_EPS),
            pfx + "max_pos": np.int64(MAX_POS),
            pfx + "input_ids": ids, pfx + "extend_lens": ext_t, pfx + "req_pool_indices": req_idx,
            pfx + "out_cache_loc": out_loc, pfx + "positions": positions,
            pfx + "prefill_logits": prefill_logits, pfx + "next_ids": next_ids,
            pfx + "decode_out_cache_loc": dec_loc, pfx + "decode_logits": decode_logits,
            pfx + "k_buffer0_after": kv.get_key_buffer(0), pfx + "v_buffer1_after": kv.get_value_buffer(1),
        })
        _re._ROPE_DICT.clear()
    _save("tiny_qwen3", **out)


if __name__ == "__main__":
    gen_tiny_qwen3()
