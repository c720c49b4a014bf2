#!/usr/bin/env python3
"""Regenerate ``tests/golden/tiny_apertus.npz`` by RUNNING the upstream reference's ``SwissAIForCausalLM`` on the CPU
(needs the reference tree, see _ref_loader.py).  Data only: seeded weights and inputs, and what the reference's own
code made of them - nothing of its source text is stored.

Same flow and same recorded keys as ``tiny_qwen3`` (gen_golden_qwen3.py): a ragged prefill of [5, 9, 1] tokens, then
one decode step; the reference's in-tree Triton extend / decode kernels run under the Triton interpreter behind a
``Probe`` attention backend, and ``_to_torch(model, reverse=False, ...)`` makes every CustomOp run its
``forward_native`` (XIELU defines ``forward`` itself: plain torch).

The reference builds ``XIELU.eps`` with ``device="cuda"``, which raises on a machine without one.  While the model is
CONSTRUCTED (and only then) ``torch.tensor`` is wrapped so that ``device="cuda"`` becomes ``"cpu"``; the value - -1e-6
rounded to bf16 - is the reference's.

Norm weights (the two layer norms, q_norm, k_norm, the final norm) sit on the ``1 + 0.1 * randn`` grid, every other
matrix on the Qwen3 generator's coarse grid (multiples of 1/64, std 0.05), which keeps the file under 1 MiB.  The raw
activation scalars differ per layer, differ from their initial values and are exact in bf16 (alpha_p raw 0.25 / -0.75,
alpha_n raw -1.0 / 0.5), so an ignored or swapped scalar shows in the logits.

  a   hidden 256, 4 q / 2 kv heads (head_dim 64), intermediate 96, vocab 64, untied head
  b   hidden 256, 2 q / 1 kv heads (head_dim 128), intermediate 160, vocab 96, tied head

Usage: python tests/golden/gen_golden_apertus.py
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

RMS_EPS = 1e-5
MAX_POS = 128


ALPHA_P_RAW = [0.25, -0.75]       # per layer; the initial value is log(e^0.8 - 1) = 0.2038
ALPHA_N_RAW = [-1.0, 0.5]         # initial log(e^0.3 - 1) = -1.0503


def gen_tiny_apertus():
    import scratchpad.nn.models.swissai.apertus as A
    from scratchpad.nn.models.swissai.config import SwissAIConfig
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
        ("a", 256, 96, 2, 4, 2, 64, 64, 1000000.0, False),
        ("b", 256, 160, 2, 2, 1, 128, 96, 1000000.0, True),
    ]
    for name, hidden, inter, nl, Hq, Hkv, D, vocab, theta, tie in variants:
        torch.manual_seed(208)
        assert D == hidden // Hq           # SwissAIConfig carries no head_dim: the reference derives it
        cfg = SwissAIConfig(
            vocab_size=vocab, hidden_size=hidden, intermediate_size=inter, num_hidden_layers=nl,
            num_attention_heads=Hq, num_key_value_heads=Hkv, max_position_embeddings=MAX_POS,
            rms_norm_eps=RMS_EPS, tie_word_embeddings=tie, attention_bias=False, hidden_act="xielu")
        # transformers>=5 keeps RoPE params only in cfg.rope_parameters; the reference reads attributes
        cfg.rope_theta = theta
        cfg.rope_scaling = None
        real_tensor = torch.tensor

        def tensor_on_cpu(*a, **k):
            if str(k.get("device", "")).startswith("cuda"):
                k["device"] = "cpu"
            return real_tensor(*a, **k)

        torch.tensor = tensor_on_cpu           # XIELU.__init__: eps = torch.tensor(eps, bfloat16, device="cuda")
        try:
            model = A.SwissAIForCausalLM(cfg).eval()
        finally:
            torch.tensor = real_tensor
        for pname, p in model.named_parameters():
            if "act_fn.alpha" in pname:
                layer = int(pname.split(".")[2])
                p.data = torch.full_like(p, (ALPHA_P_RAW if pname.endswith("alpha_p") else ALPHA_N_RAW)[layer])
            elif "norm" in pname:
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
    _save("tiny_apertus", **out)


if __name__ == "__main__":
    gen_tiny_apertus()
