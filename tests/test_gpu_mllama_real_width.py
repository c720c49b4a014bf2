"""Config 5 through the model runner at REAL width: Mllama-11B's text widths (hidden 4096, intermediate 14336, 32 / 8
heads of 128; vocabulary cut to 32000 so the CPU oracle stays in test time), 2 decoder layers - a self-attention layer
and a cross-attention layer (cross_attention_layers = [1]) - and three image requests at the full encoder length
(6404 = 4 tiles x 1601 vision positions) beside one text-only request.  A prefill (the image-token prefill: text rows
over 6404 encoder keys, non-causal, and the self-attention behind the encoder slots) and two decode steps go through
ScheduleBatch -> ModelRunner -> the HIP kernels, eager and under HIP-graph replay (one bucket, bs 4), against
oracle/mllama.forward evaluated (a) in fp32 and (b) in the same 16-bit dtype (every op rounding its output, as torch
does).  Random cross_attention_states N(0, 1) stand in for the vision tower; weights are ModelRunner's own N(0, 0.02)
initialisation with the tanh gates at 0.5.

Metric: max |logit - ref| / max |ref| per step, as tests/test_gpu_llama_real_width.py.
Asserted: (1) the HIP path is no further from the fp32 oracle than torch's own 16-bit evaluation of the same layers
+ 10 %; (2) absolute bounds (LOOSE until a dtype has been measured, then <= 1.15 x the largest measured value).
Measured on MI355X (largest over prefill and both decode steps, eager and graph; vs fp32 oracle / vs same-dtype oracle):
  fp16: HIP vs fp32 oracle 1.23e-3 .. 1.65e-3 (torch fp16 vs fp32: 1.31e-3 .. 1.63e-3), vs fp16 oracle <= 1.11e-3
  bf16: HIP vs fp32 oracle 1.23e-2 .. 1.26e-2 (torch bf16 vs fp32: 1.18e-2 .. 1.26e-2), vs bf16 oracle <= 8.55e-3
  (max |logit| 5.5 .. 6.6; eager and graph replay give the same figures; greedy tokens equal to the fp32 oracle's on
  100 % of rows in both dtypes)"""
import pytest
import torch

from oracle import llama as ollama
from oracle import mllama as omllama
from oracle import ops

pytestmark = pytest.mark.gpu

ENC_LEN = 6404
TEXT = [64, 17, 96, 33]
ENC = [ENC_LEN, 0, ENC_LEN, ENC_LEN]        # request 1 is text-only
STEPS = 2
VOCAB = 32000

# largest measured max|dlogit| / max|logit| over the steps (MI355X): (vs fp32 oracle, vs same-dtype oracle)
MEASURED = {torch.float16: (1.65e-3, 1.11e-3), torch.bfloat16: (1.26e-2, 8.55e-3)}
LOOSE = {torch.float16: (6e-3, 6e-3), torch.bfloat16: (5e-2, 5e-2)}     # used only until a dtype has been measured


def bounds(dtype):
    m = MEASURED[dtype]
    return LOOSE[dtype] if m[0] is None else (1.15 * m[0], 1.15 * m[1])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_mllama_real_width_against_fp32_and_same_dtype_oracle(dtype):
    from types import SimpleNamespace

    from scratchpad_amd.forward_info import ForwardBatch, ForwardMode
    from scratchpad_amd.mllama import get_full_text_row_masked_out_mask
    from scratchpad_amd.model_runner import ModelConfig, ModelRunner, ServerArgs, TpModelWorker
    from scratchpad_amd.schedule_batch import Req, ScheduleBatch
    bs = len(TEXT)
    ctx = ENC_LEN + max(TEXT) + 64
    cfg = ModelConfig(4096, 14336, 2, 32, 8, VOCAB, context_len=ctx, cross_attention_layers=[1])
    slots = sum(ENC) + sum(TEXT) + bs * (STEPS + 1) + 64
    mr = ModelRunner(cfg, ServerArgs(max_total_tokens=slots, max_running_requests=bs, cuda_graph_bs=[bs]),
                     dtype=dtype, seed=3)
    mr.init_cuda_graphs()
    assert mr.graph_runner is not None
    worker = TpModelWorker(mr)
    dev = mr.device
    shape = ollama.LlamaShape(4096, 14336, 2, 32, 8, VOCAB, False, 500000.0, None, 8192, 1e-5)
    w16 = {k: v.detach().cpu() for k, v in mr.model.language_model.named_parameters()}
    w32 = {k: v.float() for k, v in w16.items()}
    gen = torch.Generator().manual_seed(11)
    states16 = torch.randn(sum(ENC), 4096, generator=gen).to(dtype)
    reqs = []
    for i, (e, n) in enumerate(zip(ENC, TEXT)):
        toks = torch.randint(0, VOCAB, (n,), generator=gen).tolist()
        reqs.append(Req(str(i), "", [0] * e + toks, None, num_image_tokens=e) if e else Req(str(i), "", toks, None))
    sb = ScheduleBatch(reqs, mr.req_to_token_pool, mr.token_to_kv_pool_allocator, device=dev, is_encoder_decoder=True)
    sb.prepare_for_extend()
    assert sb.encoder_lens_cpu == ENC and sb.extend_lens == TEXT
    batch = sb.get_model_worker_batch()
    batch.encoder_states = states16.to(dev)
    out, _ = worker.forward_batch_generation(batch, skip_sample=True)
    hip = [[out.next_token_logits.float().cpu()]]

    rows = bs + 1
    kv32 = ollama.OracleKV(shape, slots, rows, ctx + 4)
    kv16 = ollama.OracleKV(shape, slots, rows, ctx + 4, dtype=dtype)
    ext = torch.tensor(TEXT, dtype=torch.int32)
    pos, start = ops.compute_position(torch.zeros(bs, dtype=torch.int32), ext)
    fb_like = SimpleNamespace(forward_mode=ForwardMode.EXTEND, extend_seq_lens_cpu=TEXT, seq_lens_cpu=torch.tensor(TEXT),
                              seq_lens=torch.tensor(TEXT), encoder_lens_cpu=ENC)
    enc_t = torch.tensor(ENC)

    def oracle(w, kv, mode, **kw):
        kv.req_to_token.copy_(mr.req_to_token_pool.req_to_token.cpu()[:rows, :ctx + 4])
        return omllama.forward(shape, [1], w, kv, mode=mode, req_pool_indices=sb.req_pool_indices.cpu(),
                               encoder_lens=enc_t, input_ids=sb.input_ids.cpu(), seq_lens=sb.seq_lens.cpu(),
                               out_cache_loc=sb.out_cache_loc.cpu(), **kw).float()
    common = dict(positions=pos, row_mask=get_full_text_row_masked_out_mask(fb_like).float(), extend_seq_lens=ext,
                  extend_start_loc=start, encoder_out_cache_loc=sb.encoder_out_cache_loc.cpu())
    ref32 = [oracle(w32, kv32, "extend", cross_attention_states=states16.float(), **common)]
    ref16 = [oracle(w16, kv16, "extend", cross_attention_states=states16, **common)]
    row_mask = (enc_t != 0).float().view(-1, 1)
    for step in range(STEPS):
        sb.output_ids = ref32[-1].argmax(-1).to(dev)          # both sides continue from the oracle's tokens
        sb.prepare_for_decode()
        dec = sb.get_model_worker_batch()
        assert mr.graph_runner.can_run(ForwardBatch.init_new(dec, mr)), "the decode step must replay a graph"
        # eager first, then the graph replay of the same step (both store the same new K / V)
        graph_runner, mr.graph_runner = mr.graph_runner, None
        try:
            eager, _ = worker.forward_batch_generation(dec, skip_sample=True)
            eager = eager.next_token_logits.float().cpu()
        finally:
            mr.graph_runner = graph_runner
        graph, _ = worker.forward_batch_generation(dec, skip_sample=True)
        hip.append([eager, graph.next_token_logits.float().cpu()])
        common = dict(positions=ops.clamp_position(sb.seq_lens.cpu()), row_mask=row_mask)
        ref32.append(oracle(w32, kv32, "decode", **common))
        ref16.append(oracle(w16, kv16, "decode", **common))

    b32, b16 = bounds(dtype)
    name = {torch.float16: "fp16", torch.bfloat16: "bf16"}[dtype]
    worst = [0.0, 0.0, 0.0]
    for i in range(STEPS + 1):
        scale = float(ref32[i].abs().max())
        dor = float((ref16[i] - ref32[i]).abs().max()) / scale
        for form, h in zip(("eager", "graph"), hip[i]):
            what = f"image prefill bs={bs}" if i == 0 else f"decode step {i} ({form})"
            d32 = float((h - ref32[i]).abs().max()) / scale
            d16 = float((h - ref16[i]).abs().max()) / scale
            worst = [max(worst[0], d32), max(worst[1], d16), max(worst[2], dor)]
            agree = float((h.argmax(-1) == ref32[i].argmax(-1)).float().mean())
            print(f"[parity] mllama real width (2 layers, encoder_len {ENC_LEN}, max|logit| {scale:.2f}) {name} {what}: "
                  f"HIP vs fp32 oracle {d32:.2e}, HIP vs {name} oracle {d16:.2e} (torch-{name} oracle vs fp32 oracle "
                  f"{dor:.2e}); greedy tokens equal on {100 * agree:.0f} % of rows")
            assert d32 <= b32, f"{what}: {d32:.2e} of max|logit| vs the fp32 oracle (bound {b32:.2e})"
            assert d16 <= b16, f"{what}: {d16:.2e} of max|logit| vs the {name} oracle (bound {b16:.2e})"
            assert d32 <= 1.10 * dor + 1e-4, f"{what}: HIP {d32:.2e} vs torch-in-{name} {dor:.2e} from the fp32 oracle"
    print(f"[parity] mllama real width {name} WORST over steps: HIP vs fp32 {worst[0]:.2e}, HIP vs {name} oracle "
          f"{worst[1]:.2e}, torch-{name} vs fp32 {worst[2]:.2e}")
