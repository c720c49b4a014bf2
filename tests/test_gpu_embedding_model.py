"""Embedding requests end to end (ModelRunner -> TpModelWorker.forward_batch_embedding -> the decoder -> one
sp_embedding_pool launch) against what the reference's own LlamaEmbeddingModel and Qwen3ForCausalLM(get_embedding=True)
made of the same ragged prefill of [5, 9, 1] tokens (tests/golden/tiny_embedding.npz).

fp32: the bar tests/test_gpu_qwen3.py holds fp32 logits to (largest deviation over largest magnitude <= 1e-4).
bf16: max |ours - reference bf16| <= 2 d16, d16 = max |reference bf16 - reference fp32| read from the fixture: the
reference's own 16-bit-versus-exact gap is the yardstick, doubled because two valid orders of the same 16-bit sums can
each sit that far from exact.  Bit equality across batches is not claimed (extend attention reorders sums)."""
import contextlib

import pytest
import torch

from tests import embedding_cases as cases

pytestmark = pytest.mark.gpu

MODELS = ["llama", "qwen3"]


def rel(got, want):
    return float((got - want).abs().max() / want.abs().max())


@contextlib.contextmanager
def counted_norms():
    """counts the launches of the two norm entries while it is open: the layers reach them as attributes of _native,
    so a counting stand-in there sees every one of them; the entries are put back on the way out"""
    from scratchpad_amd import _native
    calls = {"rmsnorm": 0, "fused_add_rmsnorm": 0}
    saved = {k: getattr(_native, k) for k in calls}

    def counting(name):
        def call(*args, **kwargs):
            calls[name] += 1
            return saved[name](*args, **kwargs)
        return call

    for k in calls:
        setattr(_native, k, counting(k))
    try:
        yield calls
    finally:
        for k, f in saved.items():
            setattr(_native, k, f)


@pytest.fixture(scope="module")
def runners():
    """one embedding runner per (model, dtype), and the fixture batch's embeddings through the worker"""
    cache = {}

    def get(name, dtype):
        if (name, dtype) not in cache:
            from scratchpad_amd import _native
            from scratchpad_amd.model_runner import TpModelWorker
            mr = cases.make_runner(name, dtype)
            worker = TpModelWorker(mr)
            before = dict(_native.EMBEDDING_CALLS)
            with counted_norms() as norms:
                emb = worker.forward_batch_embedding(cases.fixture_batch(mr, name))
            after = dict(_native.EMBEDDING_CALLS)
            cache[name, dtype] = (mr, worker, emb, (before, after), norms)
        return cache[name, dtype]
    return get


@pytest.mark.parametrize("name", MODELS)
def test_fp32_matches_the_reference_embeddings(name, runners):
    g, pfx, cfg, _ = cases.model_case(name)
    mr, _, emb, _, _ = runners(name, torch.float32)
    assert not mr.is_generation and mr.graph_runner is None
    mr.init_cuda_graphs()
    assert mr.graph_runner is None, "a non-generative runner captures nothing"
    want = torch.from_numpy(g[pfx + "emb_fp32"])
    assert emb.dtype == torch.float32 and emb.shape == want.shape == (3, cfg.hidden_size)
    got = emb.cpu()
    print(f"{name} fp32: relative deviation {rel(got, want):.2e}")
    assert rel(got, want) <= 1e-4
    assert float((got.double().norm(dim=1) - 1).abs().max()) < 1e-6


@pytest.mark.parametrize("name", MODELS)
def test_bf16_within_twice_the_references_own_gap(name, runners):
    g, pfx, cfg, _ = cases.model_case(name)
    _, _, emb, _, _ = runners(name, torch.bfloat16)
    d16 = float(g[pfx + "d16"])
    want = cases.from_bits(g[pfx + "emb_bf16"], torch.bfloat16).float()
    assert emb.dtype == torch.bfloat16
    got = emb.float().cpu()
    dev = float((got - want).abs().max())
    print(f"{name} bf16: max |ours - reference bf16| = {dev:.3e}, d16 = {d16:.3e}")
    assert 0 < d16 < 0.02, "the yardstick itself is a 16-bit rounding, not a broken run"
    assert dev <= 2 * d16
    # unit norm to within one 16-bit unit (2^-8 at 1)
    assert float((got.double().norm(dim=1) - 1).abs().max()) <= 2.0 ** -8


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", MODELS)
def test_the_fused_entry_ran_and_no_all_row_final_norm(name, dtype, runners):
    """two layers: rmsnorm once (the first input_layernorm), fused_add_rmsnorm three times (post-attention twice, the
    second input_layernorm) - the fourth, the final norm over all rows, is inside the one embedding_pool launch"""
    _, _, _, (before, after), norms = runners(name, dtype)
    assert after["fused"] == before["fused"] + 1 and after["gather"] == before["gather"]
    assert norms == {"rmsnorm": 1, "fused_add_rmsnorm": 3}


@pytest.mark.parametrize("name", MODELS)
def test_alone_in_the_batch_and_after_a_prefix_hit(name, runners):
    """the 9-token prompt alone, inside the fixture batch, and resubmitted behind a RadixCache hit on its first 4
    tokens: the same embedding within the 2 d16 bound"""
    from scratchpad_amd.radix_cache import RadixCache
    g, pfx, cfg, _ = cases.model_case(name)
    mr, worker, emb, _, _ = runners(name, torch.bfloat16)
    d16 = float(g[pfx + "d16"])
    ids = torch.from_numpy(g[pfx + "input_ids"])[5:14]
    loc = torch.from_numpy(g[pfx + "out_cache_loc"])[5:14]
    inside = emb[1].float().cpu()
    req = torch.tensor([1], dtype=torch.int64)
    alone = worker.forward_batch_embedding(cases.extend_batch(mr, ids, [9], req, loc, bid=2))[0].float().cpu()
    assert float((alone - inside).abs().max()) <= 2 * d16
    cache = RadixCache(mr.req_to_token_pool, mr.token_to_kv_pool_allocator)
    cache.insert(ids[:4].tolist(), loc[:4].to(mr.device))
    hit, _ = cache.match_prefix(ids.tolist())
    assert hit.tolist() == loc[:4].tolist()
    mr.req_to_token_pool.write((1, slice(0, 4)), hit.to(torch.int32))
    new_loc = torch.arange(91, 96, dtype=torch.int64)
    again = worker.forward_batch_embedding(
        cases.extend_batch(mr, ids[4:], [5], req, new_loc, prefix=[4], bid=3))[0].float().cpu()
    print(f"{name}: alone vs batch {float((alone - inside).abs().max()):.3e}, prefix hit vs batch "
          f"{float((again - inside).abs().max()):.3e}, d16 {d16:.3e}")
    assert float((again - inside).abs().max()) <= 2 * d16
    assert float((again - alone).abs().max()) <= 2 * d16


@pytest.mark.parametrize("name", MODELS)
def test_generation_is_untouched_by_an_embedding_batch(name):
    """a generation batch gives the logits it gave before an embedding batch ran on the same runner"""
    from scratchpad_amd.forward_info import ForwardBatch
    from scratchpad_amd.model_runner import TpModelWorker
    mr = cases.make_runner(name, torch.bfloat16, generation=True)
    assert mr.is_generation
    worker = TpModelWorker(mr)
    with counted_norms() as norms:
        first, _ = worker.forward_batch_generation(cases.fixture_batch(mr, name))
    assert norms["fused_add_rmsnorm"] == 4, "generation norms all rows"
    first = first.next_token_logits.clone()
    fb = ForwardBatch.init_new(cases.fixture_batch(mr, name), mr)
    mr.attn_backend.init_forward_metadata(fb)
    emb = mr.model.forward(fb.input_ids, fb.positions, fb, get_embedding=True).embeddings
    assert emb.shape == (3, mr.model_config.hidden_size)
    assert float((emb.float().norm(dim=1) - 1).abs().max()) <= 2.0 ** -8
    second, _ = worker.forward_batch_generation(cases.fixture_batch(mr, name))
    assert torch.equal(second.next_token_logits, first)
    with pytest.raises(ValueError, match="generative runner"):
        worker.forward_batch_embedding(cases.fixture_batch(mr, name))


def test_refusals_on_the_device():
    from scratchpad_amd.forward_info import ForwardMode, ModelWorkerBatch
    from scratchpad_amd.model_runner import TpModelWorker
    mr = cases.make_runner("llama", torch.bfloat16)
    worker = TpModelWorker(mr)
    batch = cases.fixture_batch(mr, "llama")
    batch.return_logprob = True
    with pytest.raises(NotImplementedError, match="return_logprob"):
        worker.forward_batch_embedding(batch)
    dev = mr.device
    dec = ModelWorkerBatch(bid=9, forward_mode=ForwardMode.DECODE, input_ids=torch.zeros(1, dtype=torch.int64, device=dev),
                           req_pool_indices=torch.zeros(1, dtype=torch.int64, device=dev),
                           seq_lens=torch.full((1,), 2, dtype=torch.int64, device=dev),
                           out_cache_loc=torch.ones(1, dtype=torch.int64, device=dev), seq_lens_sum=2)
    with pytest.raises(ValueError, match="non-generative"):
        worker.forward_batch_embedding(dec)
    with pytest.raises(ValueError, match="non-generative"):
        mr.sample(None, None)
