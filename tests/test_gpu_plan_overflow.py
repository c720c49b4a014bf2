"""An understated ``seq_lens_sum`` costs load balance, never a split.

The decode split plan and its partial workspace are sized from the HOST's bound on sum(seq_lens)
(``ForwardBatch.seq_lens_sum``; the reference's producer is ScheduleBatch.prepare_for_decode,
scheduler/schedule_batch.py:1230-1308, which keeps it equal to the device-side lengths).  Where a caller breaks that
contract the plan kernel, which reads the device-side lengths, doubles the split size until every (request, split)
item fits the slots the launch covers (ABI 10): the step lists every item, its logits are those of the honest step up
to the rounding of another split size, and nothing has to be reported."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _runner(items=True):
    """items=True: the backend plans the (request, split) items as it does for a model with a soft-cap layer or a shape
    the range kernel refuses, and its launches are sent to them (sp_debug_set("decode_ranges", 0) in the tests below) -
    the geometry whose slots the host's bound sizes.  items=False: the backend as it is built for Llama (round 6): plans
    are the range section alone."""
    from scratchpad_amd.model_runner import ModelConfig, ModelRunner, ServerArgs
    cfg = ModelConfig(256, 512, 2, 4, 2, 512, context_len=2048, max_position_embeddings=2048)
    args = ServerArgs(max_total_tokens=4096, max_running_requests=8, disable_cuda_graph=True)
    mr = ModelRunner(cfg, args, dtype=torch.bfloat16, seed=5)
    assert mr.attn_backend.decode_ranges > 0 and mr.attn_backend.plan_items is False, "a Llama shape plans no items"
    mr.attn_backend.plan_items = items
    return mr


@pytest.fixture
def item_geometry():
    from scratchpad_amd import _native
    _native.debug_set("decode_ranges", 0)
    yield
    _native.debug_set("decode_ranges", -1)


def _decode_batch(mr, lens, claimed_sum):
    from scratchpad_amd.forward_info import ForwardMode, ModelWorkerBatch
    dev = mr.device
    bs = len(lens)
    table = mr.req_to_token_pool.req_to_token
    g = torch.Generator().manual_seed(1)
    perm = (torch.randperm(4000, generator=g) + 1).to(torch.int32)
    off, loc = 0, []
    for b, n in enumerate(lens):
        table[b, :n] = perm[off:off + n].to(dev)
        loc.append(int(perm[off + n - 1]))
        off += n
    return ModelWorkerBatch(bid=1, forward_mode=ForwardMode.DECODE,
                            input_ids=torch.randint(0, 512, (bs,), generator=g).to(dev),
                            req_pool_indices=torch.arange(bs, device=dev), seq_lens=torch.tensor(lens, device=dev),
                            out_cache_loc=torch.tensor(loc, device=dev), seq_lens_sum=claimed_sum)


def _self_plan(mr):
    """(words 0..3 of the step's self-attention plan, the item slots its launches cover)"""
    plan, slots, _, _ = mr.attn_backend.forward_metadata[3][0]
    return plan[:4].tolist(), slots


def _close(got, want):
    """the bar of another split size (tests/test_gpu_llama.py: graph replay against eager, bf16)"""
    return torch.allclose(got, want, atol=1e-2 * float(want.abs().max()))


LENS = [600, 600, 600, 600]
UNDERSTATED = 400          # 400 // 64 + 4 = 10 slots; the lengths need 40 items at chunk 64, 8 at chunk 512


def test_understated_seq_lens_sum_grows_the_split_size(item_geometry):
    from scratchpad_amd import _native
    from scratchpad_amd.model_runner import TpModelWorker
    mr = _runner()
    worker = TpModelWorker(mr)
    honest, _ = worker.forward_batch_generation(_decode_batch(mr, LENS, sum(LENS)))
    honest = honest.next_token_logits.clone()
    (listed, chunk, needed, _), slots = _self_plan(mr)
    assert chunk == 64 and listed == needed == 40 <= slots, "the honest step keeps the host's split size"
    bad, _ = worker.forward_batch_generation(_decode_batch(mr, LENS, UNDERSTATED))
    assert _native.debug_get("decode_last_kernel") in (1, 2), "the (request, split) items ran"
    (listed, chunk, needed, _), slots = _self_plan(mr)
    assert slots == 10 and chunk == 512 and listed == needed == 8, "every item listed at a grown split size"
    assert _close(bad.next_token_logits, honest)
    # the honest step again: the same bits
    again, _ = worker.forward_batch_generation(_decode_batch(mr, LENS, sum(LENS)))
    assert torch.equal(again.next_token_logits, honest)


def _synchronous(mr):
    """claimed sum -> (token ids, logits) of the synchronous worker for LENS"""
    from scratchpad_amd.model_runner import TpModelWorker
    worker = TpModelWorker(mr)
    out = {}
    for claimed in (sum(LENS), UNDERSTATED):
        logits, ids = worker.forward_batch_generation(_decode_batch(mr, LENS, claimed))
        out[claimed] = (ids.tolist(), logits.next_token_logits.cpu())
    assert _close(out[UNDERSTATED][1], out[sum(LENS)][1])
    return out


def _check_resolved(client, want):
    logits, ids = client.resolve_last_batch_result()
    assert ids == want[0], "the synchronous worker's token ids"
    assert torch.equal(logits.next_token_logits.cpu(), want[1]), "the synchronous worker's logits"


def test_overlap_worker_gives_the_synchronous_results_for_understated_steps(item_geometry):
    """The overlap worker (tp_worker_client.py) runs an understated step like any other: the ids and logits it resolves
    are those of the synchronous worker given the same batches, and the engine goes on."""
    from scratchpad_amd.tp_worker_client import TpModelWorkerClient
    mr = _runner()
    want = _synchronous(mr)
    client = TpModelWorkerClient(mr)
    try:
        for claimed in (sum(LENS), UNDERSTATED, sum(LENS)):
            client.forward_batch_generation(_decode_batch(mr, LENS, claimed))
            _check_resolved(client, want[claimed])
        assert client.forward_thread.is_alive() and client.error is None
    finally:
        client.close()


def test_overlap_worker_keeps_going_when_step_n_plus_1_is_enqueued_first(item_geometry):
    """under real overlap scheduling step N + 1 is enqueued BEFORE step N is resolved.  An understated step
    in that window resolves to the synchronous worker's results, as do the honest steps around it, and the forward
    thread stays alive."""
    from scratchpad_amd.tp_worker_client import TpModelWorkerClient
    mr = _runner()
    want = _synchronous(mr)
    honest, bad = want[sum(LENS)], want[UNDERSTATED]
    client = TpModelWorkerClient(mr)
    try:
        good = lambda: _decode_batch(mr, LENS, sum(LENS))
        client.forward_batch_generation(good())                               # step 1
        client.forward_batch_generation(_decode_batch(mr, LENS, UNDERSTATED))  # step 2: enqueued before 1 resolves
        _check_resolved(client, honest)                                       # step 1
        client.forward_batch_generation(good())                               # step 3 enqueued before 2 resolves
        torch.cuda.synchronize()
        _check_resolved(client, bad)                                          # step 2
        client.forward_batch_generation(good())                               # step 4
        _check_resolved(client, honest)                                       # step 3
        _check_resolved(client, honest)                                       # step 4
        assert client.forward_thread.is_alive() and client.error is None
    finally:
        client.close()


def test_range_plans_do_not_size_anything_from_the_hosts_sum():
    """The backend as it is built for Llama / Mllama since round 6: plans carry the range section alone, whose slots
    (batch size + pieces) and cuts come from the device-side lengths.  A seq_lens_sum understated so far that the item
    geometry would need another split size (2000 claimed for 4 x 600: 35 slots for 40 items at chunk 64) changes NOTHING
    here: the same bits as the honest step.  Nor does a sum below the
    longest request (400 claimed for 4 x 600): the bound every length is clamped to (max_len) is the context length in an
    eager step without seq_lens_cpu, as under graph replay - it was min(context, sum - (bs - 1)) = 397 until the clamp
    silently cut every request to 397 keys."""
    from scratchpad_amd import _native
    from scratchpad_amd.model_runner import TpModelWorker
    mr = _runner(items=False)
    worker = TpModelWorker(mr)
    lens = [600, 600, 600, 600]
    honest, _ = worker.forward_batch_generation(_decode_batch(mr, lens, sum(lens)))
    assert _native.debug_get("decode_last_kernel") == 3, "the range kernel ran"
    honest = honest.next_token_logits.clone()
    assert _native.decode_plan_slots(4, 1997, 64, 2000) < 4 * 10, "the item geometry would have grown its split size"
    for claimed in (2000, 400):
        bad, _ = worker.forward_batch_generation(_decode_batch(mr, lens, claimed))
        assert _native.debug_get("decode_last_kernel") == 3
        assert mr.attn_backend.forward_metadata[1] >= max(lens), f"claimed {claimed}: max_len below the longest request"
        assert torch.equal(bad.next_token_logits, honest), f"claimed {claimed}: other logits than the honest step"


def test_item_geometry_never_returns_a_cut_request_silently(item_geometry):
    """lens [1000, 1, 1, 1] claimed as 500 in the (request, split) item geometry.  While max_len was derived from the
    sum (min(context, 500 - 3) = 497) the plan counted its items from the CLAMPED lengths - 8 + 3 = 11, exactly the 11
    slots 500 // 64 + 4 sizes - so nothing overflowed, nothing was reported and request 0 attended to 497 of its 1000
    keys.  Now the 19 items of chunk 64 become the 11 of chunk 128: every key is attended to, and the logits are the
    honest step's up to the rounding of that split size."""
    from scratchpad_amd.model_runner import TpModelWorker
    mr = _runner()
    worker = TpModelWorker(mr)
    lens = [1000, 1, 1, 1]
    honest, _ = worker.forward_batch_generation(_decode_batch(mr, lens, sum(lens)))
    honest = honest.next_token_logits.clone()
    assert _self_plan(mr)[0][:3] == [19, 64, 19]
    bad, _ = worker.forward_batch_generation(_decode_batch(mr, lens, 500))
    (listed, chunk, needed, keys), slots = _self_plan(mr)
    assert slots == 11 and chunk == 128 and listed == needed == 11 and keys == sum(lens)
    assert _close(bad.next_token_logits, honest)
    # the engine goes on: the honest step again, the same bits
    again, _ = worker.forward_batch_generation(_decode_batch(mr, lens, sum(lens)))
    assert torch.equal(again.next_token_logits, honest)


def test_cross_attention_window_without_encoder_lens_cpu():
    """An encoder-decoder decode step whose ForwardBatch carries encoder_lens but not encoder_lens_cpu: the cross
    window (up to 200 encoder keys here, behind text of <= 9 tokens) must not be clamped to the text's bound.  Checked
    at the backend seam, layer by layer (the Mllama model itself reads encoder_lens_cpu for its row mask): the cross and
    the self launch give the bits of the step that has the host copy, with and without seq_lens_cpu; a text-only request
    (encoder_len 0) reads as zeros."""
    from scratchpad_amd.attention import RadixAttention
    from scratchpad_amd.forward_info import ForwardBatch, ForwardMode
    from scratchpad_amd.model_runner import ModelConfig, ModelRunner, ServerArgs
    cfg = ModelConfig(256, 512, 2, 4, 2, 512, context_len=256, max_position_embeddings=512, cross_attention_layers=[1])
    mr = ModelRunner(cfg, ServerArgs(max_total_tokens=1024, max_running_requests=4, disable_cuda_graph=True),
                     dtype=torch.bfloat16, seed=5)
    be = mr.attn_backend
    assert be.is_encoder_decoder and be.decode_ranges > 0 and be.plan_items is False
    dev = mr.device
    g = torch.Generator(device=dev).manual_seed(7)
    for arena in (mr.token_to_kv_pool._k_arena, mr.token_to_kv_pool._v_arena):
        arena.normal_(0.0, 1.0, generator=g)
    enc, text = [200, 0, 150], [5, 9, 3]
    table = mr.req_to_token_pool.req_to_token
    perm = (torch.randperm(1000, generator=torch.Generator().manual_seed(8)) + 1).to(torch.int32).to(dev)
    off = 0
    for b, (e, t) in enumerate(zip(enc, text)):
        table[b, :e + t] = perm[off:off + e + t]
        off += e + t
    cross = next(m for m in mr.model.modules() if isinstance(m, RadixAttention) and m.is_cross_attention)
    selfa = next(m for m in mr.model.modules() if isinstance(m, RadixAttention) and not m.is_cross_attention)
    q = torch.randn(3, 4 * 64, device=dev, generator=g).to(torch.bfloat16)

    def step(enc_cpu, seq_cpu):
        fb = ForwardBatch(forward_mode=ForwardMode.DECODE, batch_size=3, input_ids=torch.zeros(3, dtype=torch.int64, device=dev),
                          req_pool_indices=torch.arange(3, device=dev), seq_lens=torch.tensor(text, device=dev),
                          out_cache_loc=torch.zeros(3, dtype=torch.int64, device=dev), seq_lens_sum=sum(text),
                          seq_lens_cpu=torch.tensor(text) if seq_cpu else None,
                          encoder_lens=torch.tensor(enc, device=dev), encoder_lens_cpu=list(enc) if enc_cpu else None,
                          req_to_token_pool=mr.req_to_token_pool, token_to_kv_pool=mr.token_to_kv_pool, attn_backend=be)
        be.init_forward_metadata(fb)
        assert be.forward_metadata[1] >= max(enc), "max_len below the longest encoder window"
        return [be.forward_decode(q.clone(), None, None, layer, fb, save_kv_cache=False).clone() for layer in (cross, selfa)]

    honest = step(True, True)
    assert torch.all(honest[0][1] == 0), "a text-only request's cross-attention row reads as zeros"
    assert not torch.equal(honest[0][0], honest[0][2])
    for seq_cpu in (True, False):
        got = step(False, seq_cpu)
        for what, a, b in zip(("cross", "self"), got, honest):
            assert torch.equal(a, b), f"{what} launch without encoder_lens_cpu (seq_lens_cpu: {seq_cpu}): other bits"
