"""sp_logprobs on the GPU against the float64 oracle of tests/logprob_oracle.py, and the two callers it serves:
Sampler.forward (device path against SP_DEVICE_LOGPROBS=0 in one process) and LogitsProcessor's prompt logprobs in
chunks (the reference's own outputs of tests/golden/input_logprobs.npz, peak memory, a model step).

Tolerances: values atol 1e-5, what the project already holds its logprobs to (tests/test_gpu_sampling_rows.py);
top-k ids equal to the oracle's (value descending, id ascending) order on every row; two paths against each other 2e-5."""
import math

import numpy as np
import pytest
import torch

from tests import logprob_oracle as lpo

pytestmark = pytest.mark.gpu
ATOL = 1e-5
POOL = 12          # distinct rows per case: larger batches repeat them under different requests


def _close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), what
    err = np.abs(got[~inf] - want[~inf])
    assert err.size == 0 or float(err.max()) <= ATOL, f"{what}: off by {float(err.max()):.3e}"
    return float(err.max()) if err.size else 0.0


@pytest.mark.parametrize("rows", [1, 8, 256])
@pytest.mark.parametrize("vocab", [4096, 32000, 50257, 128256])
@pytest.mark.parametrize("kind", [0, 1])
def test_kernel_against_float64_oracle(kind, vocab, rows):
    from scratchpad_amd import _native
    npool = min(rows, POOL)
    if kind == 0:
        pool, pool_ps = lpo.logit_rows(vocab, npool, rows), None
    else:
        pool, pool_ps = lpo.prob_rows(vocab, npool, rows)
    if vocab >= 32000 and npool >= 8:
        # the rows are tie-heavy where it matters: inside the top 20
        assert sum(not lpo.distinct_top(pool[i], 20) for i in range(npool)) >= 6
    vals = lpo.all_values(pool, kind, pool_ps)
    order = [lpo.top_order(pool[i], 20) for i in range(npool)]
    src = np.arange(rows) % npool
    chosen, top_ks, id_lists = lpo.requests(vocab, rows, kind)
    # strided rows (an odd stride: most rows start off a 16-byte boundary) with poisoned padding
    pad = 7
    wide = torch.full((rows, vocab + pad), 7e37, dtype=torch.float32)
    wide[:, :vocab] = torch.from_numpy(pool[src])
    wide = wide.cuda()
    before = wide.clone()
    before_launches = _native.LOGPROB_LAUNCHES["logprobs"]
    res = _native.logprobs(wide[:, :vocab], kind, torch.from_numpy(chosen).cuda(), top_ks, id_lists,
                           top_ps=None if pool_ps is None else torch.from_numpy(pool_ps[src]).cuda())
    top_val, top_idx, ids_val = res.lists()
    got_chosen = res.chosen.cpu().numpy()
    assert _native.LOGPROB_LAUNCHES["logprobs"] == before_launches + 1
    assert torch.equal(wide, before), "rows and their padding are read only"
    worst = _close(got_chosen, vals[src, chosen], "chosen")
    for b in range(rows):
        i, k = src[b], top_ks[b]
        assert top_idx[b] == order[i][:k].tolist(), f"row {b}: top-{k} ids"
        worst = max(worst, _close(top_val[b], vals[i, order[i][:k]], f"row {b} top values"))
        want = vals[i, id_lists[b]] if id_lists[b] else np.zeros(0)
        worst = max(worst, _close(ids_val[b], want, f"row {b} listed ids"))
    if kind == 1:
        flat = np.concatenate([np.asarray(v) for v in ids_val] + [got_chosen])
        assert np.isfinite(flat).all()
        if rows >= 8:
            assert (flat == lpo.FLOOR).any(), "some asked token is dropped by top_p 0.3 / 0.9 and reports finfo.min"
    print(f"kind {kind} vocab {vocab} rows {rows}: worst error {worst:.3e}")


def test_kernel_parts_are_optional_and_ids_outside_the_vocabulary_report_the_floor():
    from scratchpad_amd import _native
    vocab = 5000
    x = lpo.logit_rows(vocab, 4)
    vals = lpo.all_values(x, 0)
    dev = torch.from_numpy(x).cuda()
    bad = torch.tensor([-1, vocab, 1 << 40, 17], dtype=torch.int64)
    res = _native.logprobs(dev, 0, bad.cuda(), None, [[vocab, -5, 3], None, [2 ** 31], []])
    tv, ti, iv = res.lists()
    assert tv == [[]] * 4 and ti == [[]] * 4
    c = res.chosen.cpu().numpy()
    assert c[:3].tolist() == [lpo.FLOOR] * 3 and abs(c[3] - vals[3, 17]) <= ATOL
    assert iv[0][:2] == [lpo.FLOOR] * 2 and abs(iv[0][2] - vals[0, 3]) <= ATOL and iv[2] == [lpo.FLOOR]
    assert iv[1] == [] and iv[3] == []
    # nothing chosen, only a top list; probabilities without top_ps keep everything
    p, _ = lpo.prob_rows(vocab, 4)
    res = _native.logprobs(torch.from_numpy(p).cuda(), 1, None, [3, 0, 20, 1], None)
    assert res.chosen is None
    tv, ti, iv = res.lists()
    want = lpo.all_values(p, 1, None)
    for b, k in enumerate([3, 0, 20, 1]):
        order = lpo.top_order(p[b], k)
        assert ti[b] == order.tolist()
        _close(tv[b], want[b, order], f"row {b}")
    with pytest.raises(RuntimeError):
        _native.logprobs(torch.from_numpy(x), 0, None, [1] * 4, None)           # host tensor
    with pytest.raises(RuntimeError):
        _native.logprobs(dev, 0, None, [_native.LOGPROBS_MAX_TOP_K + 1] * 4, None)


# --------------------------------------------------------------------------- Sampler.forward, switch on and off
def _sampler_run(monkeypatch, switch, logits, info, nums, asked, uniform):
    from scratchpad_amd import _native
    from scratchpad_amd.llama import LogitsProcessorOutput
    from scratchpad_amd.sampler import Sampler
    monkeypatch.setenv("SP_DEVICE_LOGPROBS", switch)
    out = LogitsProcessorOutput(next_token_logits=logits.clone().cuda())
    before = _native.LOGPROB_LAUNCHES["logprobs"]
    ids = Sampler()(out, info, return_logprob=True, top_logprobs_nums=nums, token_ids_logprobs=asked,
                    uniform=None if uniform is None else uniform.cuda())
    return out, ids.cpu(), _native.LOGPROB_LAUNCHES["logprobs"] - before


@pytest.mark.parametrize("greedy", [True, False], ids=["greedy", "sampling"])
@pytest.mark.parametrize("vocab,reps", [(32000, 1), (128256, 1), (32000, 32)], ids=["v32000_bs8", "v128256_bs8", "v32000_bs256"])
def test_sampler_forward_device_path_against_the_torch_path(monkeypatch, vocab, reps, greedy):
    """bs 8: a row is cut into slices over several workgroups; bs 256: one workgroup per row."""
    from scratchpad_amd import _native
    from scratchpad_amd.llama import LogitsProcessorOutput
    from scratchpad_amd.sampler import Sampler, SamplingBatchInfo, SamplingParams
    gen = torch.Generator().manual_seed(vocab + greedy + reps)
    if greedy:
        params = [SamplingParams(temperature=0.0)] * 8
    else:
        params = [SamplingParams(temperature=0.8, top_p=0.9, top_k=50), SamplingParams(temperature=1.2),
                  SamplingParams(temperature=0.0), SamplingParams(temperature=1.0, min_p=0.1, top_p=0.5),
                  SamplingParams(temperature=0.5, top_k=5, top_p=0.5), SamplingParams(temperature=2.0, top_p=0.3),
                  SamplingParams(temperature=0.3, top_p=0.95), SamplingParams(temperature=1.0, top_p=0.999, top_k=3)]
    params = params * reps
    bs = len(params)
    logits = (torch.randn(bs, vocab, generator=gen) * 3).to(torch.bfloat16).float()
    info = SamplingBatchInfo.from_params(params, vocab, "cuda")
    assert info.is_all_greedy == greedy
    u = None if greedy else torch.rand(bs, generator=gen)
    nums = [0, 1, 5, 20, 3, 2, 7, 4] * reps
    asked = [None, [0, 1, vocab - 1], None, [5], list(range(40, 60)), None, [vocab // 2], [3, 2, 1]] * reps
    dev, dev_ids, dev_launches = _sampler_run(monkeypatch, "1", logits, info, nums, asked, u)
    ref, ref_ids, ref_launches = _sampler_run(monkeypatch, "0", logits, info, nums, asked, u)
    assert dev_launches == 1 and ref_launches == 0, "the device path launches sp_logprobs once, the torch path never"
    assert torch.equal(dev_ids, ref_ids)
    assert torch.equal(dev.next_token_logits, ref.next_token_logits)       # the in-place softmax (or the logits)
    assert dev.next_token_token_ids_logprobs_idx == ref.next_token_token_ids_logprobs_idx == [a or [] for a in asked]
    both = lambda a, b: np.allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=0, atol=2e-5)
    assert both(dev.next_token_logprobs.cpu(), ref.next_token_logprobs.cpu())
    seen = dev.next_token_logits.cpu().numpy()
    want = lpo.all_values(seen, 0 if greedy else 1, None if greedy else info.top_ps.cpu().numpy())
    compared = 0
    for b in range(bs):
        assert len(dev.next_token_top_logprobs_val[b]) == nums[b]
        assert both(dev.next_token_top_logprobs_val[b], ref.next_token_top_logprobs_val[b]), b
        assert both(dev.next_token_token_ids_logprobs_val[b], ref.next_token_token_ids_logprobs_val[b]), b
        _close(dev.next_token_top_logprobs_val[b], want[b, dev.next_token_top_logprobs_idx[b]], f"row {b}")
        # ids are compared where the oracle's top-(k + 1) logprobs are distinct: no tie rule is involved there
        if np.unique(np.sort(want[b])[::-1][:nums[b] + 1]).size == nums[b] + 1:
            compared += nums[b] > 0
            assert dev.next_token_top_logprobs_idx[b] == ref.next_token_top_logprobs_idx[b], b
        assert dev.next_token_top_logprobs_idx[b] == lpo.top_order(seen[b], nums[b]).tolist(), b
    assert compared >= 1
    # a batch that asks for no logprobs launches nothing new
    before = _native.LOGPROB_LAUNCHES["logprobs"]
    out = LogitsProcessorOutput(next_token_logits=logits.clone().cuda())
    ids = Sampler()(out, info, uniform=None if u is None else u.cuda())
    assert _native.LOGPROB_LAUNCHES["logprobs"] == before and torch.equal(ids.cpu(), dev_ids)


def test_top_k_above_the_cap_takes_the_torch_path():
    from scratchpad_amd import _native
    from scratchpad_amd.llama import LogitsProcessorOutput
    from scratchpad_amd.sampler import Sampler, SamplingBatchInfo, SamplingParams
    vocab, k = 32000, _native.LOGPROBS_MAX_TOP_K + 8
    x = lpo.logit_rows(vocab, 1, "cap")
    x = np.concatenate([x, (np.random.default_rng(0).permutation(vocab).astype(np.float32) / 997)[None]])
    info = SamplingBatchInfo.from_params([SamplingParams(temperature=0.0)] * 2, vocab, "cuda")
    out = LogitsProcessorOutput(next_token_logits=torch.from_numpy(x).cuda())
    before = _native.LOGPROB_LAUNCHES["logprobs"]
    ids = Sampler()(out, info, return_logprob=True, top_logprobs_nums=[2, k], token_ids_logprobs=[[7], None])
    assert _native.LOGPROB_LAUNCHES["logprobs"] == before
    want = lpo.all_values(x, 0)
    assert ids.tolist() == [int(x[0].argmax()), int(x[1].argmax())]
    _close(out.next_token_logprobs.cpu().numpy(), want[np.arange(2), ids.cpu().numpy()], "chosen")
    assert [len(v) for v in out.next_token_top_logprobs_val] == [2, k]
    assert out.next_token_top_logprobs_idx[1] == lpo.top_order(x[1], k).tolist()         # row 1 has no ties
    _close(out.next_token_top_logprobs_val[1], want[1, lpo.top_order(x[1], k)], "row 1")
    _close(out.next_token_top_logprobs_val[0], np.sort(want[0])[::-1][:2], "row 0")
    _close(out.next_token_token_ids_logprobs_val[0], want[0, [7]], "listed")


# --------------------------------------------------------------------------- prompt logprobs in chunks
def _fixture_batch(g, c, dev):
    from types import SimpleNamespace
    from scratchpad_amd.forward_info import ForwardBatch, ForwardMode
    nreq = len(c["spec"])
    ext = c["extend_lens"].tolist()
    fb = ForwardBatch(forward_mode=ForwardMode.EXTEND, batch_size=nreq, input_ids=None, req_pool_indices=None,
                      seq_lens=None, out_cache_loc=None, seq_lens_sum=0)
    fb.extend_seq_lens = torch.tensor(ext, dtype=torch.int32, device=dev)
    fb.extend_seq_lens_cpu = ext
    fb.return_logprob = True
    fb.top_logprobs_nums = c["spec"][:, 4].tolist()
    fb.token_ids_logprobs = [c[f"r{i}_ids"].tolist() if bool(c["has_ids"][i]) else None for i in range(nreq)]
    fb.extend_logprob_start_lens_cpu = c["extend_logprob_start_lens"].tolist()
    fb.extend_input_logprob_token_ids_gpu = torch.from_numpy(c["extend_input_logprob_token_ids"]).to(dev)
    return fb, SimpleNamespace(weight=torch.from_numpy(g["head"]).to(dev))


def test_chunked_prompt_logprobs_equal_the_reference_outputs(monkeypatch):
    from types import SimpleNamespace
    from scratchpad_amd import _native, distributed
    from scratchpad_amd.llama import LogitsProcessor
    from tests.test_input_logprobs import _cases, _check_output
    distributed.initialize_model_parallel(1)
    dev = torch.device("cuda:0")
    inside = at_request = 0
    for ci, g, c in _cases():
        if not bool(c["has_input"]):
            continue
        ext, st = c["extend_lens"].tolist(), c["extend_logprob_start_lens"].tolist()
        spans, _, _, _ = LogitsProcessor.input_logprob_plan(ext, st)
        kept = sum(b - a for a, b in spans)
        starts = set(np.cumsum([b - a for a, b in spans])[:-1].tolist())       # kept rows where a request begins
        for chunk in (1, 3, kept + 5):
            cuts = set(range(chunk, kept, chunk))
            inside += len(cuts - starts)
            at_request += len(cuts & starts)
            monkeypatch.setenv("SP_LOGPROB_CHUNK_ROWS", str(chunk))
            fb, head = _fixture_batch(g, c, dev)
            proc = LogitsProcessor(SimpleNamespace(vocab_size=int(g["vocab"])))
            before = _native.LOGPROB_LAUNCHES["logprobs"]
            res = proc(None, torch.from_numpy(c["hidden"]).to(dev), head, fb)
            assert _native.LOGPROB_LAUNCHES["logprobs"] - before == math.ceil(kept / chunk)
            _check_output(res, c, len(c["spec"]), 5e-5, f"case {ci} in chunks of {chunk}")
    assert inside > 0 and at_request > 0, "a chunk boundary inside a request and one at a request boundary both occur"


def test_chunked_prompt_logprobs_with_temperature_scaling(monkeypatch):
    """temp_scaled_logprobs (logits_processor.py:292-301, 441-442) through the chunk loop: the input logprobs see
    their request's temperature, the sampled logits do not.  Against float64 of the fixture's hidden states and head
    at the fixture's 5e-5, and against the dense path (SP_DEVICE_LOGPROBS=0) on the same batch."""
    from types import SimpleNamespace
    from scratchpad_amd import _native, distributed
    from scratchpad_amd.llama import LogitsProcessor
    from tests.test_input_logprobs import _cases
    distributed.initialize_model_parallel(1)
    dev = torch.device("cuda:0")
    ran = 0
    for ci, g, c in _cases():
        if not bool(c["has_input"]):
            continue
        nreq, vocab = len(c["spec"]), int(g["vocab"])
        temps = torch.tensor([0.5, 1.7, 0.9, 1.3, 2.0, 0.7][:nreq] + [1.1] * max(nreq - 6, 0), dtype=torch.float32)
        ext, st = c["extend_lens"].tolist(), c["extend_logprob_start_lens"].tolist()
        spans, sample_idx, input_idx, pruned_lens = LogitsProcessor.input_logprob_plan(ext, st)
        kept = torch.cat([torch.from_numpy(c["hidden"])[a:b] for a, b in spans]).double()
        logits64 = (kept @ torch.from_numpy(g["head"]).double().T)[:, :vocab]
        row_t = torch.cat([temps[i].repeat(b - a) for i, (a, b) in enumerate(spans)]).double().view(-1, 1)
        lp64 = torch.log_softmax(logits64 / row_t, dim=-1)[input_idx]
        want = lp64[torch.arange(len(input_idx)), torch.from_numpy(c["extend_input_logprob_token_ids"]).long()]
        results = {}
        for switch, chunk in (("1", 3), ("0", 3)):
            monkeypatch.setenv("SP_DEVICE_LOGPROBS", switch)
            monkeypatch.setenv("SP_LOGPROB_CHUNK_ROWS", str(chunk))
            fb, head = _fixture_batch(g, c, dev)
            fb.temp_scaled_logprobs = True
            fb.sampling_info = SimpleNamespace(temperatures=temps.view(-1, 1).to(dev), top_ps=torch.ones(nreq, device=dev))
            before = _native.LOGPROB_LAUNCHES["logprobs"]
            results[switch] = LogitsProcessor(SimpleNamespace(vocab_size=vocab))(
                None, torch.from_numpy(c["hidden"]).to(dev), head, fb)
            assert (_native.LOGPROB_LAUNCHES["logprobs"] > before) == (switch == "1")
        on, off = results["1"], results["0"]
        assert torch.allclose(on.input_token_logprobs.cpu().double(), want, atol=5e-5), f"case {ci}"
        assert torch.allclose(on.input_token_logprobs, off.input_token_logprobs, atol=5e-5)
        # the sampled logits are not scaled
        assert torch.allclose(on.next_token_logits.cpu(), torch.from_numpy(c["next_token_logits"]), atol=5e-5)
        assert torch.allclose(on.next_token_logits.cpu().double(), logits64[sample_idx], atol=5e-5)
        for field in ("input_top_logprobs_val", "input_token_ids_logprobs_val"):
            a, b = getattr(on, field), getattr(off, field)
            assert (a is None) == (b is None)
            for ra, rb in zip(a or [], b or []):
                assert len(ra) == len(rb)
                for x, y in zip(ra, rb):
                    assert np.allclose(np.asarray(x, np.float64), np.asarray(y, np.float64), atol=5e-5), (ci, field)
        ran += 1
    assert ran >= 1


def test_chunked_prompt_logprobs_bound_the_peak_memory(monkeypatch):
    """4096 kept rows x vocab 32 000 behind an fp16 head, in chunks of 512: the chunk is one eighth of the rows, and a
    factor two is left for the GEMM output in the model dtype and the allocator's rounding."""
    from types import SimpleNamespace
    from scratchpad_amd import distributed
    from scratchpad_amd.forward_info import ForwardBatch, ForwardMode
    from scratchpad_amd.llama import LogitsProcessor
    distributed.initialize_model_parallel(1)
    dev = torch.device("cuda:0")
    rows, hidden, vocab = 4096, 256, 32000
    gen = torch.Generator().manual_seed(11)
    head = SimpleNamespace(weight=(torch.randn(vocab, hidden, generator=gen) * 0.05).half().to(dev))
    states = torch.randn(rows, hidden, generator=gen).half().to(dev)
    tokens = torch.randint(0, vocab, (rows,), generator=gen).to(dev)
    monkeypatch.setenv("SP_LOGPROB_CHUNK_ROWS", "512")

    def run(switch):
        monkeypatch.setenv("SP_DEVICE_LOGPROBS", switch)
        fb = ForwardBatch(forward_mode=ForwardMode.EXTEND, batch_size=1, input_ids=None, req_pool_indices=None,
                          seq_lens=None, out_cache_loc=None, seq_lens_sum=0)
        fb.extend_seq_lens = torch.tensor([rows], dtype=torch.int32, device=dev)
        fb.extend_seq_lens_cpu = [rows]
        fb.return_logprob = True
        fb.top_logprobs_nums = [5]
        fb.token_ids_logprobs = [None]
        fb.extend_logprob_start_lens_cpu = [0]
        fb.extend_input_logprob_token_ids_gpu = tokens
        proc = LogitsProcessor(SimpleNamespace(vocab_size=vocab))
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        res = proc(None, states, head, fb)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, res

    peak_dev, res_dev = run("1")
    peak_ref, res_ref = run("0")
    print(f"peak memory over the LogitsProcessor call: device path {peak_dev / 2 ** 20:.1f} MiB, "
          f"torch path {peak_ref / 2 ** 20:.1f} MiB")
    assert peak_dev * 4 <= peak_ref
    assert torch.allclose(res_dev.input_token_logprobs, res_ref.input_token_logprobs, atol=2e-2)
    assert np.allclose(res_dev.input_top_logprobs_val[0], res_ref.input_top_logprobs_val[0], atol=2e-2)
    assert torch.allclose(res_dev.next_token_logits, res_ref.next_token_logits, atol=2e-2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_model_step_with_input_logprobs_in_small_chunks(monkeypatch, dtype):
    """the scenario of tests/test_input_logprobs.py's model step - 9 + 4 + 1 kept rows - in chunks of 4 rows, held to
    that test's own oracle and tolerances"""
    from scratchpad_amd import _native
    from tests.test_input_logprobs import test_model_step_with_input_logprobs_against_oracle as scenario
    monkeypatch.setenv("SP_LOGPROB_CHUNK_ROWS", "4")
    before = _native.LOGPROB_LAUNCHES["logprobs"]
    scenario(dtype)
    # the chunks of the logits processor, and the sampler's launch for the next-token logprobs of the same batch
    assert _native.LOGPROB_LAUNCHES["logprobs"] - before == math.ceil((9 + 4 + 1) / 4) + 1
