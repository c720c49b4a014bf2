"""Sampling penalties and grammar masks through ScheduleBatch + ModelRunner (+ TpModelWorkerClient): a tiny Llama
(vocab 2 000, random weights, fp32) decodes a mixed batch - penalised greedy, penalised top-p, unpenalised rows - for
more than 48 steps with a request finishing (filter_batch), a newly prefilled one joining (merge_batch), one
retract_decode + re-admission and one chunked prefill.  Every sample() call is wrapped: the logits are cloned before it,
tests/penalty_oracle.py is applied to the clone with the history the driver tracked on the host, and

* the logits the sampler saw are within the bound of tests/penalty_oracle.tolerance (untouched columns bit-identical),
* every greedy row whose oracle top-2 gap exceeds twice that bound drew the oracle's id (rows below it are skipped;
  at most 1 % of row-steps, asserted),
* unpenalised rows are bit-identical (logits and ids) to a run of the same trace without any penalty,
* a min_new_tokens row never emits a stop id early and does afterwards,
* the overlap worker gives the ids of the synchronous one, one cumulate launch per emitted-token step in both,
* under the overlap worker a request admitted into the pool row of a request whose last batch is still queued starts
  from its own history (the reset runs behind that batch's cumulate),
* after retraction the device history equals req.output_ids,
* a masked token is never drawn (stub grammar objects of both mask forms),
* a trace without penalties or masks launches none of the new kernels and allocates no store."""
from collections import Counter

import numpy as np
import pytest
import torch

from tests import penalty_oracle as po

pytestmark = pytest.mark.gpu
VOCAB = 2000
STEPS = 52
STOP_BELOW = 1000          # the min_new_tokens request's stop ids: every id below this


def make_runner():
    from scratchpad_amd.model_runner import ModelConfig, ModelRunner, ServerArgs
    cfg = ModelConfig(128, 256, 2, 2, 1, VOCAB, context_len=160, max_position_embeddings=512)
    mr = ModelRunner(cfg, ServerArgs(max_total_tokens=2048, max_running_requests=8, disable_cuda_graph=True),
                     dtype=torch.float32, seed=3)
    for name, p in mr.model.named_parameters():       # logits of spread O(1), not O(0.01)
        if "lm_head" in name or "embed_tokens" in name:
            p.data.mul_(60.0)
    mr.sampler.generator = torch.Generator(device=mr.device).manual_seed(17)      # the fixed uniforms
    return mr


def params(penalised):
    from scratchpad_amd.sampler import SamplingParams
    pen = lambda **kw: kw if penalised else {}
    return {
        "A": SamplingParams(temperature=0.0, max_new_tokens=999, **pen(frequency_penalty=0.5, presence_penalty=0.3,
                            min_new_tokens=6, stop_token_ids=list(range(STOP_BELOW)))),
        "B": SamplingParams(temperature=0.8, top_p=0.9, max_new_tokens=999, **pen(repetition_penalty=1.3, frequency_penalty=-0.25)),
        "C": SamplingParams(temperature=0.0, max_new_tokens=999),
        "D": SamplingParams(temperature=1.0, top_k=20, max_new_tokens=999),
        "E": SamplingParams(temperature=0.0, max_new_tokens=999, **pen(presence_penalty=1.1, repetition_penalty=0.9)),
        "F": SamplingParams(temperature=0.0, max_new_tokens=999, **pen(frequency_penalty=1.5)),
        "H": SamplingParams(temperature=0.0, max_new_tokens=999),
    }


class Trace:
    """what the wrapped ModelRunner.sample saw: per call (rids, logits before, logits the sampler saw, ids)"""

    def __init__(self, mr):
        self.calls, self.rids = [], None
        inner_sample, inner_sampler = mr.sample, mr.sampler.forward
        box = {}

        def sampler_forward(logits_output, *args, **kwargs):
            box["seen"] = logits_output.gather_full_logits().clone()      # (a sampling batch turns them into probabilities)
            return inner_sampler(logits_output, *args, **kwargs)

        def sample(logits_output, forward_batch):
            before = logits_output.gather_full_logits().clone()
            ids = inner_sample(logits_output, forward_batch)
            self.calls.append((list(self.rids), before.cpu().numpy(), box.pop("seen").cpu().numpy(), ids.cpu().tolist()))
            return ids
        mr.sampler.forward = sampler_forward
        mr.sample = sample


def run(overlap, penalised, trace=False):
    """the trace described in the module docstring; returns ({rid: emitted ids}, Trace or None, notes)"""
    from scratchpad_amd import _native
    from scratchpad_amd.model_runner import TpModelWorker
    from scratchpad_amd.penalty_state import penalty_state_of
    from scratchpad_amd.sampler import SamplingBatchInfo
    from scratchpad_amd.schedule_batch import FINISH_LENGTH, Req, ScheduleBatch
    from scratchpad_amd.tp_worker_client import TpModelWorkerClient
    mr = make_runner()
    tr = Trace(mr) if trace else None
    worker = TpModelWorkerClient(mr) if overlap else TpModelWorker(mr)
    r2t, alloc, dev = mr.req_to_token_pool, mr.token_to_kv_pool_allocator, mr.device
    sp = params(penalised)
    gen = torch.Generator().manual_seed(5)
    prompt = lambda n: torch.randint(0, VOCAB, (n,), generator=gen).tolist()
    reqs = {k: Req(k, "", prompt(n), sp[k]) for k, n in (("A", 7), ("B", 5), ("C", 9), ("D", 4), ("E", 6), ("F", 14), ("H", 3))}
    launches0 = dict(_native.PENALTY_LAUNCHES)
    notes = {}
    pending = []              # overlap: batches whose ids have not been resolved yet, as lists of requests

    def batch(rs):
        return ScheduleBatch(list(rs), r2t, alloc, device=dev, model_config=mr.model_config, enable_overlap=overlap)

    def forward(b):
        """one forward + sample; the sampled ids go to the requests (at once, or one launch later under overlap)"""
        if tr:
            tr.rids = [r.rid for r in b.reqs]
        _, ids = worker.forward_batch_generation(b.get_model_worker_batch())
        b.output_ids = ids
        if overlap:
            pending.append(list(b.reqs))
            if len(pending) > 1:
                settle()
        else:
            for r, t in zip(b.reqs, ids.tolist()):
                r.output_ids.append(t)

    def settle():
        _, real = worker.resolve_last_batch_result()
        for r, t in zip(pending.pop(0), real):
            r.output_ids.append(t)

    def drain():
        while pending:
            settle()

    def admit(rs):
        b = batch(rs)
        b.prepare_for_extend()
        b.sampling_info = SamplingBatchInfo.from_schedule_batch(b, VOCAB)
        return b

    sb = admit([reqs[k] for k in "ABCD"])
    forward(sb)
    for step in range(STEPS):
        if step == 10:                                   # C finishes: filter_batch, its row and slots go back
            drain()
            c = reqs["C"]
            c.finished_reason = FINISH_LENGTH(length=len(c.output_ids))
            idx = [r.rid for r in sb.reqs].index("C")
            n = int(sb.seq_lens[idx])
            sb.filter_batch()
            alloc.free(r2t.req_to_token[c.req_pool_idx, :n].to(torch.int64))
            r2t.free(c.req_pool_idx)
        if step == 15:                                   # E is prefilled on its own and joins: merge_batch
            nb = admit([reqs["E"]])
            forward(nb)
            sb.merge_batch(nb)
        if step == 25:                                   # retraction of the request with the fewest tokens (E) ...
            drain()
            retracted, _ = sb.retract_decode(1)
            assert [r.rid for r in retracted] == ["E"] and reqs["E"].req_pool_idx is None
            notes["retracted_after"] = len(reqs["E"].output_ids)
        if step == 27:                                   # ... and its re-admission: the history is seeded from output_ids
            drain()
            e = reqs["E"]
            e.init_next_round_input()
            nb = admit([e])
            notes["seeded"] = len(e.output_ids)
            forward(nb)
            if penalised:        # (seeded in front of this batch's own sample, then the new token is counted)
                drain()
                got, out_len = penalty_state_of(r2t, create=False).history(e.req_pool_idx)
                assert {t: c for t, c in got} == dict(Counter(e.output_ids))
                assert out_len == len(e.output_ids) == notes["seeded"] + 1
            sb.merge_batch(nb)
        if step == 33:                                   # F: chunked prefill, 8 + 6 tokens
            drain()
            f = reqs["F"]
            f.fill_ids = f.origin_input_ids[:8]
            nb = admit([f])
            forward(nb)                                  # the token a non-final chunk samples is thrown away
            drain()
            f.output_ids.clear()
            f.prefix_indices = r2t.req_to_token[f.req_pool_idx, :8].to(torch.int64).clone()
            r2t.free(f.req_pool_idx)
            f.fill_ids = None
            nb = admit([f])
            forward(nb)
            if penalised:
                drain()
                assert penalty_state_of(r2t).history(f.req_pool_idx) == ([[f.output_ids[0], 1]], 1), "the discarded token was kept"
            sb.merge_batch(nb)
        if step == 40:                                   # H: an unpenalised request joins a penalised batch
            nb = admit([reqs["H"]])
            forward(nb)
            sb.merge_batch(nb)
        sb.prepare_for_decode()
        forward(sb)
    drain()
    if overlap:
        worker.close()
    torch.cuda.synchronize()
    state = penalty_state_of(r2t, create=False)
    if state is not None:
        state.check()
    notes["launches"] = {k: _native.PENALTY_LAUNCHES[k] - launches0[k] for k in launches0}
    notes["store"] = state
    notes["rows"] = {k: r.req_pool_idx for k, r in reqs.items()}
    notes["samples"] = 1 + STEPS + 5
    return {k: list(r.output_ids) for k, r in reqs.items()}, tr, notes


@pytest.fixture(scope="module")
def runs():
    return {"pen": run(False, True, trace=True), "plain": run(False, False, trace=True), "overlap": run(True, True)}


def test_logits_and_greedy_ids_follow_the_oracle_at_every_step(runs):
    tokens, tr, notes = runs["pen"]
    sp = params(True)
    hist = {k: [] for k in tokens}
    row_steps = skipped = greedy_checked = 0
    worst = 0.0
    assert len(tr.calls) == notes["samples"] and len(tr.calls) - 6 >= 48
    discarded = [i for i, c in enumerate(tr.calls) if c[0] == ["F"]][0]      # the non-final chunk's sample
    for call, (rids, before, seen, ids) in enumerate(tr.calls):
        p = [sp[r] for r in rids]
        freq, pres, rep = ([getattr(q, n) for q in p] for n in ("frequency_penalty", "presence_penalty", "repetition_penalty"))
        min_new = [q.min_new_tokens for q in p]
        stops = [sorted(q.stop_token_ids or ()) for q in p]
        h = [hist[r] for r in rids]
        want = po.apply_penalties(before, h, freq, pres, rep, min_new, stops)
        tol = po.tolerance(before, h, freq, pres, rep)
        worst = max(worst, po.check_against(seen, want, before, tol, f"sample call {call} {rids}"))
        for i, r in enumerate(rids):
            row_steps += 1
            if not sp[r].needs_penalty_state:
                assert np.array_equal(seen[i].view(np.int32), before[i].view(np.int32)), (call, r)
            if sp[r].top_k == 1:
                order = np.argsort(want[i])[::-1][:2]
                gap = float(want[i][order[0]]) - float(want[i][order[1]])
                if gap > 2 * float(max(tol[i][order[0]], tol[i][order[1]])):
                    assert ids[i] == int(order[0]), (call, r, ids[i], int(order[0]), gap)
                    greedy_checked += 1
                else:
                    skipped += 1
        if call == discarded:
            continue                              # thrown away: not part of F's history
        for r, t in zip(rids, ids):
            hist[r].append(t)
    print(f"row-steps {row_steps}, greedy rows checked {greedy_checked}, skipped for a small gap {skipped}, "
          f"worst |diff| / bound {worst:.3f}")
    assert skipped <= 0.01 * row_steps, (skipped, row_steps)
    assert greedy_checked >= 100
    assert hist == tokens


def test_min_new_tokens_holds_stop_ids_back_and_then_releases_them(runs):
    a = runs["pen"][0]["A"]
    assert all(t >= STOP_BELOW for t in a[:6]), a[:6]
    assert any(t < STOP_BELOW for t in a[6:]), "half the vocabulary are stop ids: one is drawn once they are released"
    assert any(t < STOP_BELOW for t in runs["plain"][0]["A"][:6]), "the trace without min_new_tokens is no witness"


def test_device_history_equals_output_ids_after_the_whole_trace(runs):
    tokens, _, notes = runs["pen"]
    assert notes["seeded"] == notes["retracted_after"] > 0
    for k in "ABEF":
        got, out_len = notes["store"].history(notes["rows"][k])
        assert {t: c for t, c in got} == dict(Counter(tokens[k])) and out_len == len(tokens[k]), k
    assert max(Counter(tokens["A"]).values()) >= 1 and len(tokens["A"]) == STEPS + 1


def test_unpenalised_rows_are_bit_identical_to_a_run_without_penalties(runs):
    (tok_p, tr_p, _), (tok_u, tr_u, notes_u) = runs["pen"], runs["plain"]
    for k in "CDH":
        assert tok_p[k] == tok_u[k], k
    assert tok_p["A"] != tok_u["A"] and tok_p["E"] != tok_u["E"]
    same = 0
    for (rids_p, before_p, seen_p, _), (rids_u, before_u, _, _) in zip(tr_p.calls, tr_u.calls):
        assert rids_p == rids_u
        for i, r in enumerate(rids_p):
            if r in "CDH":
                assert np.array_equal(before_p[i].view(np.int32), before_u[i].view(np.int32)), r
                assert np.array_equal(seen_p[i].view(np.int32), before_u[i].view(np.int32)), r
                same += 1
    assert same >= 60


def test_a_trace_without_penalties_launches_nothing_new_and_allocates_no_store(runs):
    notes = runs["plain"][2]
    assert notes["launches"] == {"reset": 0, "cumulate": 0, "apply": 0, "mask": 0}
    assert notes["store"] is None


def test_overlap_worker_gives_the_same_ids_with_one_cumulate_per_step(runs):
    (tok_s, _, notes_s), (tok_o, _, notes_o) = runs["pen"], runs["overlap"]
    assert tok_o == tok_s
    # one apply and one cumulate per sample() call of a batch with penalised rows, in both modes; seeding adds one
    # cumulate per position of a re-admitted history (E after its retraction) and one reset per admission
    for notes in (notes_s, notes_o):
        penalised_calls = notes["samples"] - 1           # every call but the prefill of H on its own
        assert notes["launches"]["apply"] == penalised_calls
        assert notes["launches"]["cumulate"] == penalised_calls + notes["seeded"]
        assert notes["launches"]["mask"] == 0


def test_sampler_ids_without_penalties_are_the_kernels_own():
    """a batch with neither penalties nor masks goes through the sampler exactly as before: its ids are those of the
    argmax / softmax / sample kernels called directly on the existing sampling inputs"""
    from scratchpad_amd import _native
    from scratchpad_amd.llama import LogitsProcessorOutput
    from scratchpad_amd.sampler import Sampler, SamplingBatchInfo, SamplingParams
    from tests import sampling_inputs as si
    rows, vocab = 16, 4096
    logits, temps = si.softmax_logits(vocab, rows)
    ks, ps, ms, u = si.model_params(vocab, rows, 0)
    prm = [SamplingParams(temperature=float(t), top_k=int(k) if k < si.K_ALL else -1, top_p=float(p), min_p=float(m))
           for t, k, p, m in zip(temps, ks, ps, ms)]
    info = SamplingBatchInfo.from_params(prm, vocab, "cuda")
    before = dict(_native.PENALTY_LAUNCHES)
    uu = torch.from_numpy(u).cuda()
    got = Sampler()(LogitsProcessorOutput(next_token_logits=logits.cuda().clone()), info, uniform=uu)
    probs = _native.softmax_temperature_(logits.cuda().clone(), info.temperatures)
    want = _native.top_k_top_p_min_p_sample(probs, info.top_ks, info.top_ps, info.min_ps, uu)
    assert torch.equal(got, want)
    greedy = SamplingBatchInfo.from_params([SamplingParams(temperature=0.0)] * rows, vocab, "cuda")
    assert torch.equal(Sampler()(LogitsProcessorOutput(next_token_logits=logits.cuda()), greedy), _native.argmax(logits.cuda()))
    assert _native.PENALTY_LAUNCHES == before and not info.needs_logits_bias


class StubGrammar:
    """follows constrained/base_backend.py as SamplingBatchInfo.update_regex_vocab_mask uses it; allows ids = 0 mod 3"""
    finished = False

    def __init__(self, packed):
        self.packed = packed

    def allocate_vocab_mask(self, vocab_size, batch_size, device):
        if self.packed:
            return torch.full((batch_size, (vocab_size + 31) // 32), -1, dtype=torch.int32)      # all allowed, as xgrammar allocates
        return torch.zeros((batch_size, vocab_size), dtype=torch.bool)

    def fill_vocab_mask(self, vocab_mask, idx):
        allowed = torch.arange(0, VOCAB, 3)
        if self.packed:
            bits = torch.zeros(vocab_mask.shape[1] * 32, dtype=torch.int64)
            bits[allowed] = 1
            words = (bits.view(-1, 32) << torch.arange(32)).sum(1)
            vocab_mask[idx] = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)
        else:
            vocab_mask[idx].fill_(True)
            vocab_mask[idx][allowed] = False

    @staticmethod
    def move_vocab_mask(vocab_mask, device):
        return vocab_mask.to(device)


@pytest.mark.parametrize("packed", [True, False])
def test_a_masked_token_is_never_drawn(packed):
    from scratchpad_amd import _native
    from scratchpad_amd.model_runner import TpModelWorker
    from scratchpad_amd.sampler import SamplingBatchInfo, SamplingParams
    from scratchpad_amd.schedule_batch import Req, ScheduleBatch
    mr = make_runner()
    worker = TpModelWorker(mr)
    gen = torch.Generator().manual_seed(8)
    prm = [SamplingParams(temperature=0.0), SamplingParams(temperature=1.0, top_p=0.95), SamplingParams(temperature=0.0),
           SamplingParams(temperature=0.0, frequency_penalty=0.5)]
    reqs = [Req(str(i), "", torch.randint(0, VOCAB, (5 + i,), generator=gen).tolist(), p) for i, p in enumerate(prm)]
    for i in (0, 1, 3):
        reqs[i].grammar = StubGrammar(packed)
    sb = ScheduleBatch(reqs, mr.req_to_token_pool, mr.token_to_kv_pool_allocator, device=mr.device,
                       model_config=mr.model_config, has_grammar=True)
    sb.prepare_for_extend()
    sb.sampling_info = SamplingBatchInfo.from_schedule_batch(sb, VOCAB)
    before = _native.PENALTY_LAUNCHES["mask"]
    drawn = [[] for _ in reqs]
    for step in range(13):
        if step:
            sb.prepare_for_decode()
        _, ids = worker.forward_batch_generation(sb.get_model_worker_batch())
        for d, r, t in zip(drawn, reqs, ids.tolist()):
            d.append(t)
            r.output_ids.append(t)
        sb.output_ids = ids
    assert _native.PENALTY_LAUNCHES["mask"] - before == 13
    for i in (0, 1, 3):
        assert all(t % 3 == 0 for t in drawn[i]), (i, drawn[i])
    assert any(t % 3 for t in drawn[2]), "the row without a grammar is not masked"


def test_overlap_admission_into_a_row_whose_previous_owner_is_still_queued():
    """The overlap scheduler sees a finish one step late: batch k is queued with request R still in it when R's row
    is freed and handed to the next admission (rows are first-freed-first).  The forward thread is held before batch k
    here, so everything the scheduler thread does for the admission happens first; R's last, discarded token must
    still not reach the history of the request that now owns the row, and its min_new_tokens count starts at 0."""
    import threading
    from scratchpad_amd.penalty_state import penalty_state_of
    from scratchpad_amd.sampler import SamplingBatchInfo, SamplingParams
    from scratchpad_amd.schedule_batch import FINISH_LENGTH, Req, ScheduleBatch
    from scratchpad_amd.tp_worker_client import TpModelWorkerClient
    mr = make_runner()
    client = TpModelWorkerClient(mr)
    gate, held, inner = threading.Event(), {}, client._run_one

    def run_one(batch, first_slot):
        if batch is held.get("batch"):
            assert gate.wait(60)
        return inner(batch, first_slot)
    client._run_one = run_one
    r2t, alloc, dev = mr.req_to_token_pool, mr.token_to_kv_pool_allocator, mr.device
    gen = torch.Generator().manual_seed(21)
    prompt = lambda n: torch.randint(0, VOCAB, (n,), generator=gen).tolist()
    old = Req("R", "", prompt(6), SamplingParams(temperature=0.0, max_new_tokens=99, frequency_penalty=0.5))
    other = Req("S", "", prompt(5), SamplingParams(temperature=0.0, max_new_tokens=99, presence_penalty=0.25))
    new = Req("N", "", prompt(7), SamplingParams(temperature=0.0, max_new_tokens=99, frequency_penalty=1.5, min_new_tokens=3,
                                                 stop_token_ids=list(range(STOP_BELOW))))
    pending = []

    def batch(rs):
        return ScheduleBatch(list(rs), r2t, alloc, device=dev, model_config=mr.model_config, enable_overlap=True)

    def forward(b, hold=False):
        mwb = b.get_model_worker_batch()
        if hold:
            held["batch"] = mwb
        _, ids = client.forward_batch_generation(mwb)
        b.output_ids = ids
        pending.append(list(b.reqs))

    def settle():
        _, real = client.resolve_last_batch_result()
        for r, t in zip(pending.pop(0), real):
            r.output_ids.append(t)

    try:
        sb = batch([old, other])
        sb.prepare_for_extend()
        sb.sampling_info = SamplingBatchInfo.from_schedule_batch(sb, VOCAB)
        forward(sb)
        for _ in range(3):
            sb.prepare_for_decode()
            forward(sb)
            settle()
        sb.prepare_for_decode()
        forward(sb, hold=True)                       # batch k: R is still in it, the forward thread waits in front of it
        settle()                                     # the result of batch k - 1: the scheduler decides R is finished
        old.finished_reason = FINISH_LENGTH(length=len(old.output_ids))
        row, n = old.req_pool_idx, int(sb.seq_lens[0])
        sb.filter_batch()
        alloc.free(r2t.req_to_token[row, :n].to(torch.int64))
        r2t.free(row)
        r2t.free_slots = [row] + [x for x in r2t.free_slots if x != row]      # a saturated pool: the next row out is R's
        nb = batch([new])
        nb.prepare_for_extend()
        assert new.req_pool_idx == row
        nb.sampling_info = SamplingBatchInfo.from_schedule_batch(nb, VOCAB)
        forward(nb)
        torch.cuda.synchronize()                     # whatever the scheduler side enqueued has run
        gate.set()
        settle()                                     # batch k (R's token is discarded with its request) ...
        old_tokens = len(old.output_ids)
        settle()                                     # ... and the admission
        sb.merge_batch(nb)
        for _ in range(4):
            sb.prepare_for_decode()
            forward(sb)
            settle()
        torch.cuda.synchronize()
    finally:
        gate.set()
        client.close()
    assert old_tokens == 5
    state = penalty_state_of(r2t, create=False)
    state.check()
    got, out_len = state.history(row)
    assert {t: c for t, c in got} == dict(Counter(new.output_ids)) and out_len == len(new.output_ids), (got, new.output_ids)
    assert len(new.output_ids) == 5 and all(t >= STOP_BELOW for t in new.output_ids[:3])
    got, out_len = state.history(other.req_pool_idx)
    assert {t: c for t, c in got} == dict(Counter(other.output_ids)) and out_len == len(other.output_ids)
