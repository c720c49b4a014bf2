"""Host side of the sampling penalties: SamplingParams' new fields (defaults, verify() ranges and messages against
what the reference's own class gave, recorded in tests/golden/penalties.npz) and the reference's call forms on
SamplingBatchInfo (no device work: binding and host tensors only)."""
import dataclasses
import inspect
import json
import threading

import pytest
import torch

from tests import golden

G = golden.load("penalties")


def test_defaults_are_the_references():
    from scratchpad_amd.sampler import SamplingParams
    want = json.loads(str(G["params_defaults"]))
    p = SamplingParams()
    for k, v in want.items():
        assert getattr(p, k) == v, k
    assert not p.needs_penalty_state
    assert sorted(SamplingParams(stop_token_ids=[5, 3, 5]).stop_token_ids) == json.loads(str(G["params_stop_ids_kept_as"]))
    # behind the existing parameters: the old positional form still binds the same way
    names = list(inspect.signature(SamplingParams.__init__).parameters)[1:]
    assert names[:6] == ["max_new_tokens", "temperature", "top_p", "top_k", "min_p", "ignore_eos"]
    assert names[6:] == ["frequency_penalty", "presence_penalty", "repetition_penalty", "min_new_tokens", "stop_token_ids"]


def test_verify_ranges_and_messages_are_the_references():
    from scratchpad_amd.sampler import SamplingParams
    cases = json.loads(str(G["params_verify"]))
    assert sum(c["error"] is not None for c in cases) >= 8 and any(c["error"] is None for c in cases)
    for c in cases:
        p = SamplingParams(**c["kwargs"])
        if c["error"] is None:
            p.verify()
        else:
            with pytest.raises(ValueError) as e:
                p.verify()
            assert str(e.value) == c["error"], c["kwargs"]


def test_repetition_penalty_zero_is_refused():
    from scratchpad_amd.sampler import SamplingParams
    with pytest.raises(ValueError, match="repetition_penalty"):
        SamplingParams(repetition_penalty=0.0).verify()
    for kw in (dict(frequency_penalty=0.1), dict(presence_penalty=-0.1), dict(repetition_penalty=1.2),
               dict(min_new_tokens=1)):
        assert SamplingParams(**kw).needs_penalty_state, kw


def test_reference_call_forms_bind():
    from scratchpad_amd.sampler import PenalizerOrchestrator, SamplingBatchInfo, SamplingParams
    sig = lambda f: inspect.signature(f)
    sig(SamplingBatchInfo.update_regex_vocab_mask).bind(None)
    sig(SamplingBatchInfo.update_penalties).bind(None)
    sig(SamplingBatchInfo.apply_logits_bias).bind(None, None)
    assert list(sig(SamplingBatchInfo.apply_logits_bias).parameters) == ["self", "logits"]
    sig(PenalizerOrchestrator.cumulate_output_tokens).bind(None, None)
    info = SamplingBatchInfo.from_params([SamplingParams(temperature=0.0), SamplingParams(top_k=5)], 100, "cpu")
    assert not info.has_penalties and not info.needs_logits_bias and info.vocab_mask is None
    assert info.penalizer_orchestrator.is_required is False
    info.update_penalties()
    info.update_regex_vocab_mask()
    logits = torch.zeros(2, 100)
    info.apply_logits_bias(logits)                 # nothing to apply: nothing launched, logits untouched
    assert torch.equal(logits, torch.zeros(2, 100))
    info.penalizer_orchestrator.cumulate_output_tokens(torch.tensor([1, 2]))
    # managers/tp_worker_client.py:195-199
    again = dataclasses.replace(info, sampling_info_done=threading.Event(), penalizer_orchestrator=None)
    assert again.penalizer_orchestrator is None and again.temperatures is info.temperatures
    assert isinstance(again.sampling_info_done, threading.Event)


def test_penalised_params_need_a_store_and_host_tensors_are_refused():
    from scratchpad_amd.sampler import SamplingBatchInfo, SamplingParams
    with pytest.raises(RuntimeError, match="PenaltyState"):
        SamplingBatchInfo.from_params([SamplingParams(frequency_penalty=0.5)], 100, "cpu")
    info = SamplingBatchInfo.from_params([SamplingParams()], 100, "cpu")
    info.vocab_mask = torch.zeros(1, 100, dtype=torch.bool)
    assert info.needs_logits_bias
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        info.apply_logits_bias(torch.zeros(1, 100))


def test_filter_and_merge_keep_penalty_rows_aligned():
    """host tensors stand in for the device ones: filter_batch / merge_batch only index and concatenate"""
    from scratchpad_amd.sampler import SamplingBatchInfo, SamplingParams
    store = object()
    a = SamplingBatchInfo.from_params(
        [SamplingParams(frequency_penalty=0.5, min_new_tokens=3, stop_token_ids=[7, 9]), SamplingParams(),
         SamplingParams(repetition_penalty=1.2)], 100, "cpu", req_pool_indices=[4, 2, 6], penalty_state=store,
        stop_token_ids=[{7, 9}, {1}, {1}])
    assert a.has_penalties and a.req_pool_indices.tolist() == [4, -1, 6]
    assert a.stop_token_ids.tolist() == [[7, 9], [-1, -1], [-1, -1]] and a.min_new_tokens.tolist() == [3, 0, 0]
    b = SamplingBatchInfo.from_params([SamplingParams(), SamplingParams(top_k=3)], 100, "cpu")
    a.merge_batch(b)
    assert len(a) == 5 and a.req_pool_indices.tolist() == [4, -1, 6, -1, -1]
    assert a.repetition_penalties.tolist() == pytest.approx([1, 1, 1.2, 1, 1])
    assert a.frequency_penalties.tolist() == [0.5, 0, 0, 0, 0] and a.stop_token_ids.shape == (5, 2)
    a.filter_batch([2, 4, 0], torch.tensor([2, 4, 0]))
    assert a.req_pool_indices.tolist() == [6, -1, 4] and a.min_new_tokens.tolist() == [0, 0, 3]
    assert a.stop_token_ids.tolist() == [[-1, -1], [-1, -1], [7, 9]] and a.penalty_state is store
    assert a.penalised_rows == [True, False, True]
    c = SamplingBatchInfo.from_params([SamplingParams()], 100, "cpu")
    c.merge_batch(a)                      # a side that had none receives neutral rows
    assert c.has_penalties and c.req_pool_indices.tolist() == [-1, 6, -1, 4] and c.penalty_state is store
    again = dataclasses.replace(c, sampling_info_done=threading.Event(), penalizer_orchestrator=None)
    assert again.has_penalties and again.penalty_state is store


def test_update_regex_vocab_mask_follows_the_grammar_protocol():
    from scratchpad_amd.sampler import SamplingBatchInfo, SamplingParams

    class Grammar:
        finished = False

        def __init__(self, allowed):
            self.allowed = allowed

        def allocate_vocab_mask(self, vocab_size, batch_size, device):
            return torch.zeros(batch_size, vocab_size, dtype=torch.bool, device=device)

        def fill_vocab_mask(self, vocab_mask, idx):
            vocab_mask[idx].fill_(1)
            vocab_mask[idx][self.allowed] = False

        @staticmethod
        def move_vocab_mask(vocab_mask, device):
            return vocab_mask

    info = SamplingBatchInfo.from_params([SamplingParams()] * 3, 50, "cpu")
    done = Grammar([1])
    done.finished = True
    info.grammars = [None, Grammar([3, 4]), done]
    assert info.needs_logits_bias
    info.update_regex_vocab_mask()
    assert info.vocab_mask.shape == (3, 50) and info.vocab_mask.dtype == torch.bool
    assert not info.vocab_mask[0].any() and not info.vocab_mask[2].any()
    assert info.vocab_mask[1].sum() == 48 and not info.vocab_mask[1, 3]
    info.grammars = None
    info.update_regex_vocab_mask()
    assert info.vocab_mask is None


def test_filter_drops_the_penalty_rows_with_the_last_penalised_request():
    """a running batch whose penalised requests have all left is again a batch that launches nothing new"""
    from scratchpad_amd.sampler import SamplingBatchInfo, SamplingParams
    a = SamplingBatchInfo.from_params([SamplingParams(temperature=0.0, presence_penalty=0.5), SamplingParams(temperature=0.0),
                                       SamplingParams(temperature=0.0)], 100, "cpu", req_pool_indices=[1, 2, 3],
                                      penalty_state=object(), stop_token_ids=[set(), set(), set()])
    assert a.has_penalties and a.needs_logits_bias
    a.filter_batch([0, 2], torch.tensor([0, 2]))
    assert a.has_penalties and a.penalised_rows == [True, False]
    a.filter_batch([1], torch.tensor([1]))
    assert not a.has_penalties and not a.needs_logits_bias and a.req_pool_indices is None and a.stop_token_ids is None
    b = SamplingBatchInfo.from_params([SamplingParams(repetition_penalty=1.5)], 100, "cpu", req_pool_indices=[7],
                                      penalty_state=a.penalty_state, stop_token_ids=[set()])
    a.merge_batch(b)                       # ... and can take penalised rows again
    assert a.has_penalties and a.req_pool_indices.tolist() == [-1, 7] and a.penalised_rows == [False, True]


def test_stop_ids_skip_a_tokenizer_without_an_eos_id():
    from types import SimpleNamespace
    from scratchpad_amd.sampler import SamplingBatchInfo, SamplingParams
    tok = SimpleNamespace(eos_token_id=None, additional_stop_token_ids={4})
    req = SimpleNamespace(sampling_params=SamplingParams(min_new_tokens=2, stop_token_ids=[9]), eos_token_ids=None,
                          tokenizer=tok, req_pool_idx=0)
    pool = SimpleNamespace(penalty_state=object())
    info = SamplingBatchInfo.from_schedule_batch(SimpleNamespace(reqs=[req], device="cpu", req_to_token_pool=pool), 100)
    assert info.stop_token_ids.tolist() == [[4, 9]]
