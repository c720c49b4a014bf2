"""Next-token sampler on the HIP kernels of csrc/sampling.hip.

Mirrors nn/layers/sampler.py:24-163 (``Sampler.forward``), sampling/sampling_params.py:16-71
(``SamplingParams``: temperature < eps means greedy, top_k == -1 means the whole vocabulary) and the
tensor fields of sampling/sampling_batch_info.py:14-137 (``SamplingBatchInfo.from_schedule_batch``).
Sampling penalties (frequency / presence / repetition, ``min_new_tokens`` over the stop ids) and grammar vocab
masks run on the device between the logits processor and this sampler (``SamplingBatchInfo.apply_logits_bias``,
csrc/penalties.hip, penalty_state.py; DESIGN.md "Penalties and vocab masks").  Out of scope: the grammar back-ends
themselves (the masks of objects that follow constrained/base_backend.py are applied, nothing compiles a grammar),
``logit_bias`` (a field nothing in the reference ever fills) and custom logit processors (pickled Python).

Differences by design:
* the filter never sorts the vocabulary (see the kernel header) and carries mass as integers, so
  the drawn token is a pure function of (probabilities, top_k, top_p, min_p, uniform) - identical on
  every TP rank without the MIN all-reduce of sampler.py:146-157, which is still available as
  ``sync_token_ids_across_tp``;
* both reference back-ends ("flashinfer" rejection sampling and the "pytorch" sort) draw from the
  same filtered distribution; one kernel covers both.  With min-p the flashinfer branch
  renormalises between its top-k and top-p steps (sampler.py:91-96); the joint definition of
  sampler.py:195-221 is the one implemented, for every branch;
* penalty state is a per-request list of (token, count) on the device, indexed by ``req_pool_idx``, not a dense
  ``[bs, vocab]`` tensor per penalizer: ``filter_batch`` / ``merge_batch`` move the per-row scalars only,
  ``update_penalties()`` has nothing to do, and the tokens are cumulated where they are drawn
  (``ModelRunner.sample``), in the synchronous and the overlap worker alike.
"""
import threading
from dataclasses import dataclass, field
from typing import List, Optional

import torch
from torch import nn

from . import _native
from .penalty_state import PenaltyState, penalty_state_of

_SAMPLING_EPS = 1e-6
TOP_K_ALL = 1 << 30


class SamplingParams:
    """sampling/sampling_params.py:16-71 (the fields the sampler and the penalty kernels read)."""

    def __init__(self, max_new_tokens: int = 128, temperature: float = 1.0, top_p: float = 1.0,
                 top_k: int = -1, min_p: float = 0.0, ignore_eos: bool = False, frequency_penalty: float = 0.0,
                 presence_penalty: float = 0.0, repetition_penalty: float = 1.0, min_new_tokens: int = 0,
                 stop_token_ids: Optional[List[int]] = None):
        self.max_new_tokens = max_new_tokens
        self.stop_token_ids = set(stop_token_ids) if stop_token_ids else None
        self.frequency_penalty = frequency_penalty
        self.presence_penalty = presence_penalty
        self.repetition_penalty = repetition_penalty
        self.min_new_tokens = min_new_tokens
        self.temperature = temperature
        self.top_p = top_p
        self.top_k = top_k
        self.min_p = min_p
        self.ignore_eos = ignore_eos
        if 0 <= self.temperature < _SAMPLING_EPS:      # greedy
            self.temperature = 1.0
            self.top_k = 1
        if self.top_k == -1:
            self.top_k = TOP_K_ALL

    @property
    def needs_penalty_state(self) -> bool:
        """does this request need its output history on the device (any of the four parameters not neutral)"""
        return (self.frequency_penalty != 0.0 or self.presence_penalty != 0.0 or self.repetition_penalty != 1.0
                or self.min_new_tokens > 0)

    def verify(self):
        """sampling_params.py:73-114"""
        if self.temperature < 0.0:
            raise ValueError(f"temperature must be non-negative, got {self.temperature}.")
        if not 0.0 < self.top_p <= 1.0:
            raise ValueError(f"top_p must be in (0, 1], got {self.top_p}.")
        if not 0.0 <= self.min_p <= 1.0:
            raise ValueError(f"min_p must be in [0, 1], got {self.min_p}.")
        if self.top_k < 1:
            raise ValueError(f"top_k must be -1 (disable) or at least 1, got {self.top_k}.")
        if not -2.0 <= self.frequency_penalty <= 2.0:
            raise ValueError(f"frequency_penalty must be in [-2, 2], got {self.frequency_penalty}.")
        if not -2.0 <= self.presence_penalty <= 2.0:
            raise ValueError(f"presence_penalty must be in [-2, 2], got {self.presence_penalty}.")
        if not 0.0 <= self.repetition_penalty <= 2.0:
            raise ValueError(f"repetition_penalty must be in [0, 2], got {self.repetition_penalty}.")
        if self.repetition_penalty == 0.0:
            # inside the reference's range, but its formula (sampling_batch_info.py:336-340) turns every -inf column
            # (a masked or stop token) into -inf * 0 = NaN
            raise ValueError("repetition_penalty must not be 0 (it would turn masked logits into NaN), got 0.0.")
        if not 0 <= self.min_new_tokens:
            raise ValueError(f"min_new_tokens must be in [0, max_new_tokens], got {self.min_new_tokens}.")
        if self.max_new_tokens is not None:
            if self.max_new_tokens < 0:
                raise ValueError(f"max_new_tokens must be at least 0, got {self.max_new_tokens}.")
            if not self.min_new_tokens <= self.max_new_tokens:
                raise ValueError(f"min_new_tokens must be in [0, max_new_tokens({self.max_new_tokens})], got "
                                 f"{self.min_new_tokens}.")


class PenalizerOrchestrator:
    """What the reference's call sites read of penaltylib.BatchedPenalizerOrchestrator (schedule_batch.py:1254-1275):
    ``is_required`` and ``cumulate_output_tokens(ids)``.  A view of its SamplingBatchInfo - the state itself lives in
    the pool's PenaltyState, so an info whose orchestrator was replaced by None still applies its penalties."""

    def __init__(self, info: "SamplingBatchInfo"):
        self._info = info

    @property
    def is_required(self) -> bool:
        return self._info.has_penalties

    def cumulate_output_tokens(self, output_ids: torch.Tensor) -> None:
        self._info.cumulate_output_tokens(output_ids)


_PENALTY_ROWS = ("frequency_penalties", "presence_penalties", "repetition_penalties", "min_new_tokens",
                 "stop_token_ids", "req_pool_indices")


@dataclass
class SamplingBatchInfo:
    temperatures: torch.Tensor      # [bs, 1] fp32
    top_ps: torch.Tensor            # [bs] fp32
    top_ks: torch.Tensor            # [bs] int32
    min_ps: torch.Tensor            # [bs] fp32
    is_all_greedy: bool
    need_min_p_sampling: bool
    vocab_size: int
    device: str = "cuda"
    grammars: Optional[list] = None
    # grammar mask of this step: int32 [bs, w] packed (xgrammar) or bool [bs, vocab] (outlines); update_regex_vocab_mask
    vocab_mask: Optional[torch.Tensor] = None
    sampling_info_done: Optional[threading.Event] = None
    penalizer_orchestrator: Optional[PenalizerOrchestrator] = field(default=None, repr=False, compare=False)
    # penalties: all None while no request of the batch has any.  Rows follow the batch; the history they index
    # (penalty_state, rows req_pool_indices; -1 = a row without penalties) follows the request.
    frequency_penalties: Optional[torch.Tensor] = None      # [bs] fp32
    presence_penalties: Optional[torch.Tensor] = None       # [bs] fp32
    repetition_penalties: Optional[torch.Tensor] = None     # [bs] fp32
    min_new_tokens: Optional[torch.Tensor] = None           # [bs] int32
    stop_token_ids: Optional[torch.Tensor] = None           # [bs, max_stops] int32, -1 = none
    req_pool_indices: Optional[torch.Tensor] = None         # [bs] int64
    penalty_state: Optional[PenaltyState] = field(default=None, repr=False, compare=False)
    penalised_rows: Optional[List[bool]] = None             # host copy of "req_pool_indices >= 0", row by row

    @classmethod
    def from_params(cls, params: List[SamplingParams], vocab_size: int, device: str,
                    req_pool_indices: Optional[List[int]] = None, penalty_state: Optional[PenaltyState] = None,
                    stop_token_ids: Optional[List[set]] = None):
        """``req_pool_indices`` / ``penalty_state`` / ``stop_token_ids`` (one set per request: what ends it): needed
        as soon as one of the params carries a penalty - its history lives in that store under that row."""
        f32 = lambda xs: torch.tensor(xs, dtype=torch.float).to(device, non_blocking=True)
        info = cls(
            temperatures=f32([p.temperature for p in params]).view(-1, 1),
            top_ps=f32([p.top_p for p in params]),
            top_ks=torch.tensor([p.top_k for p in params], dtype=torch.int32).to(device, non_blocking=True),
            min_ps=f32([p.min_p for p in params]),
            is_all_greedy=all(p.top_k <= 1 for p in params),
            need_min_p_sampling=any(p.min_p > 0 for p in params),
            vocab_size=vocab_size, device=device)
        info.penalizer_orchestrator = PenalizerOrchestrator(info)
        needs = [p.needs_penalty_state for p in params]
        if any(needs):
            if penalty_state is None or req_pool_indices is None:
                raise RuntimeError("sampling penalties need the pool's PenaltyState and the requests' req_pool_idx "
                                   "(SamplingBatchInfo.from_schedule_batch after prepare_for_extend)")
            if any(n and (r is None or r < 0) for n, r in zip(needs, req_pool_indices)):
                raise RuntimeError("a penalised request has no req_pool_idx yet: build the SamplingBatchInfo after "
                                   "prepare_for_extend")
            stops = [sorted(s) if (n and p.min_new_tokens > 0 and s) else []
                     for n, p, s in zip(needs, params, stop_token_ids or [None] * len(params))]
            width = max(len(s) for s in stops)
            info.frequency_penalties = f32([p.frequency_penalty for p in params])
            info.presence_penalties = f32([p.presence_penalty for p in params])
            info.repetition_penalties = f32([p.repetition_penalty for p in params])
            info.min_new_tokens = torch.tensor([p.min_new_tokens for p in params], dtype=torch.int32).to(
                device, non_blocking=True)
            info.stop_token_ids = torch.tensor([s + [-1] * (width - len(s)) for s in stops],
                                               dtype=torch.int32).view(len(params), width).to(device, non_blocking=True)
            info.req_pool_indices = torch.tensor([r if n else -1 for n, r in zip(needs, req_pool_indices)],
                                                 dtype=torch.int64).to(device, non_blocking=True)
            info.penalty_state = penalty_state
            info.penalised_rows = list(needs)
        return info

    @classmethod
    def from_schedule_batch(cls, batch, vocab_size: int):
        """sampling_batch_info.py:54-137; a request without sampling_params is greedy.  The stop ids of a request are
        what min_new_tokens.py:29-46 collects, from the fields Req has: the params' stop_token_ids, the request's
        eos_token_ids and, when it carries a tokenizer, that one's eos / additional stop ids."""
        greedy = SamplingParams(temperature=0.0)
        params = [getattr(r, "sampling_params", None) or greedy for r in batch.reqs]
        if not any(p.needs_penalty_state for p in params):
            return cls.from_params(params, vocab_size, batch.device)
        stops = []
        for r, p in zip(batch.reqs, params):
            s = set(p.stop_token_ids or ()) | set(getattr(r, "eos_token_ids", None) or ())
            tok = getattr(r, "tokenizer", None)
            if tok is not None:
                s |= set(getattr(tok, "additional_stop_token_ids", None) or ()) | {tok.eos_token_id}
            stops.append({t for t in s if t is not None})      # (a tokenizer without an eos id)
        return cls.from_params(params, vocab_size, batch.device, [r.req_pool_idx for r in batch.reqs],
                               penalty_state_of(batch.req_to_token_pool), stops)

    def __len__(self):
        return self.temperatures.shape[0]

    @property
    def has_penalties(self) -> bool:
        return self.frequency_penalties is not None

    @property
    def needs_logits_bias(self) -> bool:
        """must the sampler see full fp32 logits that went through apply_logits_bias (no greedy shortcut)"""
        return self.has_penalties or self.vocab_mask is not None or bool(self.grammars)

    def filter_batch(self, keep_indices: List[int], keep_indices_device: torch.Tensor):
        """sampling_batch_info.py filter_batch: keep the rows of the surviving requests.  The penalty histories stay
        where they are (rows of the request pool); only the per-row scalars are gathered."""
        self.temperatures = self.temperatures[keep_indices_device]
        self.top_ps = self.top_ps[keep_indices_device]
        self.top_ks = self.top_ks[keep_indices_device]
        self.min_ps = self.min_ps[keep_indices_device]
        if self.has_penalties:
            self.penalised_rows = [self.penalised_rows[i] for i in keep_indices]
            if any(self.penalised_rows):
                for name in _PENALTY_ROWS:
                    setattr(self, name, getattr(self, name)[keep_indices_device])
            else:
                # the last penalised request has left: back to a batch that launches nothing new and keeps the
                # vocab-parallel greedy shortcut
                for name in _PENALTY_ROWS:
                    setattr(self, name, None)
                self.penalised_rows = None
        self.vocab_mask = None          # rows of the batch before: rebuilt by update_regex_vocab_mask

    def _neutral_penalty_rows(self, n: int, width: int):
        dev = self.temperatures.device
        return {"frequency_penalties": torch.zeros(n, dtype=torch.float, device=dev),
                "presence_penalties": torch.zeros(n, dtype=torch.float, device=dev),
                "repetition_penalties": torch.ones(n, dtype=torch.float, device=dev),
                "min_new_tokens": torch.zeros(n, dtype=torch.int32, device=dev),
                "stop_token_ids": torch.full((n, width), -1, dtype=torch.int32, device=dev),
                "req_pool_indices": torch.full((n,), -1, dtype=torch.int64, device=dev)}

    def merge_batch(self, other: "SamplingBatchInfo"):
        if self.has_penalties or other.has_penalties:
            width = max(x.stop_token_ids.shape[1] for x in (self, other) if x.has_penalties)
            sides = []
            for x in (self, other):
                rows = ({k: getattr(x, k) for k in _PENALTY_ROWS} if x.has_penalties
                        else x._neutral_penalty_rows(len(x), width))
                pad = width - rows["stop_token_ids"].shape[1]
                if pad:
                    rows["stop_token_ids"] = torch.nn.functional.pad(rows["stop_token_ids"], (0, pad), value=-1)
                sides.append(rows)
            for name in _PENALTY_ROWS:
                setattr(self, name, torch.cat([sides[0][name], sides[1][name]]))
            self.penalised_rows = ((self.penalised_rows or [False] * len(self))
                                   + (other.penalised_rows or [False] * len(other)))
            if self.penalty_state is None:
                self.penalty_state = other.penalty_state
            elif other.penalty_state is not None and other.penalty_state is not self.penalty_state:
                raise RuntimeError("merge_batch: the two batches keep their penalty histories in different pools")
        self.temperatures = torch.cat([self.temperatures, other.temperatures])
        self.top_ps = torch.cat([self.top_ps, other.top_ps])
        self.top_ks = torch.cat([self.top_ks, other.top_ks])
        self.min_ps = torch.cat([self.min_ps, other.min_ps])
        self.is_all_greedy = self.is_all_greedy and other.is_all_greedy
        self.need_min_p_sampling = self.need_min_p_sampling or other.need_min_p_sampling
        self.vocab_mask = None

    def update_regex_vocab_mask(self):
        """sampling_batch_info.py:167-190, against grammar objects that follow constrained/base_backend.py
        (allocate_vocab_mask / fill_vocab_mask / move_vocab_mask, ``finished``).  The grammar's own apply_vocab_mask
        (Triton / masked_fill_) is not taken: apply_logits_bias picks the HIP kernel by the mask's dtype."""
        if not self.grammars:
            self.vocab_mask = None
            return
        first_grammar = next(grammar for grammar in self.grammars if grammar)
        self.vocab_mask = first_grammar.allocate_vocab_mask(vocab_size=self.vocab_size, batch_size=len(self.temperatures),
                                                            device=self.device)
        for i, grammar in enumerate(self.grammars):
            if grammar and not grammar.finished:
                grammar.fill_vocab_mask(self.vocab_mask, i)
        self.vocab_mask = first_grammar.move_vocab_mask(self.vocab_mask, self.device)

    def update_penalties(self):
        """sampling_batch_info.py:144-165 builds the dense linear / scaling tensors here; the (token, count) lists are
        already on the device, so there is nothing to do."""

    def apply_logits_bias(self, logits: torch.Tensor):
        """sampling_batch_info.py:324-344, in place on fp32 logits [bs, vocab]: the penalties (sp_penalty_apply), then
        the grammar mask (sp_vocab_mask_apply).  Host tensors are refused, as by every other op."""
        if self.has_penalties:
            if self.penalty_state is None:
                raise RuntimeError("apply_logits_bias: the batch has penalties but no PenaltyState")
            self.penalty_state.apply(logits, self.vocab_size, self.req_pool_indices, self.frequency_penalties,
                                     self.presence_penalties, self.repetition_penalties, self.min_new_tokens,
                                     self.stop_token_ids)
        if self.vocab_mask is not None:
            _native.vocab_mask_apply_(logits, self.vocab_mask)

    def cumulate_output_tokens(self, output_ids: torch.Tensor):
        """Count the ids just drawn (int64 [bs], device) in their requests' histories; ids outside the vocabulary
        (the overlap worker's negative placeholders) and rows without penalties are ignored by the kernel."""
        if self.has_penalties:
            self.penalty_state.cumulate(self.req_pool_indices, output_ids.to(torch.int64), self.vocab_size)


def top_p_normalize_probs(probs: torch.Tensor, top_ps: torch.Tensor) -> torch.Tensor:
    """sampler.py:224-232"""
    return _native.top_k_top_p_min_p_renorm(probs, None, top_ps, None)


def top_k_renorm_prob(probs: torch.Tensor, top_ks: torch.Tensor) -> torch.Tensor:
    """nn/kernels/sampling.py:19-50"""
    return _native.top_k_top_p_min_p_renorm(probs, top_ks, None, None)


def top_p_renorm_prob(probs: torch.Tensor, top_ps: torch.Tensor) -> torch.Tensor:
    """nn/kernels/sampling.py:64-97"""
    return _native.top_k_top_p_min_p_renorm(probs, None, top_ps, None)


def get_top_logprobs(logprobs: torch.Tensor, top_logprobs_nums: List[int]):
    """sampler.py:235-250"""
    assert len(top_logprobs_nums) == logprobs.shape[0]
    ret = logprobs.topk(max(top_logprobs_nums), dim=1)
    values, indices = ret.values.tolist(), ret.indices.tolist()
    return ([values[i][:k] for i, k in enumerate(top_logprobs_nums)],
            [indices[i][:k] for i, k in enumerate(top_logprobs_nums)])


def get_token_ids_logprobs(logprobs: torch.Tensor, token_ids_logprobs: List[Optional[List[int]]]):
    """sampler.py:253-263"""
    vals, idxs = [], []
    for i, ids in enumerate(token_ids_logprobs):
        vals.append(logprobs[i, ids].tolist() if ids is not None else [])
        idxs.append(ids if ids is not None else [])
    return vals, idxs


class Sampler(nn.Module):
    def __init__(self, tp_group=None, use_nan_detection: bool = False):
        super().__init__()
        self.tp_group = tp_group
        self.use_nan_detection = use_nan_detection
        self.generator: Optional[torch.Generator] = None     # seedable source of the uniforms

    def forward(self, logits_output, sampling_info: SamplingBatchInfo, return_logprob: bool = False,
                top_logprobs_nums: Optional[List[int]] = None,
                token_ids_logprobs: Optional[List[Optional[List[int]]]] = None,
                uniform: Optional[torch.Tensor] = None) -> torch.Tensor:
        if sampling_info.is_all_greedy and not return_logprob and not self.use_nan_detection \
                and hasattr(logits_output, "greedy_token_ids") \
                and not getattr(sampling_info, "needs_logits_bias", False):
            # vocab-parallel greedy: no [bs, vocab] gather, no fp32 copy (LogitsProcessorOutput)
            ids = logits_output.greedy_token_ids()
            if sampling_info.grammars:
                self.sync_token_ids_across_tp(ids)
            return ids
        # every rank runs the same sampler on the same batch: the gather is an explicit collective here
        # (a batch with penalties or a vocab mask: these are the logits apply_logits_bias has been through)
        logits = (logits_output.gather_full_logits() if hasattr(logits_output, "gather_full_logits")
                  else logits_output.next_token_logits)
        if self.use_nan_detection and torch.any(torch.isnan(logits)):
            logits = torch.where(torch.isnan(logits), torch.full_like(logits, -1e5), logits)
        # return_logprob: one sp_logprobs launch over the rows the sampler has just read and one packed copy to the
        # host; SP_DEVICE_LOGPROBS=0 and top lists beyond the kernel's cap keep the dense torch passes
        on_device = (return_logprob and _native.device_logprobs_on()
                     and max(top_logprobs_nums or [0]) <= _native.LOGPROBS_MAX_TOP_K)
        logprobs = result = None
        if sampling_info.is_all_greedy:
            ids = _native.argmax(logits)
            if on_device:
                result = _native.logprobs(logits, 0, ids, top_logprobs_nums, token_ids_logprobs)
            elif return_logprob:
                logprobs = torch.nn.functional.log_softmax(logits, dim=-1)
        else:
            probs = _native.softmax_temperature_(logits, sampling_info.temperatures)
            if uniform is None:
                uniform = torch.rand(probs.shape[0], device=probs.device, generator=self.generator)
            ids = _native.top_k_top_p_min_p_sample(
                probs, sampling_info.top_ks, sampling_info.top_ps,
                sampling_info.min_ps if sampling_info.need_min_p_sampling else None, uniform)
            if on_device:
                result = _native.logprobs(probs, 1, ids, top_logprobs_nums, token_ids_logprobs,
                                          top_ps=sampling_info.top_ps)
            elif return_logprob:
                logprobs = torch.log(top_p_normalize_probs(probs, sampling_info.top_ps)).clamp(
                    min=torch.finfo(probs.dtype).min)
        want_top = bool(top_logprobs_nums) and any(x > 0 for x in top_logprobs_nums)
        want_ids = bool(token_ids_logprobs) and any(x is not None for x in token_ids_logprobs)
        if result is not None:
            if want_top or want_ids:
                top_val, top_idx, ids_val = result.lists()
                if want_top:
                    logits_output.next_token_top_logprobs_val, logits_output.next_token_top_logprobs_idx = top_val, top_idx
                if want_ids:
                    logits_output.next_token_token_ids_logprobs_val = ids_val
                    logits_output.next_token_token_ids_logprobs_idx = [x if x is not None else []
                                                                       for x in token_ids_logprobs]
            logits_output.next_token_logprobs = result.chosen
        elif return_logprob:
            if want_top:
                (logits_output.next_token_top_logprobs_val,
                 logits_output.next_token_top_logprobs_idx) = get_top_logprobs(logprobs, top_logprobs_nums)
            if want_ids:
                (logits_output.next_token_token_ids_logprobs_val,
                 logits_output.next_token_token_ids_logprobs_idx) = get_token_ids_logprobs(logprobs, token_ids_logprobs)
            logits_output.next_token_logprobs = logprobs[
                torch.arange(len(ids), device=ids.device), ids]
        if sampling_info.grammars:
            self.sync_token_ids_across_tp(ids)
        return ids

    def sync_token_ids_across_tp(self, ids: torch.Tensor):
        """sampler.py:146-157: MIN all-reduce of the drawn ids over the TP group."""
        if self.tp_group is not None and getattr(self.tp_group, "world_size", 1) > 1:
            torch.distributed.all_reduce(ids, op=torch.distributed.ReduceOp.MIN,
                                         group=self.tp_group.device_group)
