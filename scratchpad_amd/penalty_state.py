"""Device state of the sampling penalties: per request, the distinct tokens it has emitted and how often.

The reference keeps a dense fp32 ``[bs, vocab]`` tensor per penalizer (sampling/penaltylib/penalizers/*.py), gathers
every one of them on ``filter_batch`` and concatenates them on ``merge_batch``.  Here the state is a list of
(token, count) pairs per REQUEST, in rows indexed by ``req_pool_idx`` like ``ReqToTokenPool.req_to_token``: a request
keeps its row for as long as it runs, so filtering and merging batches move nothing but the per-row scalars of
``SamplingBatchInfo``.  ``capacity`` is the pool's ``max_context_len`` - a request cannot emit more tokens than that,
so a row cannot fill up; the kernel still never writes past it and raises a sticky error word instead
(``PenaltyState.check``).  Kernels: csrc/penalties.hip.

The store belongs to a ``ReqToTokenPool`` and is created by the first batch that needs it (``penalty_state_of``): an
engine that never sees a penalised request allocates nothing.
"""
from typing import List, Optional, Sequence, Tuple

import torch

from . import _native


class PenaltyState:
    def __init__(self, pool_rows: int, capacity: int, device: str):
        self.pool_rows, self.capacity, self.device = pool_rows, capacity, device
        self.entries = torch.zeros((pool_rows, capacity, 2), dtype=torch.int32, device=device)
        self.n_distinct = torch.zeros((pool_rows,), dtype=torch.int32, device=device)
        self.out_len = torch.zeros((pool_rows,), dtype=torch.int32, device=device)
        self.error = torch.zeros((1,), dtype=torch.int32, device=device)

    def reset(self, pool_row_indices: torch.Tensor) -> None:
        """Forget the history of these pool rows (requests being admitted)."""
        _native.penalty_reset(self.n_distinct, self.out_len, pool_row_indices)

    def cumulate(self, req_pool_indices: torch.Tensor, token_ids: torch.Tensor, vocab_size: int) -> None:
        """One emitted token per row: count it in the row's list.  Ids outside [0, vocab_size) and pool rows outside
        the store (-1: a row without penalties) are ignored."""
        _native.penalty_cumulate(self.entries, self.n_distinct, self.out_len, self.error, req_pool_indices,
                                 token_ids, vocab_size)

    def apply(self, logits: torch.Tensor, vocab_size: int, req_pool_indices: torch.Tensor,
              frequency_penalties: torch.Tensor, presence_penalties: torch.Tensor,
              repetition_penalties: torch.Tensor, min_new_tokens: Optional[torch.Tensor] = None,
              stop_token_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
        return _native.penalty_apply_(logits, vocab_size, self.entries, self.n_distinct, self.out_len,
                                      req_pool_indices, frequency_penalties, presence_penalties,
                                      repetition_penalties, min_new_tokens, stop_token_ids)

    def seed(self, pool_rows: Sequence[int], histories: Sequence[Sequence[int]], vocab_size: int) -> None:
        """Reset the rows and replay each one's emitted tokens (admission: empty for a fresh request, the whole
        output for a retracted one).  One cumulate launch per position of the longest history - retraction is rare."""
        if len(pool_rows) == 0:
            return
        rows = torch.tensor(list(pool_rows), dtype=torch.int64).to(self.device, non_blocking=True)
        self.reset(rows)
        longest = max(len(h) for h in histories)
        if longest == 0:
            return
        ids = torch.full((longest, len(pool_rows)), -1, dtype=torch.int64)
        for j, h in enumerate(histories):
            if len(h):
                ids[:len(h), j] = torch.tensor(list(h), dtype=torch.int64)
        ids = ids.to(self.device, non_blocking=True)
        for step in range(longest):
            self.cumulate(rows, ids[step], vocab_size)

    def check(self) -> None:
        """Raise if a cumulate ever found a row full (synchronises: call at check points, not per step)."""
        if int(self.error.item()) != 0:
            raise RuntimeError("penalty state: a request's token list was full (more distinct output tokens than the "
                               f"pool's max_context_len = {self.capacity}); its penalties are incomplete")

    def history(self, pool_row: int) -> Tuple[List[List[int]], int]:
        """([[token, count], ...], out_len) of one pool row, read back (tests, debugging)."""
        n = int(self.n_distinct[pool_row].item())
        return self.entries[pool_row, :n].cpu().tolist(), int(self.out_len[pool_row].item())


def penalty_state_of(req_to_token_pool, create: bool = True) -> Optional[PenaltyState]:
    """The store that goes with this request pool; created on first use (``create``), else None while there is none."""
    state = getattr(req_to_token_pool, "penalty_state", None)
    if state is None and create:
        state = PenaltyState(req_to_token_pool.size, req_to_token_pool.max_context_len, req_to_token_pool.device)
        req_to_token_pool.penalty_state = state
    return state
