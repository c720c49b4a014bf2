"""Float64 statement of sp_logprobs (include/scratchpad_hip.h) and the seeded rows its tests run on.  Nothing here
touches a GPU.

kind 0: value(t) = log_softmax(row)[t] in float64 of the fp32 logits.
kind 1: value(t) = log(p[t] / kept_mass) under the library's top-p filter - oracle/sampling.py's select_rows: ranks by
        (p descending, id ascending), mass as integers floor(p * 2^48) - and finfo(float32).min for a token the filter
        drops or that carries no mass.
Top-k order: by the INPUT value descending, token id ascending: np.lexsort((id, -value))."""
import hashlib

import numpy as np
import torch

from oracle import sampling as osamp

FLOOR = float(np.finfo(np.float32).min)


def _seed(*key) -> int:
    return int.from_bytes(hashlib.blake2b(repr(key).encode(), digest_size=4).digest(), "little")


def all_values(rows: np.ndarray, kind: int, top_ps=None) -> np.ndarray:
    """float64 [n, vocab]: the value of every token of every row."""
    rows = np.asarray(rows, dtype=np.float32)
    if kind == 0:
        x = rows.astype(np.float64)
        mx = x.max(axis=1, keepdims=True)
        with np.errstate(divide="ignore", invalid="ignore"):
            return x - (mx + np.log(np.exp(x - mx).sum(axis=1, keepdims=True)))
    keep, totals = osamp.select_rows(rows, None, None if top_ps is None else np.asarray(top_ps, np.float32), None)
    p = osamp.clean(rows).astype(np.float64)
    out = np.full(rows.shape, FLOOR, dtype=np.float64)
    for b in range(rows.shape[0]):
        ok = keep[b] & (p[b] > 0)
        if int(totals[b]) > 0:
            out[b, ok] = np.log(p[b, ok] / (float(int(totals[b])) / osamp.FX_ONE))
    return out


def top_order(row: np.ndarray, k: int) -> np.ndarray:
    """ids of the first k tokens by (value descending, id ascending)."""
    row = np.asarray(row, dtype=np.float32) + np.float32(0)
    return np.lexsort((np.arange(row.shape[0]), -row.astype(np.float64)))[:k]


def expected(rows, kind, top_ps, chosen, top_ks, id_lists):
    """-> (chosen values [n], per row top values, per row top ids, per row listed-id values); an id outside the
    vocabulary reports FLOOR."""
    vals = all_values(rows, kind, top_ps)
    n, vocab = vals.shape
    at = lambda b, t: vals[b, t] if 0 <= t < vocab else FLOOR
    tops = [top_order(rows[b], int(top_ks[b])) for b in range(n)]
    return (np.array([at(b, int(chosen[b])) for b in range(n)]),
            [vals[b, tops[b]] for b in range(n)], [tops[b].tolist() for b in range(n)],
            [np.array([at(b, int(t)) for t in (id_lists[b] or [])], dtype=np.float64) for b in range(n)])


def distinct_top(row: np.ndarray, k: int) -> bool:
    """are the k + 1 largest values of the row pairwise distinct (the top-k ids then do not depend on a tie rule)"""
    v = np.sort(np.asarray(row, dtype=np.float32))[::-1][:k + 1]
    return bool(np.all(np.diff(v) != 0))


# --------------------------------------------------------------------------- seeded inputs
def logit_rows(vocab: int, rows: int, seed=0) -> np.ndarray:
    """bf16-rounded N(0, 1) x 3 logits (about 2 800 distinct values: tie-heavy from vocab 32 000 up), with special
    rows where the batch has room: row 1 all equal, row 2 with -inf entries as a grammar mask leaves them (every
    third id kept), row 3 a descending ramp (every element enters the top list of its wave)."""
    g = torch.Generator().manual_seed(_seed("logprob_logits", vocab, seed))
    x = (torch.randn(rows, vocab, generator=g) * 3).to(torch.bfloat16).float().numpy()
    if rows > 1:
        x[1] = np.float32(1.25)
    if rows > 2:
        x[2, np.arange(vocab) % 3 != 0] = -np.inf
    if rows > 3:
        x[3] = np.arange(vocab, dtype=np.float32)[::-1] / np.float32(vocab)
    return x


def prob_rows(vocab: int, rows: int, seed=0):
    """-> (probabilities fp32 [rows, vocab], top_ps [rows]): fp32 softmax of logit_rows (its -inf entries become
    zeros, its equal row a plateau), top_p cycling 0.3 / 0.9 / 1.0."""
    x = torch.from_numpy(logit_rows(vocab, rows, ("probs", seed)))
    p = torch.softmax(x, dim=-1).numpy().astype(np.float32)
    return p, np.resize(np.array([0.3, 0.9, 1.0], dtype=np.float32), rows)


def requests(vocab: int, rows: int, seed=0):
    """-> (chosen int64 [rows], top_ks list, id lists): top-k cycling 20 / 0 / 1 / 5, lists empty (None), short or 20
    long, some ids repeated."""
    r = np.random.default_rng(_seed("logprob_requests", vocab, rows, seed))
    chosen = r.integers(0, vocab, rows).astype(np.int64)
    top_ks = [(20, 0, 1, 5)[(b + b // 4) % 4] for b in range(rows)]
    id_lists = []
    for b in range(rows):
        mode = (b + 1) % 3
        if mode == 0:
            id_lists.append(None)
        else:
            ids = r.integers(0, vocab, 3 if mode == 1 else 20).tolist()
            ids[-1] = ids[0]
            id_lists.append(ids)
    return chosen, top_ks, id_lists
