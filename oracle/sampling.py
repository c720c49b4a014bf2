"""CPU oracle for the sampler (TEST INFRASTRUCTURE ONLY - see oracle/ops.py header).

Two layers, both restating nn/layers/sampler.py of the reference (paths relative to
``/root/reference/scratchpad``):

1. ``*_reference`` functions: the reference's torch formulation (sort, fp32 cumsum, masks) -
   sampler.py:195-232.  Pinned by ``tests/golden/sampling.npz`` (the reference's own functions run
   on CPU with ``torch.multinomial`` intercepted, tests/golden/gen_golden.py::gen_sampling).

2. ``select`` / ``sample`` / ``renorm``: the same filter stated WITHOUT a sort, on exact integers,
   which is the definition the HIP kernel implements bit for bit:
     * ``fx(p) = floor(p * 2^48)`` (exact in float64),
     * tokens are ranked by (p descending, token id ascending); a token is kept iff
       rank < top_k  and  sum of fx over higher-ranked tokens <= fx(top_p)  and  p >= p_max*min_p
       (fp32 product) - i.e. sampler.py:205-213 with the cumulative sum carried in integers,
     * the sample for a uniform u is the token whose half-open interval of the kept cumulative
       mass, taken in token-id order, contains ``r = min(floor(u * total), total - 1)``.
   The integer formulation removes the dependence on summation order (the reference's fp32 cumsum
   over a 128k vocabulary wobbles by ~1e-6), so every TP rank draws the same token from the same
   logits - the property sampler.py:146-157 asks of the sampling kernels.
   Bad entries are defined as the kernel defines them (``prob_bits`` in csrc/sampling.hip): NaN and
   values <= 0 rank as zero - after every positive value, among themselves by token id - and carry
   no mass; a renormalised row holds 0 where the input held one.  ``top_k <= 0`` keeps nothing (the
   kernel clamps a negative top_k to 0) and a row whose kept mass is 0 draws token 0.
   ``select_rows`` / ``sample_rows`` / ``renorm_rows`` state the same definition for a whole batch
   with one sort and an exact uint64 cumulative sum per row instead of a Python loop
   (the fx sum of a row is below 2^49); tests/test_oracle_sampling_rows.py proves the two forms equal,
   bit for bit, and the loop stays the definition.
   Layer 2 agrees with layer 1 except for tokens whose exclusive cumulative mass is within fp32
   rounding of top_p, and in the order of exactly tied probabilities (torch.sort is not stable);
   tests/test_oracle_golden.py checks both statements on the fixtures.
"""
import numpy as np
import torch

FX_BITS = 48
FX_ONE = float(2 ** FX_BITS)


# --------------------------------------------------------------------------- layer 1
def softmax_temperature(logits: torch.Tensor, temperatures: torch.Tensor) -> torch.Tensor:
    """sampler.py:71-73: logits.div_(temperatures); softmax(dim=-1) in fp32."""
    return torch.softmax(logits.float() / temperatures.float().view(-1, 1), dim=-1)


def filter_sorted_reference(probs, top_ks, top_ps, min_ps=None):
    """sampler.py:202-213: returns (probs_sort with dropped entries zeroed, probs_idx)."""
    probs_sort, probs_idx = probs.sort(dim=-1, descending=True)
    probs_sum = torch.cumsum(probs_sort, dim=-1)
    rank = torch.arange(probs.shape[-1]).view(1, -1)
    probs_sort[rank >= top_ks.view(-1, 1)] = 0.0
    probs_sort[(probs_sum - probs_sort) > top_ps.view(-1, 1)] = 0.0
    if min_ps is not None:
        thr = probs_sort[:, 0] * min_ps
        probs_sort[probs_sort < thr.view(-1, 1)] = 0.0
    return probs_sort, probs_idx


def top_p_normalize_reference(probs, top_ps):
    """sampler.py:224-232 (top_p_normalize_probs_torch)."""
    probs_sort, probs_idx = probs.sort(dim=-1, descending=True)
    probs_sum = torch.cumsum(probs_sort, dim=-1)
    probs_sort[(probs_sum - probs_sort) > top_ps.view(-1, 1)] = 0.0
    probs_sort.div_(probs_sort.sum(dim=-1, keepdim=True))
    return torch.zeros_like(probs_sort).scatter_(-1, probs_idx, probs_sort)


# --------------------------------------------------------------------------- layer 2
def fx(p: np.ndarray) -> np.ndarray:
    return np.floor(p.astype(np.float64) * FX_ONE).astype(np.uint64)


def clean(probs: np.ndarray) -> np.ndarray:
    """Bad entries (NaN, negative, -0.0) read as +0.0: no mass, ranked with the zeros."""
    p = np.asarray(probs, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(p > 0, p, np.float32(0.0))


def select(probs_row: np.ndarray, top_k: int, top_p: float, min_p: float = 0.0):
    """Keep mask (bool[vocab]) and total kept mass (python int, fixed point) of one row."""
    p = clean(probs_row)
    n = p.shape[0]
    order = np.lexsort((np.arange(n), -p.astype(np.float64)))      # p desc, id asc
    w = [int(x) for x in fx(p[order])]
    top_p_fx = int(np.floor(np.float64(np.float32(top_p)) * FX_ONE))
    thr = np.float32(p.max()) * np.float32(min_p)                  # fp32 product
    keep = np.zeros(n, dtype=bool)
    acc = 0
    for rank, (tok, wt) in enumerate(zip(order, w)):
        if rank >= top_k or acc > top_p_fx or p[tok] < thr:
            break
        keep[tok] = True
        acc += wt
    return keep, acc


def sample(probs_row: np.ndarray, top_k: int, top_p: float, min_p: float, u: float) -> int:
    keep, total = select(probs_row, top_k, top_p, min_p)
    if total == 0:
        return 0
    w = fx(clean(probs_row))
    r = int(np.floor(np.float64(np.float32(u)) * np.float64(total)))
    r = min(r, total - 1)
    acc = 0
    for tok in np.flatnonzero(keep):
        acc += int(w[tok])
        if acc > r:
            return int(tok)
    raise AssertionError("unreachable: r < total")


def renorm(probs_row: np.ndarray, top_k: int, top_p: float, min_p: float = 0.0) -> np.ndarray:
    """Kept probabilities divided by the kept mass, dropped ones zero (fp32)."""
    keep, total = select(probs_row, top_k, top_p, min_p)
    p = clean(probs_row)
    out = np.zeros_like(p)
    if total:
        out[keep] = p[keep] / np.float32(np.float64(total) / FX_ONE)
    return out


# --------------------------------------------------------------------------- layer 2, whole batches
def _param(xs, b, default):
    return default if xs is None else xs[b]


def _select_row(p: np.ndarray, top_k, top_p, min_p):
    """One row of select_rows: (keep mask, total, rank order, kept count).  p is clean()."""
    n = p.shape[0]
    bits = p.view(np.uint32).astype(np.int64)                       # positive floats order as their patterns
    order = np.lexsort((np.arange(n), -bits))                       # p desc, id asc
    ps = p[order]
    w = fx(ps)
    cum = np.cumsum(w, dtype=np.uint64)
    ok = np.ones(n, dtype=bool)
    if top_k is not None:
        ok &= np.arange(n) < max(int(top_k), 0)
    if top_p is not None:
        ok &= (cum - w) <= np.uint64(int(np.floor(np.float64(np.float32(top_p)) * FX_ONE)))
    if min_p is not None:
        ok &= ps >= ps[0] * np.float32(min_p)                       # fp32 product
    nkeep = n if ok.all() else int(np.argmin(ok))                   # the loop stops at the first failure
    keep = np.zeros(n, dtype=bool)
    keep[order[:nkeep]] = True
    return keep, (int(cum[nkeep - 1]) if nkeep else 0), order, nkeep


def select_rows(probs, top_ks=None, top_ps=None, min_ps=None):
    """select() for every row of probs [bs, vocab]: (keep bool[bs, vocab], totals uint64[bs]).
    A parameter array that is None switches that filter off, as a NULL pointer does in the C ABI."""
    probs = clean(probs)
    keep = np.zeros(probs.shape, dtype=bool)
    totals = np.zeros(probs.shape[0], dtype=np.uint64)
    for b in range(probs.shape[0]):
        keep[b], totals[b], _, _ = _select_row(probs[b], _param(top_ks, b, None), _param(top_ps, b, None),
                                               _param(min_ps, b, None))
    return keep, totals


def sample_rows(probs, top_ks, top_ps, min_ps, uniform, selected=None):
    """sample() for every row: int64[bs].  `selected` takes the result of select_rows on the same inputs."""
    probs = clean(probs)
    keep, totals = selected if selected is not None else select_rows(probs, top_ks, top_ps, min_ps)
    ids = np.zeros(probs.shape[0], dtype=np.int64)
    for b in range(probs.shape[0]):
        total = int(totals[b])
        if total == 0:
            continue
        r = min(int(np.floor(np.float64(np.float32(uniform[b])) * np.float64(total))), total - 1)
        cum = np.cumsum(np.where(keep[b], fx(probs[b]), np.uint64(0)), dtype=np.uint64)   # id order
        ids[b] = int(np.searchsorted(cum, np.uint64(r), side="right"))          # first id with cum > r
    return ids


def renorm_rows(probs, top_ks=None, top_ps=None, min_ps=None, selected=None):
    """renorm() for every row: fp32[bs, vocab]."""
    probs = clean(probs)
    keep, totals = selected if selected is not None else select_rows(probs, top_ks, top_ps, min_ps)
    out = np.zeros_like(probs)
    for b in range(probs.shape[0]):
        if totals[b]:
            out[b, keep[b]] = probs[b, keep[b]] / np.float32(np.float64(int(totals[b])) / FX_ONE)
    return out


def cut_level(probs_row, top_k=None, top_p=None, min_p=None) -> str:
    """Where the kernel's radix descent (11 + 11 + 10 bits of the fp32 pattern) has to tell tokens apart to
    find this row's cut: "keep_all" if nothing is dropped; otherwise the pivot is the pattern of the
    highest-ranked dropped token, and the deepest level whose selected digit holds more than one
    distinct pattern is "level2" (other patterns share the pivot's top 22 bits), "level1" (top 11 bits
    only) or "level0" (the pivot's patterns are alone in their level-0 digit)."""
    p = clean(probs_row)
    _, _, order, nkeep = _select_row(p, top_k, top_p, min_p)
    if nkeep == p.shape[0]:
        return "keep_all"
    bits = p.view(np.uint32)
    pivot = bits[order[nkeep]]
    ties = int((bits == pivot).sum())
    if int(((bits >> 10) == (pivot >> 10)).sum()) > ties:
        return "level2"
    if int(((bits >> 21) == (pivot >> 21)).sum()) > ties:
        return "level1"
    return "level0"
