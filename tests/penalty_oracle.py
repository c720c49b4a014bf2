"""CPU statement of the penalty / vocab-mask semantics the HIP kernels (csrc/penalties.hip) are held to.

fp32 numpy, every operation rounded on its own, in the kernel's order:
    x -= c * frequency;  x -= presence;  x = x > 0 ? x / repetition : x * repetition
for every distinct emitted token t with count c, then -inf at the row's stop ids while out_len < min_new_tokens.
tests/test_penalty_oracle.py holds this file to tests/golden/penalties.npz (the reference's own outputs); the GPU
tests hold the kernels to this file.  A plain module (not a conftest): the tests import it.
"""
from collections import Counter

import numpy as np

U = 2.0 ** -24      # unit round-off of fp32


def counts_of(history):
    """Counter of the tokens >= 0 of one row's history (a list, or a -1 padded array)."""
    return Counter(int(t) for t in history if int(t) >= 0)


def apply_penalties(logits, histories, freq, pres, rep=None, min_new=None, stops=None, vocab=None):
    """logits fp32 [bs, width] (not modified) -> penalised copy.  histories[r]: the tokens row r has emitted, in any
    order, with repeats (or a Counter); stops: per row, an iterable of stop ids (-1 entries ignored)."""
    x = np.array(logits, dtype=np.float32, copy=True)
    bs = x.shape[0]
    vocab = x.shape[1] if vocab is None else vocab
    one = np.float32(1.0)
    for r in range(bs):
        f, p = np.float32(freq[r]), np.float32(pres[r])
        rp = one if rep is None else np.float32(rep[r])
        cnt = histories[r] if isinstance(histories[r], Counter) else counts_of(histories[r])
        if cnt and not (f == 0 and p == 0 and rp == 1):
            toks = np.array([t for t in cnt if 0 <= t < vocab], dtype=np.int64)
            c = np.array([cnt[int(t)] for t in toks], dtype=np.float32)
            v = x[r, toks]
            v = (v - (c * f).astype(np.float32)).astype(np.float32)
            v = (v - p).astype(np.float32)
            with np.errstate(invalid="ignore", divide="ignore"):
                v = np.where(v > 0, (v / rp).astype(np.float32), (v * rp).astype(np.float32))
            x[r, toks] = v
        if min_new is not None and stops is not None and int(min_new[r]) > 0:
            if sum(cnt.values()) < int(min_new[r]):
                for s in stops[r]:
                    if 0 <= int(s) < vocab:
                        x[r, int(s)] = -np.inf
    return x


def apply_bitmask(logits, bitmask):
    """xgrammar's packed form: int32 [bs, w], bit j of word i = token 32 i + j, 1 = allowed.  Columns at or beyond
    min(width, 32 w) are left alone; w > ceil(width / 32) is refused."""
    x = np.array(logits, dtype=np.float32, copy=True)
    bs, width = x.shape
    w = bitmask.shape[1]
    if w > (width + 31) // 32:
        raise ValueError("Bitmask width too large")
    limit = min(width, 32 * w)
    bits = ((bitmask.astype(np.int64)[:, :, None] >> np.arange(32)[None, None, :]) & 1).reshape(bs, 32 * w)
    x[:, :limit][bits[:, :limit] == 0] = -np.inf
    return x


def apply_bool_mask(logits, mask):
    """outlines' form: bool [bs, width], True = forbidden."""
    x = np.array(logits, dtype=np.float32, copy=True)
    x[np.asarray(mask, dtype=bool)] = -np.inf
    return x


def tolerance(logits_in, histories, freq, pres, rep=None):
    """Per-element bound on |ours - reference| for the entry pass, fp32 [bs, width]; 0 where nothing is touched:

        |diff| <= c^2 u |f| + 3 u max(|x|, c |f| + |p|),   u = 2^-24.

    The reference adds f to an fp32 cell c times (scatter_add_) and subtracts the cell; ours multiplies c * f once.
    c additions of f accumulate at most c^2 u |f| of error (each partial sum is at most c |f|); the product has none
    of it when f is exact in binary with few bits (0.5, -0.25, 1.5: every partial sum and c * f are exact), so the
    term is dropped for such f.  The two subtractions round once each on both sides, on operands of magnitude at
    most max(|x|, c |f| + |p|) up to a factor the constant 3 absorbs.
    The same bound is held where a repetition penalty follows (`rep` only tells which rows are touched) and where
    the reference forms the linear tensor first and adds it (apply_logits_bias).  (A worst-case analysis of those two
    would allow more - one more rounding each, and a factor max(rep, 1 / rep) on what the division inherits - but
    nothing recorded from the reference comes near it: the worst touched cell of the fixture is at 0.56 of this
    bound, and repetition alone is the same bits on both sides.)"""
    x = np.asarray(logits_in, dtype=np.float64)
    tol = np.zeros_like(x)
    for r in range(x.shape[0]):
        f, p = abs(float(np.float32(freq[r]))), abs(float(np.float32(pres[r])))
        rp = 1.0 if rep is None else float(np.float32(rep[r]))
        if f == 0 and p == 0 and rp == 1.0:
            continue                    # a neutral row is not touched at all: bit-identical
        exact = float(np.float32(freq[r])) * 8 == int(float(np.float32(freq[r])) * 8)
        cnt = histories[r] if isinstance(histories[r], Counter) else counts_of(histories[r])
        for t, c in cnt.items():
            if not 0 <= t < x.shape[1]:
                continue
            tol[r, t] = (0.0 if exact else c * c * U * f) + 3 * U * max(abs(x[r, t]), c * f + p)
    return tol


def check_against(got, want, logits_in, tol, what=""):
    """got / want fp32 [bs, width]: -inf positions equal, |diff| <= tol elsewhere, and columns with tol == 0 that
    are not -inf in `want` bit-identical to the input (compared as int32)."""
    got, want, logits_in = (np.ascontiguousarray(a, dtype=np.float32) for a in (got, want, logits_in))
    ninf_w, ninf_g = np.isneginf(want), np.isneginf(got)
    assert np.array_equal(ninf_w, ninf_g), f"{what}: -inf positions differ ({int((ninf_w != ninf_g).sum())} cells)"
    fin = ~ninf_w
    with np.errstate(invalid="ignore"):
        diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    bad = fin & ~(diff <= tol)
    assert not bad.any(), (f"{what}: {int(bad.sum())} cells beyond the bound, worst {float(diff[bad].max()):.3e} "
                           f"against {float(tol[bad][np.argmax(diff[bad])]):.3e}")
    untouched = fin & (tol == 0)
    assert np.array_equal(got.view(np.int32)[untouched], logits_in.view(np.int32)[untouched]), \
        f"{what}: untouched columns are not bit-identical to the input"
    return float(np.max(np.where(fin & (tol > 0), diff / np.maximum(tol, 1e-300), 0.0), initial=0.0))
