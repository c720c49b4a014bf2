"""Statement and error model of sp_embedding_pool (TEST INFRASTRUCTURE ONLY).

The statement, in fp64 with the rounding points of the reference's path - the decoder's final RMSNorm
(nn/layers/layernorm.py:34-51), ``Pooler(PoolingType.LAST)`` (nn/layers/pooler.py:38-50) and ``F.normalize`` on a
``dtype`` tensor:

    row_i  = extend_seq_lens[0] + ... + extend_seq_lens[i] - 1
    r      = residual ? x[row_i] + residual[row_i] : x[row_i]
    n      = weight ? round(round(r * rsqrt(mean(r^2) + eps)) * weight) : r
    out[i] = normalize ? round(n / max(round(sqrt(sum n^2)), round(1e-12))) : n

round() rounds to ``dtype``; a quotient is first an fp32 number (torch divides in fp32), which an fp64 quotient rounded
to fp32 reproduces exactly (53 >= 2 * 24 + 2 bits).  The sum of squares lives in fp32: one beyond the fp32 range is inf.
A sequence without tokens, or a row_i outside [0, T), gives zeros (the kernel's range check; the reference would raise
or wrap).  ``tests/test_embedding_oracle.py`` pins ``l2_normalize`` to the rows the reference's own Pooler produced.

Error model of the L2 step (``l2_interval``), in the manner of tests/moe_oracle.py.  The kernel evaluates the same
formula on the same ``dtype`` values n; the only thing that differs from the statement is that sum n^2 is accumulated
in fp32.  Everything behind the sum is monotone: sqrt and its two roundings, the clamp, and - per element - the
quotient and its two roundings (decreasing in the denominator for n > 0, increasing for n < 0).  So the kernel's result
lies between the statement evaluated at S (1 - delta) and at S (1 + delta), |S' - S| <= delta S being the bound on the
fp32 sum S'.  Where the two ends are the same ``dtype`` number (no rounding boundary within reach) the kernel must match
bit for bit.  Two bounds, all terms being non-negative:

  any order   delta = H 2^-24: H products and H - 1 additions, each within 2^-24 relative.  It is so wide at serving
              widths that few results are pinned: on standard-normal rows the interval is a single number for 86 % of
              the bf16 and 15 % of the fp16 elements at H = 12288 (69 % of fp16 at H = 4096), and for no fp32 element
              at any width (the sum's own last bit already moves every quotient).
  this order  delta = gamma(depth + 1), gamma(k) = k u / (1 - k u), u = 2^-24: a term passes through its product's
              rounding and at most ``depth`` additions.  The order is the one include/scratchpad_hip.h fixes by
              ``hidden`` alone - a lane adds the V elements of chunks t, t + 256, ... one after the other (V = elements
              per 16 bytes), six butterfly steps fold a wave, four additions fold the waves - so depth(H) =
              V ceil(ceil(H / V) / 256) + 10.  This interval lies inside the first, so a result inside it satisfies both;
              it is the one the tests hold the kernel to (default), and under it fewer than 5 % of the 16-bit elements
              have a boundary within reach.  (fp32 results are held to the interval alone: it is a few units in the
              last place wide, never a point.)
"""
from typing import Optional, Tuple

import torch

F32_MAX = float(torch.finfo(torch.float32).max)


def rnd(t: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """fp64 -> ``dtype`` -> fp64, through fp32 where the device holds an fp32 number first"""
    return t.to(torch.float32).to(dtype).to(torch.float64)


def last_rows(lens: torch.Tensor, num_tokens: int) -> torch.Tensor:
    """row_i per sequence, -1 where the kernel writes zeros"""
    lens = lens.to(torch.int64)
    rows = torch.cumsum(lens, 0) - 1
    bad = (lens <= 0) | (rows < 0) | (rows >= num_tokens)
    return torch.where(bad, torch.full_like(rows, -1), rows)


def _denominator(S: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """[B, 1] fp64 sums of squares -> max(round(sqrt(S)), round(1e-12)); a sum beyond the fp32 range is inf"""
    S = torch.where(S > F32_MAX, torch.full_like(S, float("inf")), S)
    norm = rnd(torch.sqrt(S), dtype)
    return torch.clamp_min(norm, float(torch.tensor(1e-12, dtype=dtype)))


def _quotient(n64: torch.Tensor, denom: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    return rnd(n64 / denom, dtype)


def l2_normalize(n: torch.Tensor) -> torch.Tensor:
    """F.normalize(n, p=2, dim=1) at its rounding points; n [B, H] in its dtype -> the same dtype"""
    n64 = n.to(torch.float64)
    return _quotient(n64, _denominator((n64 * n64).sum(1, keepdim=True), n.dtype), n.dtype).to(n.dtype)


def sum_depth(hidden: int, dtype: torch.dtype) -> int:
    """additions a term of the kernel's sum of squares passes through (see the module docstring)"""
    V = 4 if dtype == torch.float32 else 8
    chunks = -(-hidden // V)
    return V * -(-chunks // 256) + 6 + 4


def sum_delta(hidden: int, dtype: torch.dtype, any_order: bool = False) -> float:
    u = 2.0 ** -24
    if any_order:
        return hidden * u
    k = sum_depth(hidden, dtype) + 1
    return k * u / (1.0 - k * u)


def l2_interval(n: torch.Tensor, any_order: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """(lo, hi) in n's dtype, elementwise: every result an fp32 accumulation of sum n^2 can give (NaN: both ends)"""
    n64 = n.to(torch.float64)
    S = (n64 * n64).sum(1, keepdim=True)
    delta = sum_delta(n.shape[1], n.dtype, any_order)
    a = _quotient(n64, _denominator(S * (1.0 - delta), n.dtype), n.dtype)
    b = _quotient(n64, _denominator(S * (1.0 + delta), n.dtype), n.dtype)
    return torch.minimum(a, b).to(n.dtype), torch.maximum(a, b).to(n.dtype)


def inside(got: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor) -> torch.Tensor:
    """elementwise: lo <= got <= hi, or NaN where the statement is NaN"""
    g, l, h = got.double(), lo.double(), hi.double()
    return ((g >= l) & (g <= h)) | (torch.isnan(g) & torch.isnan(l) & torch.isnan(h))


def is_point(lo: torch.Tensor, hi: torch.Tensor) -> torch.Tensor:
    return (lo == hi) | (torch.isnan(lo) & torch.isnan(hi))


def same_bits(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """elementwise bit equality up to the sign of zero and the payload of NaN"""
    return (a == b) | (torch.isnan(a) & torch.isnan(b))


def rmsnorm_rows(r: torch.Tensor, weight: torch.Tensor, eps: float, dtype: torch.dtype) -> torch.Tensor:
    """the norm step of the statement on fp64 rows r (the exact x + residual) -> ``dtype`` values as fp64"""
    rs = torch.rsqrt((r * r).mean(1, keepdim=True) + eps)
    return rnd(rnd(r * rs, dtype) * weight.to(torch.float64), dtype)


def embedding_pool(x: torch.Tensor, lens: torch.Tensor, normalize: bool = True,
                   residual: Optional[torch.Tensor] = None, weight: Optional[torch.Tensor] = None,
                   eps: float = 0.0) -> torch.Tensor:
    """The whole statement on host tensors; x [T, H] in its dtype -> [B, H] in the same dtype"""
    dtype = x.dtype
    rows = last_rows(lens, x.shape[0])
    ok = rows >= 0
    idx = rows.clamp_min(0)
    r = x[idx].to(torch.float64)
    if residual is not None:
        r = r + residual[idx].to(torch.float64)
    n = rmsnorm_rows(r, weight, eps, dtype) if weight is not None else rnd(r, dtype)
    n = n.to(dtype)
    out = l2_normalize(n) if normalize else n
    return torch.where(ok[:, None], out, torch.zeros_like(out))
