"""Oracle of the delta topping kernels (sp_delta_group / sp_delta_mm).

The reference cannot produce golden vectors for this operation: it hands the arithmetic to triteia (not part of its
tree) over buffers in triteia's Marlin tile order.  The oracle is therefore the operation's own statement evaluated in
fp64 on the SAME stored values - the 16-bit x, y and scales and the integer codes, unpacked here by a restatement of the
format that shares no code with the package under test:

    y[t, n] = y_old[t, n] + scale_s[n] * sum_k x[t, k] * q_s[n, k]          s = idx[t], q = code - 8

for rows with 0 <= idx[t] < slots; every other row is left alone.  Next to each value it returns the magnitude sum the
error model is stated in (the same expression with every factor replaced by its absolute value).

Error model.  The products x q are exact in fp32 (an 11-bit by a 4-bit significand).  The kernel sums them in an order
that K alone fixes: super-steps of 256 columns dealt round-robin to 8 partial sums, a partial sum being one chain of
v_mfma_f32_16x16x32 (8 per super-step, each adding 32 products to the accumulator - counted as 33 sequential fp32
roundings, the worst any internal order of the matrix core can do), the 8 partial sums folded in order (7 additions),
one multiplication by the scale, one addition of y_old and one rounding to the activation dtype:

    c(K)            = 33 * 8 * ceil(ceil(K / 256) / 8) + 7 + 1 + 1 + 1
    |y_got - y|    <= ulp_dtype(y) / 2 + c(K) 2^-23 * y_abs          y_abs = |y_old| + |scale| sum_k |x| |q|

(2^-23 per operation rather than the 2^-24 of a correctly rounded one: the bound does not lean on how the matrix core
rounds inside a step; the spare unit in c(K) covers the second-order terms).  Plain torch on the CPU."""
import math

import torch

MANT = {torch.float16: 10, torch.bfloat16: 7}
MIN_EXP = {torch.float16: -14, torch.bfloat16: -126}


def ulp(e: torch.Tensor, dtype) -> torch.Tensor:
    """spacing of `dtype` at the fp64 values e (the subnormal spacing below the smallest normal)"""
    ex = torch.floor(torch.log2(e.abs().clamp_min(1e-300))).clamp_min(MIN_EXP[dtype])
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), ex - MANT[dtype])


def depth(K: int) -> int:
    return 33 * 8 * math.ceil(math.ceil(K / 256) / 8) + 10


def dense_codes(codes: torch.Tensor, meta: torch.Tensor) -> torch.Tensor:
    """q [..., N, K] fp64 (the integers code - 8 at the kept positions, 0 elsewhere) of codes uint8 [..., N, K / 4] and
    meta uint8 [..., N, K / 8], element by element from the format's statement"""
    c = codes.cpu().to(torch.int64)
    m = meta.cpu().to(torch.int64)
    lead, G = c.shape[:-1], c.shape[-1]
    q = torch.zeros(lead + (G, 4), dtype=torch.float64)
    for g in range(G):
        nib = (m[..., g // 2] >> (4 * (g % 2))) & 15
        p0, p1 = nib & 3, nib >> 2
        assert bool((p0 < p1).all()), "a meta nibble names two positions p0 < p1"
        q[..., g, :].scatter_(-1, p0.unsqueeze(-1), ((c[..., g] & 15) - 8).double().unsqueeze(-1))
        q[..., g, :].scatter_(-1, p1.unsqueeze(-1), ((c[..., g] >> 4) - 8).double().unsqueeze(-1))
    return q.reshape(lead + (4 * G,))


def group(indices: torch.Tensor, slots: int):
    """(slot_offsets [slots + 1], sorted_rows) of a stable host sort of the rows with an index in [0, slots)"""
    idx = [int(v) for v in indices.cpu().tolist()]
    rows = [t for s in range(slots) for t, v in enumerate(idx) if v == s]
    counts = [sum(1 for v in idx if v == s) for s in range(slots)]
    offsets = [0]
    for n in counts:
        offsets.append(offsets[-1] + n)
    return offsets, rows


def mm(y_old, x, q, scales, idx):
    """(y, y_abs) fp64 [T, N]: q fp64 [slots, N, K] from dense_codes, scales [slots, N]; skipped rows: y = y_old,
    y_abs = |y_old|"""
    y = y_old.cpu().double().clone()
    yab = y.abs()
    x64, s64 = x.cpu().double(), scales.cpu().double()
    for t in range(y.shape[0]):
        s = int(idx[t])
        if not 0 <= s < q.shape[0]:
            continue
        y[t] += s64[s] * (q[s] @ x64[t])
        yab[t] += s64[s].abs() * (q[s].abs() @ x64[t].abs())
    return y, yab


def bound(y, y_abs, K, dtype):
    return 0.5 * ulp(y, dtype) + depth(K) * 2.0 ** -23 * y_abs
