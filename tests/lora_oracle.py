"""Oracle of the LoRA topping kernels (sp_lora_shrink / sp_lora_expand).

The reference cannot produce golden vectors for this operation: it hands the arithmetic to
``triteia.python.ops.ldmm``, which is not part of its tree, and its manager asserts LoRA off.  The oracle is therefore
the operation's own statement evaluated in fp64 on the SAME stored 16-bit inputs:

    tmp[t, :]            = scale * (x[t, :K] . A[idx[t]])                        A[slot]: [K, S r]
    y[t, s n + c]        = y_old[t, s n + c] + tmp[t, s r:(s+1) r] . B[idx[t]][:, s n + c]     B[slot]: [r, S n]

for rows with 0 <= idx[t] < slots; every other row is left alone.  Next to each value it returns the magnitude sum the
error model is stated in (the same expression with every factor replaced by its absolute value):

    |tmp_got - tmp| <= (K + 1) 2^-23 * tmp_abs                                   tmp_abs = scale sum_k |x||A|
    |y_got - y|     <= ulp_dtype(y) / 2 + (K + r + 2) 2^-23 * y_abs             y_abs = |y_old| + sum_j tmp_abs |B|

(fp32 accumulation of K resp. r products, one multiplication by scale, one addition of y_old, one rounding to the
activation dtype).  Plain torch on the CPU; nothing here imports the package under test."""
import torch

MANT = {torch.float16: 10, torch.bfloat16: 7}
MIN_EXP = {torch.float16: -14, torch.bfloat16: -126}


def ulp(e: torch.Tensor, dtype) -> torch.Tensor:
    """spacing of `dtype` at the fp64 values e (the subnormal spacing below the smallest normal)"""
    ex = torch.floor(torch.log2(e.abs().clamp_min(1e-300))).clamp_min(MIN_EXP[dtype])
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), ex - MANT[dtype])


def live_rows(idx: torch.Tensor, slots: int) -> torch.Tensor:
    idx = idx.cpu().long()
    return (idx >= 0) & (idx < slots)


def shrink(x, A, idx, scale):
    """(tmp, tmp_abs) fp64 [T, R]; rows that are skipped hold 0 in both"""
    x64, A64 = x.cpu().double(), A.cpu().double()
    T, R = x64.shape[0], A64.shape[2]
    tmp = torch.zeros(T, R, dtype=torch.float64)
    tab = torch.zeros(T, R, dtype=torch.float64)
    live = live_rows(idx, A64.shape[0])
    for t in range(T):
        if live[t]:
            a = A64[int(idx[t])]
            tmp[t] = scale * (x64[t] @ a)
            tab[t] = abs(scale) * (x64[t].abs() @ a.abs())
    return tmp, tab


def expand(y_old, tmp, tmp_abs, B, idx, num_slices):
    """(y, y_abs) fp64 [T, S n] from fp64 tmp / tmp_abs [T, S r]; skipped rows: y = y_old, y_abs = |y_old|"""
    y = y_old.cpu().double().clone()
    yab = y.abs()
    B64 = B.cpu().double()
    r, n = B64.shape[1], B64.shape[2] // num_slices
    live = live_rows(idx, B64.shape[0])
    for t in range(y.shape[0]):
        if not live[t]:
            continue
        b = B64[int(idx[t])]
        for s in range(num_slices):
            cols = slice(s * n, (s + 1) * n)
            y[t, cols] += tmp[t, s * r:(s + 1) * r] @ b[:, cols]
            yab[t, cols] += tmp_abs[t, s * r:(s + 1) * r] @ b[:, cols].abs()
    return y, yab


def tmp_bound(tmp_abs, K):
    return (K + 1) * 2.0 ** -23 * tmp_abs


def y_bound(y, y_abs, K, r, dtype):
    return 0.5 * ulp(y, dtype) + (K + r + 2) * 2.0 ** -23 * y_abs
