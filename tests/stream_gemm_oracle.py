"""Oracle of the weight-streaming GEMM core (csrc/stream_gemm.h) and of the three dense statements its kernels compute
(TEST INFRASTRUCTURE ONLY; imports nothing from the package under test).

The statements, in fp64 on the SAME stored 16-bit operands, with the rounding points gemm_skinny.hip and moe.hip state
(``rnd`` = to fp32, then to the activation dtype):

    plain      out = rnd(x . w^T)                                         sp_gemm_skinny, epilogue 0
    silu_mul   h   = rnd(rnd(silu(rnd(x . wg^T))) * rnd(x . wu^T))        epilogue 1, sp_moe_gate_up
    down       tmp = rnd(rnd(h . w2^T) * weight)                          sp_moe_down

Error model (derived from the summation structure, not fitted; the style of tests/delta_oracle.py).  The products a b
of two 16-bit values are exact in fp32.  The 8 waves of a workgroup take the ceil(K / 32) k-steps round-robin, so a
wave's partial sum is ONE chain of at most ceil(ceil(K / 32) / 8) v_mfma_f32_16x16x32, each adding 32 products to the
accumulator - counted as 33 sequential fp32 roundings, the worst any internal order of the matrix core can do.  The 8
partial sums are folded in wave order from +0 (8 additions, the first exact: 7 roundings) and one rounding is spare for
the second-order terms:

    c(K) = 33 ceil(ceil(K / 32) / 8) + 8          |sum_fp32 - sum| <= c(K) 2^-23 sum|a||b|

(2^-23 per operation rather than the 2^-24 of a correctly rounded one: the bound does not lean on how the matrix core
rounds inside a step.)  Everything behind the sum is a rounding or exact in fp32, so the interval is carried through
the chain with ``rerr`` exactly as tests/moe_oracle.py does: a value v known to within e rounds to within rerr(v, e) of
rnd(v), which is ZERO unless v lies within e of a rounding boundary.  silu keeps moe_oracle's terms (slope at most 1.1,
8 2^-24 |g| for its fp32 evaluation); a product a b moves by at most ea |b| + eb |a| + ea eb.  Where no boundary is near
the bound is 0 and the kernel must match bit for bit.

Every statement comes in two forms: ``*_of`` takes the fp64 products (what tests/test_stream_gemm_oracle.py feeds
deliberately wrong ones into), the plain name takes the operands and also returns the magnitude sums."""
import math

import torch

from tests.helpers import rerr, rnd
from tests.moe_oracle import U32, silu64

K_MATRIX = (32, 224, 1920, 2048, 2336, 4384)      # 1, 7, 60, 64, 73 and 137 k-steps
SEED = 5000


def ksteps(K: int) -> int:
    return math.ceil(K / 32)


def depth(K: int) -> int:
    return 33 * math.ceil(ksteps(K) / 8) + 8


def operands(K: int, dtype, rows: int = 16, cols: int = 80, seed: int = SEED):
    """(x [rows, K] ~ N(0, 1), w [cols, K] ~ N(0, 1) K^-1/2) in ``dtype``: the seeded inputs the CPU sensitivity test
    qualifies and the GPU tests use"""
    g = torch.Generator().manual_seed(seed + K)
    x = torch.randn(rows, K, generator=g).to(dtype)
    w = (torch.randn(cols, K, generator=g) * K ** -0.5).to(dtype)
    return x, w


def products(x: torch.Tensor, w: torch.Tensor):
    """(x . w^T, sum|x||w|, the accumulation error c(K) 2^-23 sum|x||w|) in fp64: [rows of x, rows of w]"""
    x64, w64 = x.cpu().double(), w.cpu().double()
    mag = x64.abs() @ w64.abs().T
    return x64 @ w64.T, mag, depth(x64.shape[1]) * 2.0 ** -23 * mag


def plain_of(P, eP, dtype):
    return rnd(P, dtype), rerr(P, eP, dtype)


def silu_mul_of(G, eG, U, eU, dtype):
    g, eg = rnd(G, dtype), rerr(G, eG, dtype)
    u, eu = rnd(U, dtype), rerr(U, eU, dtype)
    s = silu64(g)
    es = 1.1 * eg + 8 * U32 * g.abs()
    sr, esr = rnd(s, dtype), rerr(s, es, dtype)
    prod = sr * u
    eprod = esr * u.abs() + eu * sr.abs() + esr * eu
    return rnd(prod, dtype), rerr(prod, eprod, dtype)


def down_of(D, eD, weight, dtype):
    """weight: fp64 [rows] or [rows, 1], values of the activation dtype (the product with a rounded sum is exact)"""
    wt = weight.double().reshape(-1, 1)
    d, ed = rnd(D, dtype), rerr(D, eD, dtype)
    scaled = d * wt
    return rnd(scaled, dtype), rerr(scaled, ed * wt.abs(), dtype)


def plain(x, w):
    """(value, bound, sum|x||w|) fp64 [M, N] of x [M, K] and w [N, K]"""
    P, mag, eP = products(x, w)
    return plain_of(P, eP, x.dtype) + (mag,)


def silu_mul(x, wg, wu):
    """(value, bound, gate magnitudes, up magnitudes) fp64 [M, I] of x [M, K] and the gate / up rows wg, wu [I, K]"""
    G, magG, eG = products(x, wg)
    U, magU, eU = products(x, wu)
    return silu_mul_of(G, eG, U, eU, x.dtype) + (magG, magU)


def down(h, w2, weight):
    """(value, bound, sum|h||w2|) fp64 [M, H] of h [M, I], w2 [H, I] and one routing weight per row"""
    D, mag, eD = products(h, w2)
    return down_of(D, eD, weight, h.dtype) + (mag,)


def compare(what: str, got: torch.Tensor, want: torch.Tensor, bound: torch.Tensor, K: int):
    """print the case's largest err / bound and the share of its elements whose bound is 0, then hold every element to
    its bound"""
    got = got.detach().cpu().double()
    assert got.shape == want.shape == bound.shape, (got.shape, want.shape, bound.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    err = (got - want).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300),
                        torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = int(ratio.argmax()) if ratio.numel() else 0
    top = float(ratio.flatten()[worst]) if ratio.numel() else 0.0
    share = float((bound == 0).double().mean()) if bound.numel() else 0.0
    print(f"[stream gemm] {what}: largest err/bound {top:.3f}, bound 0 on {share:.3f} of {bound.numel()} elements")
    over = err > bound
    assert not bool(over.any()), (f"{what}: {int(over.sum())} of {over.numel()} elements outside the derived bound; "
                                  f"worst at {tuple(int(i) for i in torch.unravel_index(torch.tensor(worst), err.shape))}"
                                  f", K {K}, err {float(err.flatten()[worst]):.3e}, err/bound {top:.3f}")
