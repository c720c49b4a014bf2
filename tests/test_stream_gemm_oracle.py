"""tests/stream_gemm_oracle.py can see the defects it is for (CPU).

For every reduction length of the matrix, both dtypes and each of the three statements, the fp64 products of the seeded
operands are damaged the way a wrong index in csrc/stream_gemm.h would damage them, rounded as the kernel rounds, and
the derived bound has to reject the result: at least one element outside.  This is a condition on the INPUTS (x ~ N(0,
1), w ~ N(0, 1) K^-1/2, the seeds of stream_gemm_oracle.operands) - the GPU tests use the same operands, so a kernel
with one of these defects cannot pass them.

The defects (a workgroup = 8 waves taking the k-steps round-robin; a lane loads 8 elements of one W row per k-step):
    fragment   one lane's 16 bytes of W of one k-step missing: 8 products of one output column
    twice      one k-step counted twice
    last       the last k-step of wave 0 dropped
    rows       two rows of the 16-row block exchanged
    wave0      the 8 partial sums folded from red[1] instead of red[0]: wave 0's k-steps missing"""
import pytest
import torch

from tests import stream_gemm_oracle as O

DEFECTS = ("fragment", "twice", "last", "rows", "wave0")
N = 40


def step(x64, w64, s):
    """the contribution of k-step s to x . w^T"""
    return x64[:, 32 * s:32 * s + 32] @ w64[:, 32 * s:32 * s + 32].T


def damaged(defect, P, x64, w64):
    steps = x64.shape[1] // 32
    P = P.clone()
    if defect == "fragment":
        s, n, q = steps // 2, 5, 2
        sl = slice(32 * s + 8 * q, 32 * s + 8 * q + 8)
        P[:, n] -= x64[:, sl] @ w64[n, sl]
    elif defect == "twice":
        P += step(x64, w64, steps // 3)
    elif defect == "last":
        P -= step(x64, w64, 8 * ((steps - 1) // 8))
    elif defect == "rows":
        P[[3, 11]] = P[[11, 3]]
    elif defect == "wave0":
        for s in range(0, steps, 8):
            P -= step(x64, w64, s)
    return P


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("K", O.K_MATRIX)
def test_the_bound_rejects_every_defect(K, dtype):
    x, w = O.operands(K, dtype)
    x64, wg64, wu64 = x.double(), w[:N].double(), w[N:].double()
    wt = (0.25 + 0.75 * torch.rand(16, generator=torch.Generator().manual_seed(K))).to(dtype).double()
    G, _, eG = O.products(x, w[:N])
    U, _, eU = O.products(x, w[N:])

    def results(defect):
        """the three statements on the gate product damaged by ``defect`` (exchanged rows take their up sums along)"""
        Gd = damaged(defect, G, x64, wg64) if defect else G
        Ud = damaged(defect, U, x64, wu64) if defect == "rows" else U
        return {"plain": O.plain_of(Gd, eG, dtype), "silu_mul": O.silu_mul_of(Gd, eG, Ud, eU, dtype),
                "down": O.down_of(Gd, eG, wt, dtype)}

    right = results(None)
    for name, (want, bound) in right.items():
        print(f"[oracle] K {K} {dtype} {name}: bound 0 on {float((bound == 0).double().mean()):.3f} of "
              f"{bound.numel()} elements, largest bound {float(bound.max()):.3e}")
    for defect in DEFECTS:
        for name, (got, _) in results(defect).items():
            want, bound = right[name]
            outside = int(((got - want).abs() > bound).sum())
            assert outside > 0, f"K {K} {dtype} {name}: the bound accepts the defect '{defect}'"


def test_the_error_model_is_the_stated_one():
    assert [O.ksteps(K) for K in O.K_MATRIX] == [1, 7, 60, 64, 73, 137]
    assert [O.depth(K) for K in O.K_MATRIX] == [41, 41, 272, 272, 338, 602]
    # an exact sum away from every rounding boundary has bound 0; one next to a boundary has the spacing
    e = torch.tensor([[1e-6]], dtype=torch.float64)
    for dtype, half in ((torch.bfloat16, 2.0 ** -8), (torch.float16, 2.0 ** -11)):
        val, b = O.plain_of(torch.tensor([[1.0 + half / 2]], dtype=torch.float64), e, dtype)
        assert float(val) == 1.0 and float(b) == 0.0
        _, b = O.plain_of(torch.tensor([[1.0 + half + 1e-7]], dtype=torch.float64), e, dtype)
        assert float(b) == 2 * half
