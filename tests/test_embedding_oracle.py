"""tests/embedding_oracle.py pinned to the reference before it judges the kernel: the fp64 statement of the L2 step
reproduces, bit for bit, the rows the reference's own ``Pooler(PoolingType.LAST, normalize=True)`` produced on the CPU
(tests/golden/tiny_embedding.npz) in bf16, fp16 and fp32 - the all-zero row (NaN in fp16, where 1e-12 is 0) and the
row whose norm leaves the fp16 range (zeros in fp16) included.  Then the error model's own claims on the seeded inputs
of tests/test_gpu_embedding_pool.py (tests/embedding_cases.py:pool_inputs), case by case: the order-specific interval
lies inside the any-order one, and fewer than 5 % of the 16-bit elements have a rounding boundary within reach.  The
rows of the gather form are the GPU test's own; those of the two norm forms are the statement's normed rows, which the
kernel's can leave only where its fp32 mean of squares moves a rounding (the GPU test asserts the share on its rows)."""
import pytest
import torch

from tests import embedding_cases as cases
from tests import embedding_oracle as eo


@pytest.mark.parametrize("H", [100, 256])
@pytest.mark.parametrize("name", ["bf16", "fp16", "fp32"])
def test_statement_reproduces_the_reference_pooler_bit_for_bit(H, name):
    x, lens, want = cases.pooler_case(H, name)
    got = eo.embedding_pool(x, lens, normalize=True)
    assert got.dtype == want.dtype and got.shape == want.shape == (5, H)
    assert bool(eo.same_bits(got, want).all()), int((~eo.same_bits(got, want)).sum())
    rows = eo.last_rows(lens, x.shape[0]).tolist()
    assert rows == [2, 3, 7, 9, 11]
    if name == "fp16":
        assert bool(torch.isnan(want[1]).all()), "0 / max(0, fp16(1e-12) = 0)"
        assert bool((want[2] == 0).all()) and bool((x[7] != 0).any()), "a norm beyond the fp16 range is inf"
    else:
        assert bool((want[1] == 0).all()) and bool(torch.isfinite(want).all())
        assert abs(float(want[2].double().norm()) - 1.0) < 1e-2
    lo, hi = eo.l2_interval(x[rows])
    assert bool(eo.inside(want, lo, hi).all()), "the reference's own fp32 sum lies inside the interval"


def test_last_rows_range_check():
    assert eo.last_rows(torch.tensor([3, 0, 2, 9]), 6).tolist() == [2, -1, 4, -1]
    assert eo.last_rows(torch.tensor([0, 1]), 6).tolist() == [-1, 0]
    assert eo.last_rows(torch.tensor([-2, 4]), 6).tolist() == [-1, 1]


EPS = 1e-5


@pytest.mark.parametrize("B", [1, 3, 70])
@pytest.mark.parametrize("H", [7, 100, 4096, 4104, 12288])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_few_elements_have_a_rounding_boundary_within_reach(dtype, H, B):
    """so that 'bit-equal wherever the interval is a point' covers nearly every element of every case of the GPU test"""
    x, res, w, lens = cases.pool_inputs(H, B, dtype)
    lens = torch.tensor(lens)
    forms = {"gather": eo.embedding_pool(x, lens, normalize=False),
             "plain": eo.embedding_pool(x, lens, normalize=False, weight=w, eps=EPS),
             "fused": eo.embedding_pool(x, lens, normalize=False, residual=res, weight=w, eps=EPS)}
    assert torch.equal(forms["gather"], x[eo.last_rows(lens, x.shape[0])])
    for form, n in forms.items():
        lo, hi = eo.l2_interval(n)
        lo2, hi2 = eo.l2_interval(n, any_order=True)
        assert bool(((lo >= lo2) & (hi <= hi2)).all()), "the order-specific interval lies inside the any-order one"
        share = float((~eo.is_point(lo, hi)).float().mean())
        print(f"{dtype} H={H} B={B} {form}: non-point share {share:.4f} "
              f"(any order: {float((~eo.is_point(lo2, hi2)).float().mean()):.4f})")
        assert share < 0.05, (form, share)
