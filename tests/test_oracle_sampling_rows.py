"""The vectorised statement of the sampler oracle (oracle.sampling.select_rows / sample_rows / renorm_rows: one sort
and an exact uint64 cumulative sum per row) equals the loop form (select / sample / renorm, the definition) exactly:
keep mask, kept mass, drawn id, and the renormalised row bit for bit - on every row of tests/golden/sampling.npz and on
rows of every input family of tests/sampling_inputs.py at a small and at a full vocabulary.  The properties the
families promise (tie-heavy rows, intended tie counts, boundaries hit exactly, every descent level of the kernel
needed somewhere) are checked here too, on the CPU.  tests/test_gpu_sampling_rows.py relies on the fast form alone."""
import collections

import numpy as np
import pytest

from oracle import sampling as osamp
from tests import golden
from tests import sampling_inputs as si


def _assert_rows_equal_loop(case, rows=None):
    keep, totals, ids, ren = si.expected(case)
    for b in (range(case.bs) if rows is None else rows):
        k, p, m = case.loop_params(b)
        want_keep, want_total = osamp.select(case.probs[b], k, p, m)
        assert np.array_equal(keep[b], want_keep), (case.name, b)
        assert int(totals[b]) == want_total, (case.name, b)
        assert int(ids[b]) == osamp.sample(case.probs[b], k, p, m, float(case.uniform[b])), (case.name, b)
        want_ren = osamp.renorm(case.probs[b], k, p, m)
        assert np.array_equal(ren[b].view(np.uint32), want_ren.view(np.uint32)), (case.name, b)


def _spread(case, n=36):
    """n row indices spread evenly over the case (all rows of a smaller case)."""
    return sorted(set(np.linspace(0, case.bs - 1, min(n, case.bs)).astype(int).tolist()))


@pytest.mark.parametrize("use_minp", [True, False])
def test_fixture_rows_all_24(use_minp):
    g = golden.load("sampling")
    probs = g["probs"].astype(np.float32)
    assert probs.shape[0] == 24
    ms = g["min_ps"].astype(np.float32)
    for u in (g["uniform"], np.zeros(24), np.full(24, si.ONE_BELOW), np.linspace(0.01, 0.99, 24)):
        case = si.Case("fixture", probs, g["top_ks"], g["top_ps"], ms if use_minp else np.zeros_like(ms), u)
        _assert_rows_equal_loop(case)
        if not use_minp:                                     # an absent min_ps array is a zero floor
            off = si.Case("fixture", probs, g["top_ks"], g["top_ps"], None, u)
            for a, b in zip(si.expected(case), si.expected(off)):
                assert np.array_equal(a, b)


def test_loop_form_reads_bad_entries_as_zero_and_clamps_top_k():
    row = np.array([0.5, np.nan, -0.25, 0.25, -0.0, 0.0, 0.125, -np.inf], dtype=np.float32)
    keep, total = osamp.select(row, 1 << 30, 1.0, 0.0)
    assert keep.all() and total == int(osamp.fx(np.float32([0.5, 0.25, 0.125])).sum())
    keep, _ = osamp.select(row, 5, 1.0, 0.0)                 # 3 positive values, then the zeros by id: 1 and 2
    assert np.flatnonzero(keep).tolist() == [0, 1, 2, 3, 6]
    assert np.array_equal(osamp.renorm(row, 5, 1.0), np.float32([0.5, 0, 0, 0.25, 0, 0, 0.125, 0]) / np.float32(0.875))
    for k in (0, -1, -(2 ** 31)):
        keep, total = osamp.select(row, k, 1.0, 0.0)
        assert not keep.any() and total == 0 and osamp.sample(row, k, 1.0, 0.0, 0.7) == 0
    assert osamp.sample(np.full(8, np.nan, np.float32), 8, 1.0, 0.0, 0.9) == 0


@pytest.mark.parametrize("vocab", [4096, 128256])
def test_family_a_model_shaped(vocab):
    case = si.family_a(vocab, rows=40)
    _assert_rows_equal_loop(case, _spread(case))


@pytest.mark.parametrize("vocab", [32000, 128256])
def test_family_a_rows_are_tie_heavy(vocab):
    case = si.family_a(vocab)
    assert max(si.distinct_values(case)) < vocab / 8


@pytest.mark.parametrize("tiny", [False, True])
@pytest.mark.parametrize("vocab", [1, 2, 65, 1025, 3072, 128256])
def test_family_b_plateaus(vocab, tiny):
    case, intended, n_top = si.family_b(vocab, tiny)
    _assert_rows_equal_loop(case, _spread(case))
    keep, totals, ids, _ = si.expected(case)
    assert np.array_equal(keep.sum(-1), n_top + intended), "the cut keeps the number of ties it was built for"
    assert bool(keep[np.arange(case.bs), ids][totals > 0].all())


@pytest.mark.parametrize("vocab", si.VOCAB_SIZES)
def test_family_b_hits_the_top_p_boundary_exactly_and_misses_it_by_one_step(vocab):
    """Among the top_p cuts: fx(top_p) equals the exclusive mass of the last kept token on some rows (the boundary
    of 'exclusive mass <= fx(top_p)' hit exactly) and, on the tiny rows, is one unit below the exclusive mass of the
    first dropped token on others.  The draws land on the first kept tie, the last kept tie and the last token above
    the plateau."""
    for tiny in (False, True):
        case, intended, n_top = si.family_b(vocab, tiny)
        keep, _, ids, _ = si.expected(case)
        exact = short = 0
        for b in range(case.bs):
            if case.top_ks[b] != si.K_ALL:
                continue
            p = osamp.clean(case.probs[b])
            order = np.lexsort((np.arange(vocab), -p.view(np.uint32).astype(np.int64)))
            excl = np.cumsum(osamp.fx(p[order]), dtype=np.uint64) - osamp.fx(p[order])
            top_p_fx = int(np.floor(np.float64(case.top_ps[b]) * osamp.FX_ONE))
            n = int(keep[b].sum())
            exact += n > 0 and int(excl[n - 1]) == top_p_fx
            short += n < vocab and int(excl[n]) == top_p_fx + 1
        if vocab == 1:
            continue       # a one-token row has no top_p boundary: its token has exclusive mass 0 and is always kept
        assert exact > 0, "some top_p cut has fx(top_p) == the exclusive mass of its last kept token"
        if tiny:           # one unit of fx is within a fp32 top_p's reach only on the rows scaled by 2^-24
            assert short > 0, "some top_p cut is one unit short of the exclusive mass of its first dropped token"
        ties = [set(ids[(intended == t) & (intended > 0)].tolist()) for t in set(intended.tolist())]
        assert vocab < 64 or any(len(s) == 3 for s in ties), "first tie, last tie and a token above are all drawn"


@pytest.mark.parametrize("vocab", [4096, 128256])
def test_family_c_neighbouring_floats(vocab):
    case = si.family_c(vocab)
    _assert_rows_equal_loop(case, _spread(case))
    levels = collections.Counter(si.cut_levels(case))
    assert levels["level2"] > 0 and levels["level1"] > 0, levels
    keep, _, _, _ = si.expected(case)
    one_digit = [b for b in range(case.bs)
                 if np.unique(case.probs[b][keep[b]].view(np.uint32) >> 21).size == 1 and keep[b].sum() > 1]
    assert len(one_digit) >= 12, "rows whose kept tokens share one level-0 digit"


@pytest.mark.parametrize("with_minp", [True, False])
@pytest.mark.parametrize("vocab", [64, 1000, 128256])
def test_family_d_zeros_denormals_bad_entries(vocab, with_minp):
    case = si.family_d(vocab, with_minp)
    _assert_rows_equal_loop(case)
    keep, totals, ids, ren = si.expected(case)
    assert np.isfinite(ren).all() and (ren >= 0).all()
    assert (totals == 0).sum() >= 4 and bool((ids[totals == 0] == 0).all())
    # rows whose kept mass is fx(top_p) exactly and whose remaining tokens hold several zero-mass patterns: all kept
    tails = []
    for b in range(case.bs):
        p, (k, top_p, m) = osamp.clean(case.probs[b]), case.params(b)
        mass = int(osamp.fx(p).sum(dtype=np.uint64))
        zero_mass = np.unique(p[osamp.fx(p) == 0])
        if k == si.K_ALL and not m and mass and mass == int(np.floor(np.float64(np.float32(top_p)) * osamp.FX_ONE)) \
                and zero_mass.size >= 3 and np.unique(zero_mass.view(np.uint32) >> 21).size >= 2:
            tails.append(b)
            assert keep[b].all() and osamp.cut_level(case.probs[b], k, top_p, m) == "keep_all", b
    assert len(tails) >= 8, "exact_boundary_zero_mass_tail rows: top_p = 1.0 and below, one-hot and several heads"
    assert {float(case.top_ps[b]) for b in tails} >= {1.0, 0.75}
    if vocab == 128256 and not with_minp:
        over = [b for b in range(case.bs) if int(osamp.fx(osamp.clean(case.probs[b])).sum(dtype=np.uint64)) > 2 ** 48]
        assert over and all(0 < keep[b].sum() < vocab for b in over), "top_p = 1.0 cuts a row whose fx sum is above fx(1)"


@pytest.mark.parametrize("vocab", [1000, 32000])
def test_family_f_parameter_edges(vocab):
    cases = si.family_f(vocab)
    assert cases[0].bs == 8 * 3 * 3 * 3
    _assert_rows_equal_loop(cases[0], _spread(cases[0], 48))
    for case in cases[1:]:
        _assert_rows_equal_loop(case, _spread(case, 12))
    keep, totals, ids, _ = si.expected(cases[0])
    nothing = cases[0].top_ks <= 0
    assert nothing.sum() == 3 * 27 and not keep[nothing].any() and not ids[nothing].any()


def test_family_g_position_independence_inputs():
    cases, positions = si.family_g(4096, batches=(1, 257))
    assert [c.bs for c in cases] == [1, 257, 257, 257] and positions == [0, 0, 128, 256]
    probe = cases[0].probs[0]
    for case, at in zip(cases, positions):
        assert np.array_equal(case.probs[at], probe)
        _assert_rows_equal_loop(case, _spread(case, 12))
    assert not np.array_equal(cases[1].probs[1], cases[2].probs[1]), "different neighbours"


def test_every_descent_level_is_needed_somewhere():
    """Counted from the oracle side (oracle.sampling.cut_level): rows whose cut the kernel can only find at level 0,
    level 1, level 2 of its radix descent, and rows it keeps whole."""
    levels = collections.Counter()
    for case in (si.family_a(32000, rows=16), si.family_b(3073)[0], si.family_c(4096), si.family_d(1000, True),
                 si.family_f(1000)[0]):
        levels.update(si.cut_levels(case))
    assert all(levels[k] > 0 for k in ("keep_all", "level0", "level1", "level2")), levels


def test_softmax_reference_is_the_float64_softmax_of_the_fp32_quotient():
    import torch
    logits, temps = si.softmax_logits(1025, 8)
    assert torch.equal(logits, logits.to(torch.bfloat16).float()) and float(logits.abs().max()) == 60.0
    want = si.softmax_float64(logits, temps)
    assert torch.allclose(want.sum(-1), torch.ones(8), atol=1e-6)
    assert torch.allclose(want, osamp.softmax_temperature(logits, temps), rtol=1e-5, atol=1e-12)
