"""tests/penalty_oracle.py (the CPU statement the penalty / vocab-mask kernels are held to) reproduces
tests/golden/penalties.npz: what the reference's own penalizers, apply_logits_bias, Triton bitmask kernel and
outlines mask made of the recorded inputs (tests/golden/gen_golden_penalties.py).

Bounds (derived in penalty_oracle.tolerance): |diff| <= c^2 u |f| + 3 u max(|x|, c |f| + |p|) per touched element,
u = 2^-24, the first term dropped for penalties that are exact in binary; -inf positions equal; untouched columns
bit-identical to the input."""
import numpy as np
import pytest

from tests import golden, penalty_oracle as po

G = golden.load("penalties")


def _stops(a):
    return [[int(s) for s in row if s >= 0] for row in a]


@pytest.mark.parametrize("key", [f"orch{i}_{w}" for i in range(int(G["orch_cases"])) for w in ("mid", "fin")])
def test_orchestrator_runs(key):
    x, want = G[key + "_logits_in"], G[key + "_logits_out"]
    hist, freq, pres, min_new = G[key + "_history"], G[key + "_freq"], G[key + "_pres"], G[key + "_min_new"]
    got = po.apply_penalties(x, hist, freq, pres, None, min_new, _stops(G[key + "_stops"]))
    tol = po.tolerance(x, hist, freq, pres)
    po.check_against(got, want, x, tol, key)


def test_fixture_covers_the_cases_it_is_there_for():
    """repeated tokens, rows with and without penalties, both signs, a step exactly at out_len == min_new_tokens,
    stop ids still masked and already released, 1 to 3 stop ids"""
    seen = set()
    for key in [f"orch{i}_{w}" for i in range(int(G["orch_cases"])) for w in ("mid", "fin")]:
        hist, freq, pres, min_new = G[key + "_history"], G[key + "_freq"], G[key + "_pres"], G[key + "_min_new"]
        lens = [sum(po.counts_of(h).values()) for h in hist]
        assert max(max(po.counts_of(h).values()) for h in hist) >= 2, key
        assert G[key + "_logits_in"].shape[0] <= 8
        seen |= {"neutral"} if any(f == 0 and p == 0 and m == 0 for f, p, m in zip(freq, pres, min_new)) else set()
        seen |= {"at"} if any(m > 0 and n == m for n, m in zip(lens, min_new)) else set()
        seen |= {"masked"} if any(n < m for n, m in zip(lens, min_new)) else set()
        seen |= {"released"} if any(0 < m < n for n, m in zip(lens, min_new)) else set()
        seen |= {"f<0"} if (freq < 0).any() else set()
        seen |= {"p<0"} if (pres < 0).any() else set()
        seen |= {f"stops{int((row >= 0).sum())}" for row in G[key + "_stops"]}
    assert seen >= {"neutral", "at", "masked", "released", "f<0", "p<0", "stops1", "stops2", "stops3"}, seen


def test_exact_penalties_agree_to_the_last_bit_of_the_bound():
    """for f in {0.5, -0.25, 1.5} c * f is exact on both sides: the c^2 u |f| term is not granted"""
    key = "orch3_fin"
    x, hist, freq, pres = G[key + "_logits_in"], G[key + "_history"], G[key + "_freq"], G[key + "_pres"]
    tol = po.tolerance(x, hist, freq, pres)
    rows = [r for r, f in enumerate(freq) if f in (0.5, -0.25, 1.5)]
    assert rows
    for r in rows:
        for t, c in po.counts_of(hist[r]).items():
            assert tol[r, t] <= 3 * po.U * max(abs(x[r, t]), c * abs(float(freq[r])) + abs(float(pres[r]))) * (1 + 1e-6)


@pytest.mark.parametrize("ci", [0, 1])
def test_apply_logits_bias_with_repetition(ci):
    key = f"bias{ci}"
    x, want = G[key + "_logits_in"], G[key + "_logits_out"]
    hist, freq, pres, rep = G[key + "_history"], G[key + "_freq"], G[key + "_pres"], G[key + "_rep"]
    got = po.apply_penalties(x, hist, freq, pres, rep)
    tol = po.tolerance(x, hist, freq, pres, rep)
    po.check_against(got, want, x, tol, key)
    assert (got != x).any()
    if ci == 0:      # repetition alone: one correctly rounded operation on both sides - the same bits
        assert np.array_equal(got.view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("ci", range(int(G["bitmask_cases"])))
def test_packed_bitmask(ci):
    key = f"bitmask{ci}"
    x, mask, want = G[key + "_logits_in"], G[key + "_mask"], G[key + "_logits_out"]
    got = po.apply_bitmask(x, mask)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    limit = min(x.shape[1], 32 * mask.shape[1])
    assert np.array_equal(got[:, limit:].view(np.int32), x[:, limit:].view(np.int32))


def test_bitmask_cases_cover_short_and_ragged_widths():
    shapes = {(G[f"bitmask{i}_logits_in"].shape[1], G[f"bitmask{i}_mask"].shape[1]) for i in range(int(G["bitmask_cases"]))}
    assert any(v % 32 == 0 and w == v // 32 for v, w in shapes)
    assert any(w == (v + 31) // 32 - 1 for v, w in shapes)
    assert any(v % 32 != 0 and w == (v + 31) // 32 for v, w in shapes)
    with pytest.raises(ValueError, match="too large"):
        po.apply_bitmask(np.zeros((1, 64), np.float32), np.zeros((1, 3), np.int32))


def test_bool_mask():
    x, mask, want = G["boolmask_logits_in"], G["boolmask_mask"], G["boolmask_logits_out"]
    got = po.apply_bool_mask(x, mask)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert np.array_equal(np.isneginf(got), mask)
