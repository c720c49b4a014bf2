"""The sort-free sampler (csrc/sampling.hip: select_cut, segment_totals, select_kernel<SAMPLE | RENORM>,
softmax_temperature_kernel) against its exact oracle on EVERY row of the input families of tests/sampling_inputs.py:
tie-heavy model-shaped rows, tie plateaus across the wave-segment and 64-lane chunk edges, clusters of neighbouring
floats (levels 1 and 2 of the radix descent), zeros / denormals / bad entries, the vocabulary sizes around the segment
rounding, the parameter edges of the C ABI, and the same row at different places of different batches.
Ids, keep counts and supports are exact; renormalised values are one fp32 division (rtol 2e-7).
tests/test_oracle_sampling_rows.py proves, on the CPU, that the vectorised oracle used here equals the loop form."""
import numpy as np
import pytest
import torch

from oracle import sampling as osamp
from tests import sampling_inputs as si

pytestmark = pytest.mark.gpu

PAD = 3.0          # strided rows: the padding holds a value larger than any probability


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(case, probs_dev):
    from scratchpad_amd import _native
    ks, ps, ms, u = _dev(case.top_ks), _dev(case.top_ps), _dev(case.min_ps), _dev(case.uniform)
    ids, cnt = _native.top_k_top_p_min_p_sample(probs_dev, ks, ps, ms, u, return_keep_count=True)
    ren, rcnt = _native.top_k_top_p_min_p_renorm(probs_dev, ks, ps, ms, return_keep_count=True)
    return ids.cpu().numpy(), cnt.cpu().numpy(), ren.cpu().numpy(), rcnt.cpu().numpy()


def check_case(case, strided=False):
    """Every row of the case: sample + renorm, twice, contiguous (and as a strided view), against the oracle."""
    keep, totals, want_ids, want_ren = si.expected(case)
    views = [_dev(case.probs)]
    if strided:
        wide = torch.full((case.bs, case.vocab + 37), PAD, dtype=torch.float32, device="cuda")
        wide[:, :case.vocab] = views[0]
        views.append(wide[:, :case.vocab])
        assert views[1].stride(0) > case.vocab
    rows = np.arange(case.bs)
    positive = osamp.clean(case.probs) > 0
    for dp in views:
        ids, cnt, ren, rcnt = _run(case, dp)
        ids2, cnt2, ren2, rcnt2 = _run(case, dp)
        assert np.array_equal(ids, ids2) and np.array_equal(cnt, cnt2) and np.array_equal(rcnt, rcnt2), case.name
        assert np.array_equal(ren.view(np.uint32), ren2.view(np.uint32)), (case.name, "two launches, different bits")
        bad = np.flatnonzero(cnt != keep.sum(-1))
        assert bad.size == 0, (case.name, "keep count", bad[:8], cnt[bad[:8]], keep.sum(-1)[bad[:8]])
        bad = np.flatnonzero(ids != want_ids)
        assert bad.size == 0, (case.name, "drawn id", bad[:8], ids[bad[:8]], want_ids[bad[:8]])
        assert bool(keep[rows, ids][totals > 0].all()), (case.name, "a dropped token was drawn")
        assert np.array_equal(rcnt, cnt), (case.name, "renorm and sample disagree on the keep count")
        # (a row whose kept mass is 0 - nothing kept, or only denormals - renormalises to zeros, as in osamp.renorm)
        bad = np.flatnonzero(((ren > 0) != (keep & positive & (totals > 0)[:, None])).any(-1))
        assert bad.size == 0, (case.name, "support", bad[:8])
        close = np.isclose(ren, want_ren, rtol=2e-7, atol=0)
        assert close.all(), (case.name, "renormalised value", np.argwhere(~close)[:4])
    return ids, cnt, ren


# --------------------------------------------------------------------------- a, e: model-shaped rows
@pytest.mark.parametrize("vocab", [128256, 32000])
def test_a_model_shaped_rows(vocab):
    case = si.family_a(vocab)
    assert max(si.distinct_values(case)) < vocab / 8, "the rows are tie-heavy (checked before any launch)"
    check_case(case, strided=True)


@pytest.mark.parametrize("vocab", si.VOCAB_SIZES)
def test_e_vocabulary_sizes_model_shaped(vocab):
    case = si.family_a(vocab, rows=16, seed="sizes")
    if vocab >= 32000:       # (a row of fewer than 8 x ~2800 tokens cannot hold 8 tokens per distinct bf16 value)
        assert max(si.distinct_values(case)) < vocab / 8
    check_case(case, strided=True)


# --------------------------------------------------------------------------- b, e: tie plateaus
@pytest.mark.parametrize("tiny", [False, True])
@pytest.mark.parametrize("vocab", si.VOCAB_SIZES)
def test_b_e_tie_plateaus(vocab, tiny):
    case, intended, n_top = si.family_b(vocab, tiny)
    _, cnt, _ = check_case(case, strided=True)
    assert np.array_equal(cnt, n_top + intended)


# --------------------------------------------------------------------------- c: neighbouring floats
@pytest.mark.parametrize("vocab", [4096, 128256])
def test_c_neighbouring_floats(vocab):
    check_case(si.family_c(vocab))


# --------------------------------------------------------------------------- d: zeros, denormals, bad entries
@pytest.mark.parametrize("with_minp", [True, False])
@pytest.mark.parametrize("vocab", [64, 1000, 128256])
def test_d_zeros_denormals_bad_entries(vocab, with_minp):
    case = si.family_d(vocab, with_minp)
    _, _, ren = check_case(case, strided=True)
    # regression (renorm_kept_bad_entry): a kept NaN / negative entry used to be divided through and written back
    assert np.isfinite(ren).all() and (ren >= 0).all()


def test_d_renorm_kept_bad_entry_is_zero():
    """The named regression row: keep-all over a row with NaN, negative and -inf entries."""
    from scratchpad_amd import _native
    row = np.array([[0.5, np.nan, -0.25, 0.25, -0.0, 0.0, 0.125, -np.inf] * 9], dtype=np.float32)
    for ks in (None, np.array([1 << 30], dtype=np.int32), np.array([30], dtype=np.int32)):
        got, cnt = _native.top_k_top_p_min_p_renorm(_dev(row), _dev(ks), None, None, return_keep_count=True)
        want = np.where(row > 0, row, 0) / np.float32(0.875 * 9)
        assert np.allclose(got.cpu().numpy(), want, rtol=2e-7, atol=0)
        assert int(cnt[0]) == (72 if ks is None or ks[0] > 72 else 30)


# --------------------------------------------------------------------------- f: parameter edges
@pytest.mark.parametrize("vocab", [1000, 32000])
def test_f_parameter_edges_and_null_pointers(vocab):
    for case in si.family_f(vocab):
        check_case(case)


# --------------------------------------------------------------------------- g: position independence
@pytest.mark.parametrize("vocab,batches", [(32000, (1, 257, 1024)), (128256, (1, 257))])
def test_g_same_row_same_result_anywhere_in_any_batch(vocab, batches):
    cases, positions = si.family_g(vocab, batches)
    seen = None
    for case, at in zip(cases, positions):
        ids, cnt, ren = check_case(case)
        here = (int(ids[at]), int(cnt[at]), ren[at].view(np.uint32).copy())
        if seen is not None:
            assert here[0] == seen[0] and here[1] == seen[1], (case.name, "id / keep count moved with the position")
            assert np.array_equal(here[2], seen[2]), (case.name, "renormalised row moved with the position")
        seen = here


# --------------------------------------------------------------------------- softmax_temperature_
@pytest.mark.parametrize("vocab", si.VOCAB_SIZES)
def test_softmax_temperature_against_float64(vocab):
    """float64 softmax of the fp32 quotient logits / T, rounded to fp32; bf16-valued logits up to +-60, T 0.05 .. 4,
    contiguous and strided rows, with and without a temperature array.  The bar is that of
    test_gpu_sampling.test_softmax_temperature_matches_oracle."""
    from scratchpad_amd import _native
    rows = 16 if vocab < 32000 else 8
    logits, temps = si.softmax_logits(vocab, rows)
    want = si.softmax_float64(logits, temps)
    got = _native.softmax_temperature_(logits.clone().cuda(), temps.cuda()).cpu()
    wide = torch.full((rows, vocab + 5), 1e4)
    wide[:, :vocab] = logits
    wide = wide.cuda()
    got_strided = _native.softmax_temperature_(wide[:, :vocab], temps.cuda().view(-1, 1)).cpu()
    assert bool((wide[:, vocab:] == 1e4).all()), "the padding of a strided row is left alone"
    for g in (got, got_strided):
        rel = torch.where(want > 1e-7, (g - want).abs() / want, torch.zeros(()))      # (atol is nothing up there)
        print(f"softmax vocab {vocab}: worst relative error {float(rel.max()):.3e} at flat index {int(rel.argmax())}")
        assert torch.allclose(g, want, rtol=1e-5, atol=1e-12)
    assert torch.equal(got, got_strided)
    got1 = _native.softmax_temperature_(logits.clone().cuda(), None).cpu()
    assert torch.allclose(got1, si.softmax_float64(logits, torch.ones(rows)), rtol=1e-5, atol=1e-12)


# --------------------------------------------------------------------------- Sampler.forward, sampling path, logprobs
@pytest.mark.parametrize("vocab", [4096, 128256])
def test_sampler_forward_sampling_path_logprobs(vocab):
    from scratchpad_amd.llama import LogitsProcessorOutput
    from scratchpad_amd.sampler import Sampler, SamplingBatchInfo, SamplingParams
    gen = torch.Generator().manual_seed(vocab)
    params = [SamplingParams(temperature=0.8, top_p=0.9, top_k=50), SamplingParams(temperature=1.2),
              SamplingParams(temperature=0.0), SamplingParams(temperature=1.0, min_p=0.1, top_p=0.5),
              SamplingParams(temperature=0.5, top_k=5, top_p=0.5), SamplingParams(temperature=2.0, top_p=0.3),
              SamplingParams(temperature=0.3, top_p=0.95), SamplingParams(temperature=1.0, top_p=0.999, top_k=3)]
    bs = len(params)
    logits = (torch.randn(bs, vocab, generator=gen) * 3).to(torch.bfloat16).float()
    info = SamplingBatchInfo.from_params(params, vocab, "cuda")
    assert not info.is_all_greedy
    u = torch.rand(bs, generator=gen)
    nums = [0, 1, 5, 20, 3, 2, 7, 4]
    asked = [None, [0, 1, vocab - 1], None, [5], list(range(40, 60)), None, [vocab // 2], [3, 2, 1]]
    out = LogitsProcessorOutput(next_token_logits=logits.clone().cuda())
    ids = Sampler()(out, info, return_logprob=True, top_logprobs_nums=nums, token_ids_logprobs=asked,
                    uniform=u.cuda()).cpu().numpy()
    # softmax was applied in place: the filter and the logprobs are checked on the probabilities the sampler really
    # saw (an id is exact only on identical inputs); the softmax itself is held to float64 just below and in
    # test_softmax_temperature_against_float64
    probs = out.next_token_logits.cpu().numpy()
    assert np.allclose(probs, si.softmax_float64(logits, info.temperatures.cpu()).numpy(), rtol=1e-5, atol=1e-12)
    case = si.Case("sampler", probs, info.top_ks.cpu().numpy(), info.top_ps.cpu().numpy(), info.min_ps.cpu().numpy(),
                   u.numpy())
    _, _, want_ids, _ = si.expected(case)
    assert np.array_equal(ids, want_ids)
    assert ids[2] == int(logits[2].argmax()), "the greedy request inside a sampling batch"
    ren = osamp.renorm_rows(probs, None, info.top_ps.cpu().numpy(), None)      # top_k = all, min_p = 0
    lowest = np.finfo(np.float32).min
    with np.errstate(divide="ignore"):
        want = np.maximum(np.log(ren.astype(np.float64)), lowest)
    got = out.next_token_logprobs.cpu().numpy()
    assert np.isfinite(got).all() and np.allclose(got, want[np.arange(bs), ids], rtol=0, atol=1e-5)
    for b in range(bs):
        vals, idx = out.next_token_top_logprobs_val[b], out.next_token_top_logprobs_idx[b]
        assert len(vals) == len(idx) == nums[b]
        assert np.allclose(vals, np.sort(want[b])[::-1][:nums[b]], rtol=0, atol=1e-5), b
        assert np.allclose(vals, want[b, idx], rtol=0, atol=1e-5), b
        vals, idx = out.next_token_token_ids_logprobs_val[b], out.next_token_token_ids_logprobs_idx[b]
        assert idx == (asked[b] or [])
        assert np.isfinite(vals).all() and np.allclose(vals, want[b, idx], rtol=0, atol=1e-5), b
    dropped = [v for b in range(bs) for v, i in zip(out.next_token_token_ids_logprobs_val[b], asked[b] or [])
               if ren[b, i] == 0]
    assert dropped and all(v == lowest for v in dropped), "dropped tokens report finfo(float32).min"
