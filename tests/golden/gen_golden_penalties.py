#!/usr/bin/env python3
"""Regenerate ``tests/golden/penalties.npz`` by RUNNING the upstream reference on the CPU (needs the reference tree,
see _ref_loader.py).  Data only: seeded inputs and what the reference's own code made of them.

  orch<i>_*   sampling/penaltylib: BatchedPenalizerOrchestrator over two batches - cumulate_output_tokens x steps
              (few distinct tokens, so they repeat), filter in the middle, merge, more steps, apply.  One apply is
              recorded before the merge ("mid") and one at the end ("fin"), each with the history of every row
              (padded token matrix), its parameters and its stop ids.  min_new_tokens values sit below, at and above
              the number of tokens emitted.
  bias<i>_*   SamplingBatchInfo.apply_logits_bias with a hand-built scaling_penalties (the repetition penalty at the
              emitted tokens, 1 elsewhere) alone (bias0) and together with linear_penalties made by the penalizers
              (bias1).
  bitmask<i>_*  constrained/triton_ops/bitmask_ops.py apply_token_bitmask_inplace_triton (Triton interpreter): full
              width, one word short, a vocabulary that is not a multiple of 32.
  boolmask_*  the outlines form (apply_vocab_mask of constrained/outlines_backend.py: True = forbidden).
  params_*    SamplingParams defaults and the messages verify() raises, as JSON text.

Usage: python tests/golden/gen_golden_penalties.py
"""
import json
import os
import sys
from types import SimpleNamespace

os.environ["TRITON_INTERPRET"] = "1"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_loader  # noqa: E402

_ref_loader.install()

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.set_grad_enabled(False)
import scratchpad.utils  # noqa: E402

scratchpad.utils.get_device_core_count = lambda: 0      # bitmask_ops reads it at import; 0 = one program per block

from scratchpad.sampling import penaltylib  # noqa: E402
from scratchpad.sampling.sampling_params import SamplingParams  # noqa: E402

PENALIZERS = {penaltylib.BatchedFrequencyPenalizer, penaltylib.BatchedMinNewTokensPenalizer,
              penaltylib.BatchedPresencePenalizer}


def make_req(freq, pres, min_new, stops, eos, extra):
    sp = SamplingParams(frequency_penalty=freq, presence_penalty=pres, min_new_tokens=min_new,
                        stop_token_ids=stops)
    tok = SimpleNamespace(eos_token_id=eos, additional_stop_token_ids=set(extra) if extra else None)
    req = SimpleNamespace(sampling_params=sp, tokenizer=tok, history=[])
    req.stop_set = sorted(set(stops or ()) | set(extra or ()) | {eos})
    return req


def make_batch(reqs):
    return SimpleNamespace(reqs=list(reqs), device="cpu", batch_size=lambda: len(reqs))


def step(orch, batch, g, pool):
    ids = pool[torch.randint(0, len(pool), (len(batch.reqs),), generator=g)]
    orch.cumulate_output_tokens(ids)
    for r, t in zip(batch.reqs, ids.tolist()):
        r.history.append(t)


def record(out, key, batch, orch, vocab, g):
    logits = torch.randn(len(batch.reqs), vocab, generator=g) * 3.0
    out[key + "_logits_in"] = logits.numpy().copy()
    orch.apply(logits)
    out[key + "_logits_out"] = logits.numpy().copy()
    reqs = batch.reqs
    longest = max(1, max(len(r.history) for r in reqs))
    hist = np.full((len(reqs), longest), -1, dtype=np.int64)
    for i, r in enumerate(reqs):
        hist[i, :len(r.history)] = r.history
    width = max(len(r.stop_set) for r in reqs)
    stops = np.full((len(reqs), width), -1, dtype=np.int32)
    for i, r in enumerate(reqs):
        stops[i, :len(r.stop_set)] = r.stop_set
    out[key + "_history"] = hist
    out[key + "_stops"] = stops
    out[key + "_freq"] = np.array([r.sampling_params.frequency_penalty for r in reqs], dtype=np.float32)
    out[key + "_pres"] = np.array([r.sampling_params.presence_penalty for r in reqs], dtype=np.float32)
    out[key + "_min_new"] = np.array([r.sampling_params.min_new_tokens for r in reqs], dtype=np.int32)


def gen_orchestrator(out):
    # (vocab, steps before filter, after filter, steps of B, after merge); total for a surviving A row = s1 + s2 + s4
    cases = [(300, 5, 4, 3, 6), (517, 9, 1, 7, 5), (1000, 12, 8, 2, 20), (2000, 30, 10, 25, 24)]
    for ci, (vocab, s1, s2, s3, s4) in enumerate(cases):
        g = torch.Generator().manual_seed(500 + ci)
        mid_a, fin_a, fin_b = s1 + s2, s1 + s2 + s4, s3 + s4
        eos = vocab - 1
        pool = torch.randint(0, vocab, (max(6, (s1 + s4) // 3),), generator=g)      # few distinct ids: they repeat
        pool[0] = eos                                     # a stop id that is also emitted (and penalised)
        # binary-exact penalties (0.5, -0.25, 1.5) next to inexact ones (0.3, -0.7, 1.1); rows without any penalty
        a = [make_req(0.5, 0.0, 0, None, eos, None),
             make_req(0.3, -0.25, mid_a, [3, 7], eos, None),            # mid: out_len == min_new exactly
             make_req(0.0, 0.0, 0, None, eos, None),                    # no penalty
             make_req(-0.7, 1.5, fin_a + 1, [5], eos, [11]),            # still masked at the end
             make_req(1.5, 1.1, fin_a, None, eos, None),                # fin: out_len == min_new exactly
             make_req(0.0, -1.3, fin_a - 1, [2, 4], eos, None)]         # released one step before the end
        b = [make_req(-0.25, 0.5, fin_b + 3, [9, 10, 12][:1 + ci % 3], eos, None),
             make_req(0.0, 0.0, 0, None, eos, None)]
        ba, bb = make_batch(a), make_batch(b)
        oa = penaltylib.BatchedPenalizerOrchestrator(vocab_size=vocab, batch=ba, penalizers=PENALIZERS)
        ob = penaltylib.BatchedPenalizerOrchestrator(vocab_size=vocab, batch=bb, penalizers=PENALIZERS)
        for _ in range(s1):
            step(oa, ba, g, pool)
        keep = [0, 1, 3, 4, 5] if ci % 2 == 0 else [5, 4, 3, 1]          # drops the unpenalised row (and row 0)
        ba.reqs = [ba.reqs[i] for i in keep]                             # ScheduleBatch.filter_batch: reqs first
        oa.filter(torch.tensor(keep, dtype=torch.int64))
        for _ in range(s2):
            step(oa, ba, g, pool)
        record(out, f"orch{ci}_mid", ba, oa, vocab, g)
        for _ in range(s3):
            step(ob, bb, g, pool)
        oa.merge(ob)                                                     # before reqs are merged (orchestrator.py:85)
        ba.reqs = ba.reqs + bb.reqs
        for _ in range(s4):
            step(oa, ba, g, pool)
        record(out, f"orch{ci}_fin", ba, oa, vocab, g)
    out["orch_cases"] = np.array(len(cases))


def gen_apply_logits_bias(out):
    from scratchpad.sampling.sampling_batch_info import SamplingBatchInfo
    for ci, with_linear in enumerate((False, True)):
        vocab, bs, steps = 800, 6, 17
        g = torch.Generator().manual_seed(600 + ci)
        reps = [1.5, 1.1, 1.0, 0.5, 1.7, 0.9]
        freqs = [0.5, 0.3, 0.0, -0.25, 0.0, 1.9] if with_linear else [0.0] * bs
        press = [0.0, -0.7, 0.0, 1.5, 0.25, 0.0] if with_linear else [0.0] * bs
        reqs = [make_req(f, p, 0, None, vocab - 1, None) for f, p in zip(freqs, press)]
        batch = make_batch(reqs)
        orch = penaltylib.BatchedPenalizerOrchestrator(vocab_size=vocab, batch=batch, penalizers=PENALIZERS)
        pool = torch.randint(0, vocab, (7,), generator=g)
        ids_all = pool[torch.randint(0, len(pool), (steps, bs), generator=g)]
        for s in range(steps):
            orch.cumulate_output_tokens(ids_all[s])
        scaling = torch.ones(bs, vocab)
        for r in range(bs):
            scaling[r, ids_all[:, r]] = reps[r]
        linear = None
        if with_linear:
            linear = torch.zeros(bs, vocab)
            orch.apply(linear)                    # what update_penalties means to build (its glue is broken upstream)
        info = SamplingBatchInfo(temperatures=torch.ones(bs, 1), top_ps=torch.ones(bs), top_ks=torch.ones(bs, dtype=torch.int32),
                                 min_ps=torch.zeros(bs), is_all_greedy=True, need_min_p_sampling=False,
                                 has_custom_logit_processor=False, vocab_size=vocab, linear_penalties=linear,
                                 scaling_penalties=scaling, device="cpu")
        logits = torch.randn(bs, vocab, generator=g) * 3.0
        key = f"bias{ci}"
        out[key + "_logits_in"] = logits.numpy().copy()
        info.apply_logits_bias(logits)
        out[key + "_logits_out"] = logits.numpy().copy()
        out[key + "_history"] = ids_all.t().contiguous().numpy()
        out[key + "_freq"] = np.array(freqs, dtype=np.float32)
        out[key + "_pres"] = np.array(press, dtype=np.float32)
        out[key + "_rep"] = np.array(reps, dtype=np.float32)


def gen_masks(out):
    from scratchpad.constrained.triton_ops.bitmask_ops import apply_token_bitmask_inplace_triton
    g = torch.Generator().manual_seed(700)
    for ci, (vocab, w) in enumerate(((1024, 32), (1024, 31), (1000, 32), (1000, 31), (300, 10))):
        bs = 4
        logits = torch.randn(bs, vocab, generator=g) * 3.0
        mask = torch.randint(-2 ** 31, 2 ** 31 - 1, (bs, w), generator=g, dtype=torch.int64).to(torch.int32)
        mask[0, 0] = 0                      # a word that forbids all 32
        mask[1, w - 1] = -1                 # ... and one that allows all
        key = f"bitmask{ci}"
        out[key + "_logits_in"] = logits.numpy().copy()
        out[key + "_mask"] = mask.numpy().copy()
        apply_token_bitmask_inplace_triton(logits, mask)
        out[key + "_logits_out"] = logits.numpy().copy()
    out["bitmask_cases"] = np.array(5)
    try:
        # wheels the outlines back-end imports at module level and this container may lack: stand-ins (their
        # arithmetic is not used - apply_vocab_mask is torch alone)
        _ref_loader._install_absent(["interegular", "outlines.fsm", "outlines.fsm.guide", "outlines.fsm.json_schema",
                                     "outlines.models", "outlines.models.transformers", "outlines.caching",
                                     "outlines_core", "outlines_core.fsm", "outlines_core.fsm.json_schema", "pydantic"])
        from scratchpad.constrained.outlines_backend import OutlinesGrammar
        apply_bool = OutlinesGrammar.apply_vocab_mask
    except Exception as e:      # the outlines wheel is absent and its stand-in does not carry the class
        raise RuntimeError(f"cannot reach the reference's outlines apply_vocab_mask: {e}")
    vocab, bs = 517, 5
    logits = torch.randn(bs, vocab, generator=g) * 3.0
    mask = torch.rand(bs, vocab, generator=g) < 0.6
    mask[2] = False
    out["boolmask_logits_in"] = logits.numpy().copy()
    out["boolmask_mask"] = mask.numpy().copy()
    apply_bool(logits=logits, vocab_mask=mask)
    out["boolmask_logits_out"] = logits.numpy().copy()


def gen_params(out):
    d = SamplingParams()
    out["params_defaults"] = np.array(json.dumps({k: getattr(d, k) for k in (
        "frequency_penalty", "presence_penalty", "repetition_penalty", "min_new_tokens", "stop_token_ids")}))
    out["params_stop_ids_kept_as"] = np.array(json.dumps(sorted(SamplingParams(stop_token_ids=[5, 3, 5]).stop_token_ids)))
    cases = [dict(frequency_penalty=2.5), dict(frequency_penalty=-2.01), dict(presence_penalty=3.0),
             dict(presence_penalty=-2.5), dict(repetition_penalty=-0.1), dict(repetition_penalty=2.5),
             dict(min_new_tokens=-1), dict(min_new_tokens=9, max_new_tokens=8), dict(max_new_tokens=-1),
             dict(frequency_penalty=2.0, presence_penalty=-2.0, repetition_penalty=2.0, min_new_tokens=8, max_new_tokens=8),
             dict(repetition_penalty=0.5, stop_token_ids=[1, 2])]
    res = []
    for kw in cases:
        try:
            SamplingParams(**kw).verify()
            res.append({"kwargs": kw, "error": None})
        except ValueError as e:
            res.append({"kwargs": kw, "error": str(e)})
    out["params_verify"] = np.array(json.dumps(res))


def main():
    out = {}
    gen_orchestrator(out)
    gen_apply_logits_bias(out)
    gen_masks(out)
    gen_params(out)
    path = os.path.join(HERE, "penalties.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays")


if __name__ == "__main__":
    main()
