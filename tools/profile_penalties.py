#!/usr/bin/env python3
"""Device time of the penalty path against the dense sequence the reference performs, in one process.

For 64 / 1 024 / 4 096 distinct emitted tokens per row at bs 256 x vocab 128 256:
  sparse:  sp_penalty_cumulate + sp_penalty_apply (frequency + presence + repetition on every row), then
           sp_vocab_mask_apply with a packed bitmask;
  dense:   what sampling_batch_info.py / penaltylib do per step, written with plain torch ops: three [bs, vocab] fp32
           passes (logits.sub_(frequency tensor), logits.sub_(presence tensor), logits.add_(min-new-token tensor)) and a
           masked_fill_ with a bool mask.

Run under `rocprofv3 --kernel-trace --stats -- python tools/profile_penalties.py [--distinct N --sparse-only]` for
per-kernel times, one run per list length for per-length statistics (the script
also prints HIP-event times per group, which include launch gaps).  Nothing is tuned for the comparison.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scratchpad_amd import _native
from scratchpad_amd.penalty_state import PenaltyState


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=256)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--distinct", type=int, nargs="*", default=[64, 1024, 4096],
                    help="list lengths to run (one per profiler run gives per-length kernel statistics)")
    ap.add_argument("--sparse-only", action="store_true", help="skip the mask kernels and the dense torch sequence")
    a = ap.parse_args()
    bs, vocab, dev = a.bs, a.vocab, "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    logits = torch.randn((bs, vocab), device=dev, generator=g) * 3
    rows = torch.randperm(bs, device=dev)
    freq = torch.full((bs,), 0.3, device=dev)
    pres = torch.full((bs,), 0.5, device=dev)
    rep = torch.full((bs,), 1.2, device=dev)
    bitmask = torch.randint(-2 ** 31, 2 ** 31 - 1, (bs, (vocab + 31) // 32), device=dev, generator=g).to(torch.int32)
    boolmask = torch.rand((bs, vocab), device=dev, generator=g) < 0.5
    dense = [torch.zeros((bs, vocab), device=dev) for _ in range(3)]
    out = {"bs": bs, "vocab": vocab, "unit": "us (HIP events, mean of %d)" % a.reps}
    for distinct in a.distinct:
        state = PenaltyState(bs, distinct + 8, dev)
        # rows already hold `distinct` tokens each (written directly: the kernels' input state)
        toks = torch.stack([torch.randperm(vocab, device=dev, generator=g)[:distinct] for _ in range(bs)]).to(torch.int32)
        state.entries[:, :distinct, 0] = toks
        state.entries[:, :distinct, 1] = 2
        state.n_distinct.fill_(distinct)
        state.out_len.fill_(2 * distinct)
        ids = toks[:, distinct // 2].to(torch.int64).contiguous()           # a token the row has: found mid-scan
        out[f"distinct_{distinct}"] = {
            "cumulate": timed(lambda: state.cumulate(rows, ids, vocab), a.reps),
            "apply": timed(lambda: state.apply(logits, vocab, rows, freq, pres, rep), a.reps),
        }
    if a.sparse_only:
        print(json.dumps(out))
        return
    out["vocab_mask_packed"] = timed(lambda: _native.vocab_mask_apply_(logits, bitmask), a.reps)
    out["vocab_mask_bool"] = timed(lambda: _native.vocab_mask_apply_(logits, boolmask), a.reps)
    out["dense_three_passes"] = timed(lambda: (logits.sub_(dense[0]), logits.sub_(dense[1]), logits.add_(dense[2])), a.reps)
    out["dense_masked_fill"] = timed(lambda: logits.masked_fill_(boolmask, float("-inf")), a.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
