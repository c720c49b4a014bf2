#!/usr/bin/env python3
"""The fused mixture-of-experts layer at the Mixtral-8x7B shape (8 experts top-2, hidden 4096, intermediate 14336) in
bf16, at T = 1, 16, 64 and 256 rows.

Timed behind the router projection, from the router logits to the combined output:
  fused   _native.moe_experts: sp_moe_route, sp_moe_gate_up, sp_moe_down, sp_moe_combine (five launches, capturable)
  loop    _native.moe_experts_eager: sp_moe_route, then one library product pair per expert over its gathered rows -
          the reference's formulation, which synchronises with the host and cannot be graph-replayed
and compared with the floor: the bytes of the experts ACTUALLY selected by the batch (3 I H 2 bytes each) at 8 TB/s.

Both forms are timed with device events around whole calls, alternating in the same process over three rounds; the
figure is the median.  One expert's weights (352 MB) exceed the 256 MiB Infinity Cache, so a repetition does not find
its weights cached.  Before anything is timed the fused output is compared with the loop's: the two differ by fp32
accumulation order only, and the largest deviation is reported relative to the largest output.

Usage: python tools/bench_moe.py [--out profiles/moe.txt]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scratchpad_amd import _native  # noqa: E402

E, K, HIDDEN, INTER = 8, 2, 4096, 14336
DTYPE = torch.bfloat16
HBM_BYTES_PER_US = 8e6          # 8 TB/s


def median_us(fn, reps):
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(times)


def bench(T, w13, w2, reps, warmup):
    g = torch.Generator(device="cuda").manual_seed(T)
    x = torch.randn(T, HIDDEN, generator=g, device="cuda").to(DTYPE)
    logits = (torch.randn(T, E, generator=g, device="cuda") * 2).to(DTYPE)
    forms = [("fused", lambda: _native.moe_experts(x, logits, w13, w2, K)),
             ("loop", lambda: _native.moe_experts_eager(x, logits, w13, w2, K))]
    a, b = forms[0][1](), forms[1][1]()
    torch.cuda.synchronize()
    dev = float((a.float() - b.float()).abs().max() / b.float().abs().max())
    if not dev <= 2e-2:
        raise SystemExit(f"T={T}: the fused layer is {dev:.3e} of the largest output away from the per-expert loop")
    for _ in range(warmup):
        for _, fn in forms:
            fn()
    torch.cuda.synchronize()
    res = {}
    for _round in range(3):
        for name, fn in forms:
            res.setdefault(name, []).append(median_us(fn, reps))
    med = {k: statistics.median(v) for k, v in res.items()}
    ids = _native.moe_route(logits, K)[0]
    selected = int(torch.unique(ids).numel())
    floor = selected * 3 * INTER * HIDDEN * 2 / HBM_BYTES_PER_US
    return (f"moe E={E} K={K} H={HIDDEN} I={INTER} bf16 T={T:4d}: fused {med['fused']:9.1f} us  loop {med['loop']:9.1f} us  "
            f"fused/loop {med['fused'] / med['loop']:.3f}  [{'ok' if med['fused'] <= med['loop'] else 'LOSES'}]  "
            f"{selected} experts selected: floor {floor:7.1f} us, fused/floor {med['fused'] / floor:.2f}  "
            f"(fused vs loop: {dev:.2e} of the largest output)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the result lines to this file (profiles/moe.txt)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_moe.py needs the GPU: a CPU timing says nothing about these kernels")
    g = torch.Generator(device="cuda").manual_seed(0)
    w13 = torch.empty(E, 2 * INTER, HIDDEN, device="cuda", dtype=DTYPE)
    w2 = torch.empty(E, HIDDEN, INTER, device="cuda", dtype=DTYPE)
    for e in range(E):
        w13[e] = (torch.randn(2 * INTER, HIDDEN, generator=g, device="cuda") * 0.02).to(DTYPE)
        w2[e] = (torch.randn(HIDDEN, INTER, generator=g, device="cuda") * 0.02).to(DTYPE)
    lines = [f"# tools/bench_moe.py on {torch.cuda.get_device_name(0)}: medians of {args.reps} event-timed calls x 3 "
             f"alternating rounds, {args.warmup} warm-up calls per form"]
    for T in (1, 16, 64, 256):
        lines.append(bench(T, w13, w2, args.reps, args.warmup))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
