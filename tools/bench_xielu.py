#!/usr/bin/env python3
"""sp_xielu and sp_gemm_skinny_xielu at the Apertus-8B MLP shape (hidden 4096, intermediate 21504) in bf16.

1. sp_xielu at 256 and 8192 rows x 21504 against the torch composition of the same formula (softplus, where, expm1,
   minimum and the products as separate tensor operations - what XIELU.forward launches).  Bytes counted for the
   kernel: T*d read and T*d written.
2. the fused projection (one sp_gemm_skinny_xielu launch) against its two launches (sp_gemm_skinny epilogue 0, then
   sp_xielu in place) at M = 1 and 16, N = 21504, K = 4096.  Bytes counted: the N*K weight stream.

Every form is timed with device events around single launches, alternating the forms in the same process over three
rounds; the figure reported is the median.  Every repetition works on another of several buffers (activations) or
weight matrices so that no launch finds its operand in a cache the previous one filled.  Outputs are compared before
anything is timed: the fused projection with its two launches bit for bit, the kernel with the same formula evaluated
by torch in fp32 on the stored bf16 inputs, to one bf16 spacing of S, the sum of the magnitudes of the formula's terms
(the result itself crosses zero on the negative branch, so a relative bound on it would be meaningless there; the bf16
composition that is TIMED rounds after every operation and is not the yardstick).

Usage: python tools/bench_xielu.py [--out FILE]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scratchpad_amd import _native  # noqa: E402

HIDDEN, INTER, BETA, EPS = 4096, 21504, 0.5, _native.XIELU_EPS
DTYPE = torch.bfloat16


def median_us(fn, reps):
    times = []
    for i in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(i)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(times), min(times)


def torch_xielu(x, alpha_p, alpha_n, eps_t):
    ap = torch.nn.functional.softplus(alpha_p)
    an = BETA + torch.nn.functional.softplus(alpha_n)
    return torch.where(x > 0, ap * x * x + BETA * x, an * torch.expm1(torch.min(x, eps_t)) - an * x + BETA * x)


def precheck(got, x, alpha_p, alpha_n):
    """largest |got - fp32 formula| in units of 2^-7 S (one bf16 spacing of S at most): the final rounding costs half a
    spacing of the result, up to 2^-8 of its magnitude, which is at most S"""
    xf = x.float()
    ap = torch.nn.functional.softplus(alpha_p.float())
    an = BETA + torch.nn.functional.softplus(alpha_n.float())
    em1 = torch.expm1(torch.clamp(xf, max=EPS))
    pos = xf > 0
    want = torch.where(pos, ap * xf * xf + BETA * xf, an * em1 - an * xf + BETA * xf)
    S = torch.where(pos, ap * xf * xf + BETA * xf.abs(), an * (em1.abs() + xf.abs()) + BETA * xf.abs())
    return float(((got.float() - want).abs() / (2.0 ** -7 * S)).max())


def alternate(forms, reps, warmup):
    for i in range(warmup):
        for _, fn in forms:
            fn(i)
    torch.cuda.synchronize()
    res = {}
    for _round in range(3):
        for name, fn in forms:
            res.setdefault(name, []).append(median_us(fn, reps))
    return ({k: statistics.median(m for m, _ in v) for k, v in res.items()},
            {k: min(m for _, m in v) for k, v in res.items()})


def scalars():
    return (torch.tensor([0.25], device="cuda", dtype=DTYPE), torch.tensor([-1.0], device="cuda", dtype=DTYPE))


def bench_activation(T, reps, warmup, nbuf):
    g = torch.Generator(device="cuda").manual_seed(T)
    bufs = [torch.randn(T, INTER, generator=g, device="cuda").to(DTYPE) for _ in range(nbuf)]
    out = torch.empty_like(bufs[0])
    ap, an = scalars()
    eps_t = torch.tensor(EPS, device="cuda", dtype=DTYPE)
    got = _native.xielu(bufs[0], ap, an, BETA, EPS)
    dev = precheck(got, bufs[0], ap, an)
    if dev > 1.0:
        raise SystemExit(f"T={T}: sp_xielu is {dev:.3f} bf16 spacings of S away from the fp32 evaluation")
    med, low = alternate([("kernel", lambda i: _native.xielu(bufs[i % nbuf], ap, an, BETA, EPS, out=out)),
                          ("torch", lambda i: torch_xielu(bufs[i % nbuf], ap, an, eps_t))], reps, warmup)
    nbytes = 2 * 2 * T * INTER
    return (f"sp_xielu T={T:5d} x {INTER} bf16: kernel {med['kernel']:8.2f} us (min {low['kernel']:.2f}, "
            f"{nbytes / med['kernel'] / 1e6:.3f} TB/s of {nbytes / 1e6:.1f} MB read + written)  torch composition "
            f"{med['torch']:8.2f} us  kernel/torch {med['kernel'] / med['torch']:.3f}")


def bench_projection(M, reps, warmup, nw):
    g = torch.Generator(device="cuda").manual_seed(M)
    ws = [(torch.randn(INTER, HIDDEN, generator=g, device="cuda") * 0.02).to(DTYPE) for _ in range(nw)]
    x = torch.randn(M, HIDDEN, generator=g, device="cuda").to(DTYPE)
    ap, an = scalars()
    lib, st, dt = _native.load(), torch.cuda.current_stream().cuda_stream, _native.SP_BF16
    one = torch.empty(M, INTER, device="cuda", dtype=DTYPE)
    two = torch.empty(M, INTER, device="cuda", dtype=DTYPE)

    def fused(i):
        w = ws[i % nw]
        lib.sp_gemm_skinny_xielu(one.data_ptr(), x.data_ptr(), w.data_ptr(), M, INTER, HIDDEN, HIDDEN, HIDDEN, INTER,
                                 ap.data_ptr(), an.data_ptr(), BETA, EPS, dt, st)

    def two_launches(i):
        w = ws[i % nw]
        lib.sp_gemm_skinny(two.data_ptr(), x.data_ptr(), w.data_ptr(), M, INTER, HIDDEN, HIDDEN, HIDDEN, INTER, 0, dt, st)
        lib.sp_xielu(two.data_ptr(), two.data_ptr(), ap.data_ptr(), an.data_ptr(), BETA, EPS, M, INTER, INTER, INTER,
                     dt, st)

    fused(0), two_launches(0)
    torch.cuda.synchronize()
    if not torch.equal(one, two):
        raise SystemExit(f"M={M}: the fused projection and its two launches differ")
    med, low = alternate([("fused", fused), ("two", two_launches)], reps, warmup)
    wbytes = 2 * INTER * HIDDEN
    return (f"up_proj + xIELU M={M:2d} N={INTER} K={HIDDEN} bf16: fused {med['fused']:7.2f} us (min {low['fused']:.2f}, "
            f"{wbytes / med['fused'] / 1e6:.3f} TB/s of weights)  two launches {med['two']:7.2f} us (min {low['two']:.2f})  "
            f"fused/two {med['fused'] / med['two']:.3f}  [{'ok: no slower' if med['fused'] <= med['two'] else 'SLOWER'}]")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the result lines to this file")
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_xielu.py needs the GPU: a CPU timing says nothing about these kernels")
    lines = [f"# tools/bench_xielu.py on {torch.cuda.get_device_name(0)}: medians of {args.reps} event-timed launches "
             f"x 3 alternating rounds, {args.warmup} warm-up launches per form"]
    for T, nbuf in ((256, 8), (8192, 3)):
        lines.append(bench_activation(T, args.reps, args.warmup, nbuf))
        print(lines[-1], flush=True)
    for M in (1, 16):
        lines.append(bench_projection(M, args.reps, args.warmup, 4))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
