#!/usr/bin/env python3
"""sp_embedding_pool against the sequence it replaces at the tail of an embedding pass: the final fused-add RMSNorm
over all T rows (sp_fused_add_rmsnorm), ``hidden_states[cumsum(extend_seq_lens) - 1]`` and ``F.normalize`` - the
kernels and torch ops the pass ran before the fused entry existed.  T = 8192 rows of H = 4096 in bf16, B = 1, 16 and 64
sequences of equal length.

A timed window is one pair of device events around a batch of back-to-back evaluations (--calls-fused of the one
launch, --calls-replaced of the sequence), each evaluation on the next of several (hidden_states, residual) pairs;
the figure reported is the window divided by its evaluations - the time per call in a stream of calls, launch and
host enqueue cost included, not a kernel time - as the median over the windows (the minimum beside it).  Windows of
the two forms alternate in the same process.  The pairs rotate so that the replaced form, whose norm reads and writes
all T rows, finds none of them in a cache (the pairs together exceed the 256 MiB of the last-level cache); the fused
form touches 2 B H elements per pair, which stay cached from one round to the next, as the rows a decoder has just
written would be.  The outputs of the two forms are compared before anything is timed: the norm step bit for bit,
the normalised rows to one bf16 unit.
Bytes counted: fused 2 B H read + B H written; replaced 2 T H read + 2 T H written by the norm, then the gather's and the
normalise's B H traffic (not counted: small).  Launches are counted by hand from the two forms.

Usage: python tools/bench_embedding.py [--out FILE]"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scratchpad_amd import _native  # noqa: E402

T, H, EPS = 8192, 4096, 1e-5
DTYPE = torch.bfloat16


def time_us(fn, first, calls):
    """time per call, in us, of `calls` back-to-back evaluations fn(first), fn(first + 1), ... between two events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(first, first + calls):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def bench(B, reps, warmup, nbuf, calls_fused, calls_replaced):
    g = torch.Generator(device="cuda").manual_seed(B)
    xs = [torch.randn(T, H, generator=g, device="cuda").to(DTYPE) for _ in range(nbuf)]
    rs = [torch.randn(T, H, generator=g, device="cuda").to(DTYPE) for _ in range(nbuf)]
    w = (1 + 0.1 * torch.randn(H, generator=g, device="cuda")).to(DTYPE)
    lens = torch.full((B,), T // B, dtype=torch.int32, device="cuda")
    out = torch.empty(B, H, dtype=DTYPE, device="cuda")

    def fused(i):
        _native.embedding_pool(xs[i % nbuf], lens, True, residual=rs[i % nbuf], weight=w, eps=EPS, out=out)

    def replaced(i):
        x, r = xs[i % nbuf], rs[i % nbuf]
        _native.fused_add_rmsnorm(x, r, w, EPS)                     # in place on all T rows
        pooled = x[torch.cumsum(lens, dim=0) - 1]
        return F.normalize(pooled, p=2, dim=1)

    # agreement first, on copies (the replaced form overwrites its inputs)
    x0, r0 = xs[0].clone(), rs[0].clone()
    n_f = _native.embedding_pool(x0, lens, False, residual=r0, weight=w, eps=EPS)
    e_f = _native.embedding_pool(x0, lens, True, residual=r0, weight=w, eps=EPS)
    _native.fused_add_rmsnorm(x0, r0, w, EPS)
    rows = torch.cumsum(lens, dim=0) - 1
    assert torch.equal(n_f, x0[rows]), "norm step differs"
    assert float((e_f.float() - F.normalize(x0[rows], p=2, dim=1).float()).abs().max()) <= 2.0 ** -8
    for i in range(warmup):
        fused(i)
        replaced(i)
    torch.cuda.synchronize()
    tf, tr = [], []
    for i in range(reps):
        tf.append(time_us(fused, i, calls_fused))
        tr.append(time_us(replaced, i, calls_replaced))
    eb = 2
    return dict(B=B, fused_us=statistics.median(tf), fused_min_us=min(tf), replaced_us=statistics.median(tr),
                replaced_min_us=min(tr), fused_bytes=3 * B * H * eb, replaced_bytes=4 * T * H * eb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--nbuf", type=int, default=6)
    ap.add_argument("--calls-fused", type=int, default=500)
    ap.add_argument("--calls-replaced", type=int, default=50)
    a = ap.parse_args()
    assert a.reps >= 20
    lines = [f"sp_embedding_pool vs fused_add_rmsnorm(T rows) + cumsum/index + F.normalize; T={T} H={H} bf16; "
             f"time per call, launch and host enqueue included: median (min) over {a.reps} device-event windows of "
             f"{a.calls_fused} fused / {a.calls_replaced} replaced back-to-back calls, after {a.warmup} warm-up rounds, "
             f"rotating over {a.nbuf} buffer pairs; {torch.cuda.get_device_name(0)} "
             f"({torch.cuda.get_device_properties(0).gcnArchName})",
             "launches: fused 1; replaced about 7 (norm, cumsum, sub, index, norm, clamp, divide)"]
    for B in (1, 16, 64):
        r = bench(B, a.reps, a.warmup, a.nbuf, a.calls_fused, a.calls_replaced)
        lines.append(f"B={r['B']:3d}  fused {r['fused_us']:8.1f} us (min {r['fused_min_us']:.1f}), {r['fused_bytes']} bytes   "
                     f"replaced {r['replaced_us']:8.1f} us (min {r['replaced_min_us']:.1f}), {r['replaced_bytes']} bytes   "
                     f"ratio {r['replaced_us'] / r['fused_us']:.1f}x")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
