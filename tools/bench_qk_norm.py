#!/usr/bin/env python3
"""sp_qk_norm_rotary against the three launches it replaces (sp_rmsnorm on q's heads, sp_rmsnorm on k's heads,
sp_rotary_embedding with the fused KV store), at the Qwen3-8B head shape (32 q / 8 kv heads, head_dim 128) in bf16 on
the model's qkv layout.

Both forms are timed with device events around single launches, alternating fused / three-launch repetitions in the
same process; the figure reported is the median over the repetitions.  Every repetition works on another of several
qkv buffers so that no launch finds its rows in a cache the previous one filled.  The outputs of the two forms are
compared bit for bit before anything is timed.  Bytes counted for the fused launch: q and k read and written, v read,
the K and V pool rows written (the weights and the cos/sin rows are shared and small).

Usage: python tools/bench_qk_norm.py [--out FILE]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scratchpad_amd import _native  # noqa: E402

HQ, HKV, D, EPS, MAX_POS = 32, 8, 128, 1e-6, 8192
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


def bench(T, reps, warmup, nbuf):
    g = torch.Generator(device="cuda").manual_seed(T)
    width = (HQ + 2 * HKV) * D
    bufs = [torch.randn(T, width, generator=g, device="cuda").to(DTYPE) for _ in range(nbuf)]
    wq = (1 + 0.1 * torch.randn(D, generator=g, device="cuda")).to(DTYPE)
    wk = (1 + 0.1 * torch.randn(D, generator=g, device="cuda")).to(DTYPE)
    inv = 1.0 / (1e6 ** (torch.arange(0, D, 2, dtype=torch.float) / D))
    fr = torch.einsum("i,j->ij", torch.arange(MAX_POS, dtype=torch.float), inv)
    cache = torch.cat((fr.cos(), fr.sin()), -1).to(DTYPE).cuda()
    pos = torch.randint(0, MAX_POS, (T,), generator=g, device="cuda", dtype=torch.int64)
    loc = (torch.randperm(T + 64, generator=g, device="cuda")[:T] + 1).to(torch.int64)
    kb = torch.zeros(T + 65, HKV, D, device="cuda", dtype=DTYPE)
    vb = torch.zeros_like(kb)
    split = lambda b: b.split([HQ * D, HKV * D, HKV * D], dim=-1)
    # contiguous q / k for the three-launch form's norms: sp_rmsnorm takes ONE row stride, so on the qkv layout the
    # per-head rows are only reachable as [T*H, D] after q and k are made contiguous - the copies are not timed
    qc = [split(b)[0].contiguous() for b in bufs]
    kc = [split(b)[1].contiguous() for b in bufs]
    qo, ko = torch.empty_like(qc[0]), torch.empty_like(kc[0])
    lib, st = _native.load(), torch.cuda.current_stream().cuda_stream

    def fused(i):
        q, k, v = split(bufs[i % nbuf])
        _native.qk_norm_rotary(pos, q, k, wq, wk, EPS, D, cache, True, value=v, k_buffer=kb, v_buffer=vb,
                               out_cache_loc=loc)

    def norm_q(i):
        lib.sp_rmsnorm(qo.data_ptr(), qc[i % nbuf].data_ptr(), wq.data_ptr(), T * HQ, D, D, D, EPS, _native.SP_BF16, st)

    def norm_k(i):
        lib.sp_rmsnorm(ko.data_ptr(), kc[i % nbuf].data_ptr(), wk.data_ptr(), T * HKV, D, D, D, EPS, _native.SP_BF16, st)

    def rotary(i):
        q, k, v = split(bufs[i % nbuf])
        _native.rotary_embedding(pos, q, k, D, cache, True, value=v, k_buffer=kb, v_buffer=vb, out_cache_loc=loc)

    # same bits first (on copies: both forms work in place)
    a = bufs[0].clone()
    q, k, v = split(a)
    _native.qk_norm_rotary(pos, q, k, wq, wk, EPS, D, cache, True, value=v, k_buffer=kb, v_buffer=vb, out_cache_loc=loc)
    kb_f, vb_f = kb.clone(), vb.clone()
    b = bufs[0].clone()
    q2, k2, v2 = split(b)
    q2.copy_(_native.rmsnorm(q2.reshape(-1, D), wq, EPS).view(T, -1))
    k2.copy_(_native.rmsnorm(k2.reshape(-1, D), wk, EPS).view(T, -1))
    _native.rotary_embedding(pos, q2, k2, D, cache, True, value=v2, k_buffer=kb, v_buffer=vb, out_cache_loc=loc)
    torch.cuda.synchronize()
    if not (torch.equal(a, b) and torch.equal(kb, kb_f) and torch.equal(vb, vb_f)):
        raise SystemExit(f"T={T}: the fused launch and the three-launch form differ")
    before = _native.QK_NORM_CALLS["fused"]
    for i in range(warmup):
        fused(i), norm_q(i), norm_k(i), rotary(i)
    torch.cuda.synchronize()
    res = {}
    for _round in range(3):                     # alternate the forms: three rounds each, the medians' median is kept
        for name, fn in (("fused", fused), ("norm_q", norm_q), ("norm_k", norm_k), ("rotary", rotary)):
            res.setdefault(name, []).append(median_us(fn, reps))
    if _native.QK_NORM_CALLS["fused"] - before != warmup + 3 * reps:
        raise SystemExit("the wrapper did not take the fused kernel")
    med = {k: statistics.median(m for m, _ in v) for k, v in res.items()}
    low = {k: min(m for _, m in v) for k, v in res.items()}
    eb = 2
    fused_bytes = eb * T * D * (2 * HQ + 2 * HKV + HKV + 2 * HKV)
    rotary_bytes = fused_bytes                  # the rotary launch alone moves the same rows
    three = med["norm_q"] + med["norm_k"] + med["rotary"]
    return (f"T={T:5d} bf16 Hq {HQ} Hkv {HKV} D {D}: fused {med['fused']:7.2f} us (min {low['fused']:.2f}, "
            f"{fused_bytes / med['fused'] / 1e6:.3f} TB/s)  three launches {three:7.2f} us = rmsnorm(q) "
            f"{med['norm_q']:.2f} + rmsnorm(k) {med['norm_k']:.2f} + rotary {med['rotary']:.2f} "
            f"({rotary_bytes / med['rotary'] / 1e6:.3f} TB/s)  fused/three {med['fused'] / three:.3f}  "
            f"[{'ok: no slower' if med['fused'] <= three else 'SLOWER'}]")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the result lines to this file")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_qk_norm.py needs the GPU: a CPU timing says nothing about these kernels")
    lines = [f"# tools/bench_qk_norm.py on {torch.cuda.get_device_name(0)}: medians of {args.reps} event-timed launches "
             f"x 3 alternating rounds, {args.warmup} warm-up launches per form"]
    for T, nbuf in ((256, 8), (8192, 6)):
        lines.append(bench(T, args.reps, args.warmup, nbuf))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
