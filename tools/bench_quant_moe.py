#!/usr/bin/env python3
"""The Llama-Quant-MoE feed-forward block on one MI355X, bf16: Llama-3-8B widths (hidden 4096, inter 14336), 8 experts
top-2, T in {1, 16, 64, 256} rows.

Per row count, in ONE process and on the same inputs, graph-replayed over 8 layer buffers (every layer its own base
MLP, router and experts: nothing is found in a cache), after a warm-up, as the median of 5 rounds with the spread
(max - min) / median:

  fused   base MLP + router projection + _native.qmoe_experts on the packed experts              [this block]
  dense   base MLP + router projection + _native.moe_experts on the experts unpacked to dense bf16 + an add
          [the formulation available before the packed kernels]
  packed-bytes rate: the packed bytes (codes + meta + scales, both projections) of the experts that own rows, over the
          fused block's time, as a fraction of 8 TB/s.  It is NOT the block's bandwidth: the base MLP's dense weights
          and the activations are left out.

  python tools/bench_quant_moe.py --out profiles/quant_moe.txt [--libs NAME ...] [--passes N]

Without --libs the product library is measured.  --libs names builds under scratchpad_amd/lib/ (SP_NATIVE_LIB), e.g.
the variants `python -m scratchpad_amd.build --qmoe-nw 2` makes; they are measured in turn, --passes times over, so
that builds alternate.  Every library is measured by a child process of its own under `timeout -k 10`; the first
child that fails ends the run (nothing more is started on the GPU).  The child's rows are JSON lines; --out appends
them verbatim behind a header."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HID, INTER, E, K, LAYERS = 4096, 14336, 8, 2, 8
ROWS = (1, 16, 64, 256)
ROUNDS, REPLAYS, WARMUP = 5, 10, 3
PEAK = 8e12


def child(seed: int) -> None:
    import torch
    sys.path.insert(0, ROOT)
    from scratchpad_amd import _native
    from scratchpad_amd.delta import unpack_delta
    dev, dt = "cuda", torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(seed)
    nib = torch.tensor([0x4, 0x8, 0xC, 0x9, 0xD, 0xE], device=dev, dtype=torch.int32)

    def packed(N, Kd):
        codes = torch.randint(0, 256, (E, N, Kd // 4), generator=g, device=dev, dtype=torch.int32).to(torch.uint8)
        lo = nib[torch.randint(0, 6, (E, N, Kd // 8), generator=g, device=dev)]
        hi = nib[torch.randint(0, 6, (E, N, Kd // 8), generator=g, device=dev)]
        scales = (0.002 + 0.004 * torch.rand((E, N), generator=g, device=dev)).to(dt)
        return codes, (lo | (hi << 4)).to(torch.uint8), scales

    def dense(p):
        return torch.stack([unpack_delta(p[0][e], p[1][e], p[2][e], dt) for e in range(E)])

    layers = []
    for _ in range(LAYERS):
        p13, p2 = packed(2 * INTER, HID), packed(HID, INTER)
        layers.append(dict(p13=p13, p2=p2, w13=dense(p13), w2=dense(p2),
                           b13=(torch.randn(2 * INTER, HID, generator=g, device=dev) * 0.02).to(dt),
                           b2=(torch.randn(HID, INTER, generator=g, device=dev) * 0.02).to(dt),
                           gate=torch.randn(E, HID, generator=g, device=dev).to(dt)))
    expert_bytes = sum(t[0].numel() * t.element_size() for p in (layers[0]["p13"], layers[0]["p2"]) for t in p)

    def base_mlp(x, L):          # llama.py's LlamaMLP.forward
        act = _native.linear_silu_mul(x, L["b13"])
        if act is None:
            act = _native.silu_and_mul(_native.linear(x, L["b13"]))
        return _native.linear(act, L["b2"])

    def fused(x, L):
        return _native.qmoe_experts(x, _native.linear(x, L["gate"]), L["p13"], L["p2"], K, _native.QMOE_ORDER_RANK,
                                    base_mlp(x, L))

    def dense_form(x, L):
        return _native.moe_experts(x, _native.linear(x, L["gate"]), L["w13"], L["w2"], K) + base_mlp(x, L)

    def measure(fn, x):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for L in layers:
                fn(x, L)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = [fn(x, L) for L in layers]
        for _ in range(WARMUP):
            graph.replay()
        torch.cuda.synchronize()
        rounds = []
        for _ in range(ROUNDS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(REPLAYS):
                graph.replay()
            b.record()
            torch.cuda.synchronize()
            rounds.append(a.elapsed_time(b) * 1e3 / (REPLAYS * LAYERS))          # microseconds per block
        return statistics.median(rounds), (max(rounds) - min(rounds)) / statistics.median(rounds), outs

    for T in ROWS:
        x = torch.randn(T, HID, generator=g, device=dev).to(dt)
        owning = []
        for L in layers:
            _, _, off, _ = _native.moe_route(_native.linear(x, L["gate"]), K)
            owning.append(int(((off[1:] - off[:-1]) > 0).sum()))
        tf, sf, of = measure(fused, x)
        td, sd, od = measure(dense_form, x)
        finite = all(bool(torch.isfinite(o.float()).all()) for o in of + od)
        own = sum(owning) / LAYERS
        print(json.dumps({"lib": os.environ.get("SP_NATIVE_LIB") or "libscratchpad_hip.so",
                          "weight_tiles": _native.qmoe_weight_tiles(), "rows": T, "fused_us": round(tf, 2),
                          "fused_spread": round(sf, 4), "dense_us": round(td, 2), "dense_spread": round(sd, 4),
                          "fused_over_dense": round(tf / td, 4), "experts_owning_rows": own,
                          "packed_bytes_rate_of_8TBps": round(own * expert_bytes / (tf * 1e-6) / PEAK, 4),
                          "finite": finite}), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--libs", nargs="*", default=[""])
    ap.add_argument("--passes", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        child(a.seed)
        return 0
    lines = [f"# tools/bench_quant_moe.py: hidden {HID}, inter {INTER}, {E} experts top-{K}, bf16, {LAYERS} layer "
             f"buffers, graph replay, median of {ROUNDS} rounds x {REPLAYS} replays, microseconds per block; spread = "
             "(max - min) / median of the rounds"]
    status = 0
    for _ in range(a.passes):
        for lib in a.libs:
            env = dict(os.environ)
            env.pop("SP_NATIVE_LIB", None)
            if lib:
                env["SP_NATIVE_LIB"] = lib
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "--seed",
                   str(a.seed)]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True)
            rows = [l for l in r.stdout.splitlines() if l.startswith("{")]
            lines += rows
            print("\n".join(rows), flush=True)
            if r.returncode != 0:
                lines.append(f"# child for {lib or 'the product library'} ended with status {r.returncode}; the run "
                             "stops here")
                print(r.stderr[-2000:], file=sys.stderr)
                status = r.returncode
                break
        if status:
            break
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
