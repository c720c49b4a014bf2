#!/usr/bin/env python3
"""sp_delta_mm at the four Llama-3-8B projections (qkv 4096 -> 6144, o 4096 -> 4096, gate_up 4096 -> 28672, down
14336 -> 4096), bf16, at 1, 16 and 256 rows with 1, 4 and 8 adapters in the batch, against the reference-style
formulation on the SAME deltas unpacked to dense bf16: for each adapter of the batch  y[rows] += x[rows] @ D[id]^T  in
torch (topping_layer.py's non-ldmm branches), with the row lists precomputed so that both forms can be captured.  The
slots hold random valid packed bytes (every code, every position pair), generated on the device.

Method (profiles/README.md): both forms are captured into a HIP graph that runs the operation once per LAYER buffer
(8 different packed / dense buffers, cycled, so no launch finds its delta in a cache the previous one filled),
replayed after a warm-up replay, timed with device events; the figure is the median of the rounds, in microseconds
per projection.  The grouping (sp_delta_group, once per forward, not per projection) is done before the capture.
Results are compared before anything is timed.  Next to the time: the packed bytes the kernel has to read (the slots
that own rows: codes + meta + scales) divided by the time, as a share of 8 TB/s.

``--e2e``: the decode step of Llama-3-8B (random weights) at 256 rows under graph replay, with a manager serving 8
delta adapters on all four projections (slots filled on the device) against the same step without a manager: added
milliseconds per step.

The driver runs every step in a child process of its own, each under its own time limit, and stops at the first
non-zero status.

Usage: python tools/bench_delta.py [--out FILE] [--e2e]"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HIDDEN, INTER, QN, KVN, LAYERS, SLOTS = 4096, 14336, 4096, 1024, 8, 8
BATCHES, ADAPTERS = (1, 16, 256), (1, 4, 8)
PROJ = {"qkv_proj": (QN + 2 * KVN, HIDDEN), "o_proj": (HIDDEN, QN), "gate_up_proj": (2 * INTER, HIDDEN),
        "down_proj": (HIDDEN, INTER)}                      # name: (N, K)
HBM_BYTES_PER_S = 8e12
STEP_TIMEOUT_S = 300
VALID_NIBBLES = (4, 8, 12, 9, 13, 14)                      # p0 | p1 << 2 for p0 < p1


def random_packed(shape_prefix, N, K, dtype, g):
    """random valid packed bytes on the device: codes [.., N, K/4], meta [.., N, K/8], scales [.., N]"""
    import torch
    codes = torch.randint(0, 256, shape_prefix + (N, K // 4), generator=g, device="cuda", dtype=torch.uint8)
    lut = torch.tensor(VALID_NIBBLES, device="cuda", dtype=torch.uint8)
    pick = lambda: lut[torch.randint(0, 6, shape_prefix + (N, K // 8), generator=g, device="cuda")]
    meta = pick() | (pick() << 4)
    scales = (torch.rand(shape_prefix + (N,), generator=g, device="cuda") * 0.004 + 0.001).to(dtype)
    return codes, meta, scales


def graph_us(run_layer, rounds=5):
    import torch
    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        for layer in range(LAYERS):
            run_layer(layer)
        st.synchronize()
        with torch.cuda.graph(g, stream=st, capture_error_mode="thread_local"):
            for layer in range(LAYERS):
                run_layer(layer)
    torch.cuda.synchronize()
    g.replay()
    times = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(3):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / (3 * LAYERS) * 1e3)
    return statistics.median(times)


def step_kernels(bs):
    import torch
    from scratchpad_amd import _native
    from scratchpad_amd.delta import unpack_delta
    dt = torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(bs)
    lines = []
    for name, (N, K) in PROJ.items():
        packed = [random_packed((SLOTS,), N, K, dt, g) for _ in range(LAYERS)]
        dense = [torch.stack([unpack_delta(c[s], m[s], sc[s], dt) for s in range(SLOTS)]) for c, m, sc in packed]
        x = torch.randn(bs, K, generator=g, device="cuda").to(dt)
        y0 = torch.randn(bs, N, generator=g, device="cuda").to(dt)
        for na in ADAPTERS:
            if na > bs:
                continue
            ids = [(i * na) // bs for i in range(bs)]           # grouped by adapter
            idx = torch.tensor(ids, dtype=torch.int32, device="cuda")
            rows = [torch.tensor([i for i in range(bs) if ids[i] == a], device="cuda") for a in range(na)]
            offs = torch.zeros(SLOTS + 1, dtype=torch.int32, device="cuda")
            srt = torch.zeros(bs, dtype=torch.int32, device="cuda")
            _native.delta_group(idx, bs, SLOTS, offs, srt)
            y_k, y_t = y0.clone(), y0.clone()

            def ours(layer):
                c, m, sc = packed[layer]
                _native.delta_mm(y_k, x, c, m, sc, offs, srt)

            def masked_torch(layer):
                for a in range(na):
                    if na == 1:
                        y_t.addmm_(x, dense[layer][a].t())
                    else:
                        y_t.index_add_(0, rows[a], x[rows[a]] @ dense[layer][a].t())

            ours(0), masked_torch(0)
            torch.cuda.synchronize()
            dev = float((y_k.float() - y_t.float()).abs().max() / y_t.float().abs().max())
            if dev > 2.0 ** -6:
                raise SystemExit(f"{name} bs {bs} adapters {na}: the two forms differ by {dev:.2e} of the scale")
            t_k, t_t = graph_us(ours), graph_us(masked_torch)
            read = na * (N * K * 3 // 8 + 2 * N)
            share = read / (t_k * 1e-6) / HBM_BYTES_PER_S
            lines.append(f"{name:13s} bs {bs:3d} adapters {na}: kernel {t_k:8.2f} us  masked torch on dense bf16 "
                         f"{t_t:8.2f} us  kernel/torch {t_k / t_t:.3f}  [{'ok: no slower' if t_k <= t_t else 'SLOWER'}]"
                         f"  packed {read / 1e6:7.1f} MB at {100 * share:5.1f}% of 8 TB/s")
            print(lines[-1], flush=True)
        del packed, dense
        torch.cuda.empty_cache()
    return lines


def step_e2e():
    import torch
    from scratchpad_amd.model_runner import ModelConfig, ModelRunner, ServerArgs
    from scratchpad_amd.toppings import DeltaAdapter, ToppingConfig
    bs, cfg = 256, ModelConfig.llama3_8b()
    res = {}
    for what in ("without a manager", "with 8 adapters"):
        ads = None
        if what != "without a manager":
            # the adapters only name the modules they serve: the slots are filled on the device below (8 x 2.6 GB of
            # packed host tensors, staged and pinned, would measure the host)
            ads = [DeltaAdapter(f"ad{i}", ToppingConfig("delta", f"ad{i}"), cfg) for i in range(SLOTS)]
            for a in ads:
                a.target_modules = set(PROJ)
        args = ServerArgs(max_total_tokens=bs * 64, max_running_requests=bs, cuda_graph_bs=[bs],
                          max_toppings_per_batch=SLOTS if ads else None)
        mr = ModelRunner(cfg, args, toppings=ads)
        mr.init_cuda_graphs()
        if ads:
            tm, pool = mr.topping_manager, mr.topping_manager.topping_memory_pool
            g = torch.Generator(device="cuda").manual_seed(1)
            for module, (N, K) in PROJ.items():
                for layer in range(cfg.num_hidden_layers):
                    c, m, sc = random_packed((SLOTS,), N, K, mr.dtype, g)
                    pool.qweight_all[module][layer].copy_(c)
                    pool.meta_all[module][layer].copy_(m)
                    pool.scales_all[module][layer].copy_(sc)
            tm.weight_indices[:bs].copy_(torch.tensor([(i * SLOTS) // bs for i in range(bs)], dtype=torch.int32))
        graph = mr.graph_runner.graphs[bs]
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize()
        times = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                graph.replay()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / 10)
        res[what] = statistics.median(times)
        del mr, graph
        torch.cuda.empty_cache()
    a, b = res["without a manager"], res["with 8 adapters"]
    line = (f"Llama-3-8B decode step, bs {bs}, graph replay (captured sequence lengths): without a manager {a:.3f} ms, "
            f"with 8 delta adapters on all four projections {b:.3f} ms: +{b - a:.3f} ms per step")
    print(line, flush=True)
    return [line]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the result lines to this file")
    ap.add_argument("--e2e", action="store_true", help="also time the whole Llama-3-8B decode step")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)      # child: "kernels:<bs>" or "e2e"
    args = ap.parse_args()
    if args.step is not None:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_delta.py needs the GPU: a CPU timing says nothing about these kernels")
        lines = step_e2e() if args.step == "e2e" else step_kernels(int(args.step.split(":")[1]))
        if args.out:
            with open(args.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return 0
    steps = [f"kernels:{bs}" for bs in BATCHES] + (["e2e"] if args.e2e else [])
    if args.out:
        with open(args.out, "a") as f:
            f.write("# tools/bench_delta.py: us per projection (one sp_delta_mm), graph-replayed over 8 layer buffers, "
                    "median of 5 rounds\n")
    for step in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step] + (["--out", args.out] if args.out else [])
        try:
            rc = subprocess.run(cmd, timeout=STEP_TIMEOUT_S * (2 if step == "e2e" else 1)).returncode
        except subprocess.TimeoutExpired:
            print(f"step {step}: time limit reached; stopping", flush=True)
            return 124
        if rc != 0:
            print(f"step {step}: exit status {rc}; stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
