#!/usr/bin/env python3
"""sp_lora_shrink + sp_lora_expand at the four Llama-3-8B projections (qkv 4096 -> 4096 + 2 x 1024, o 4096 -> 4096,
gate_up 4096 -> 2 x 14336, down 14336 -> 4096), r 16, bf16, at 1, 16 and 256 rows with 1, 4 and 8 adapters in the
batch (rows grouped by adapter, as the scheduler delivers them), against the reference-style formulation: for each
adapter of the batch  y[rows] += (x[rows] @ A[id]) @ B[id]  in torch (topping_layer.py's non-ldmm branches), with the
row lists precomputed so that both forms can be captured.

Method (profiles/README.md): both forms are captured into a HIP graph that runs the operation once per LAYER buffer
(32 different A / B buffers, cycled as _native._time_mm cycles weights, so no launch finds its adapter in a cache the
previous one filled), replayed after a warm-up replay, timed with device events; the figure is the median of the
rounds, in microseconds per projection.  Results are compared before anything is timed.

``--e2e``: the decode step of Llama-3-8B (random weights) at 256 rows under graph replay, with a manager serving 8
adapters on all four projections against the same step without a manager: added milliseconds per step.

The driver runs every step in a child process of its own, each under its own time limit, and stops at the first
non-zero status.

Usage: python tools/bench_lora.py [--out FILE] [--e2e]"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HIDDEN, INTER, QN, KVN, R, LAYERS, SLOTS = 4096, 14336, 4096, 1024, 16, 32, 8
BATCHES, ADAPTERS = (1, 16, 256), (1, 4, 8)
# name: (K, [(tmp offset in units of r, slices, n)]) - the expands of one shrink
PROJ = {"qkv_proj": (HIDDEN, [(0, 1, QN), (1, 2, KVN)]), "o_proj": (QN, [(0, 1, HIDDEN)]),
        "gate_up_proj": (HIDDEN, [(0, 2, INTER)]), "down_proj": (INTER, [(0, 1, HIDDEN)])}
STEP_TIMEOUT_S = 240


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
    dt = torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(bs)
    lines = []
    for name, (K, expands) in PROJ.items():
        S_all = sum(s for _, s, _ in expands)
        N = sum(s * n for _, s, n in expands)
        A = [(torch.randn(SLOTS, K, S_all * R, generator=g, device="cuda") * 0.05).to(dt) for _ in range(LAYERS)]
        B = [[(torch.randn(SLOTS, R, s * n, generator=g, device="cuda") * 0.05).to(dt) for _, s, n in expands]
             for _ in range(LAYERS)]
        x = torch.randn(bs, K, generator=g, device="cuda").to(dt)
        y0 = torch.randn(bs, N, generator=g, device="cuda").to(dt)
        for na in ADAPTERS:
            if na > bs:
                continue
            ids = [(i * na) // bs for i in range(bs)]           # grouped by adapter
            idx = torch.tensor(ids, dtype=torch.int32, device="cuda")
            rows = [torch.tensor([i for i in range(bs) if ids[i] == a], device="cuda") for a in range(na)]
            tmp = torch.zeros(bs, S_all * R, dtype=torch.float32, device="cuda")
            y_k, y_t = y0.clone(), y0.clone()

            def ours(layer):
                _native.lora_shrink(x, A[layer], idx, 2.0, out=tmp)
                col = 0
                for (off, s, n), b in zip(expands, B[layer]):
                    _native.lora_expand(y_k[:, col:col + s * n], tmp[:, off * R:], b, idx, s)
                    col += s * n

            def masked_torch(layer):
                for a in range(na):
                    xa = x if na == 1 else x[rows[a]]
                    t = (xa @ A[layer][a]) * 2.0
                    parts = []
                    for (off, s, n), b in zip(expands, B[layer]):
                        for k in range(s):
                            parts.append(t[:, (off + k) * R:(off + k + 1) * R] @ b[a][:, k * n:(k + 1) * n])
                    d = torch.cat(parts, 1) if len(parts) > 1 else parts[0]
                    if na == 1:
                        y_t.add_(d)
                    else:
                        y_t.index_add_(0, rows[a], d)

            ours(0), masked_torch(0)
            torch.cuda.synchronize()
            dev = float((y_k.float() - y_t.float()).abs().max() / y_t.float().abs().max())
            if dev > 2.0 ** -6:
                raise SystemExit(f"{name} bs {bs} adapters {na}: the two forms differ by {dev:.2e} of the scale")
            t_k, t_t = graph_us(ours), graph_us(masked_torch)
            lines.append(f"{name:13s} bs {bs:3d} adapters {na}: kernels {t_k:8.2f} us  masked torch {t_t:8.2f} us  "
                         f"kernels/torch {t_k / t_t:.3f}  [{'ok: no slower' if t_k <= t_t else 'SLOWER'}]")
            print(lines[-1], flush=True)
        del A, B
    return lines


def step_e2e():
    import torch
    from scratchpad_amd.model_runner import ModelConfig, ModelRunner, ServerArgs
    from scratchpad_amd.toppings import LoRAAdapter, ToppingConfig
    bs, cfg = 256, ModelConfig.llama3_8b()
    D = cfg.head_dim
    dims = {"q_proj": (HIDDEN, cfg.num_attention_heads * D), "k_proj": (HIDDEN, cfg.num_key_value_heads * D),
            "v_proj": (HIDDEN, cfg.num_key_value_heads * D), "o_proj": (cfg.num_attention_heads * D, HIDDEN),
            "gate_proj": (HIDDEN, INTER), "up_proj": (HIDDEN, INTER), "down_proj": (INTER, HIDDEN)}
    sd = {}
    for layer in range(cfg.num_hidden_layers):
        for t, (din, dout) in dims.items():
            block = "self_attn" if t in ("q_proj", "k_proj", "v_proj", "o_proj") else "mlp"
            base = f"base_model.model.model.layers.{layer}.{block}.{t}"
            sd[base + ".lora_A.weight"] = torch.randn(R, din) * 0.02
            sd[base + ".lora_B.weight"] = torch.randn(dout, R) * 0.02
    res = {}
    for what in ("without a manager", "with 8 adapters"):
        ads = None
        if what != "without a manager":
            conf = lambda u: ToppingConfig("lora", u, {"r": R, "lora_alpha": 2 * R, "target_modules": list(dims)})
            ads = [LoRAAdapter(f"ad{i}", conf(f"ad{i}"), cfg).initialize_weights(sd) for i in range(SLOTS)]
        args = ServerArgs(max_total_tokens=bs * 64, max_running_requests=bs, cuda_graph_bs=[bs],
                          max_toppings_per_batch=SLOTS if ads else None)
        mr = ModelRunner(cfg, args, toppings=ads)
        mr.init_cuda_graphs()
        if ads:
            tm = mr.topping_manager
            for i in range(SLOTS):
                tm.load_topping(f"ad{i}", i)
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
            f"with 8 adapters on all four projections {b:.3f} ms: +{b - a:.3f} ms per step")
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
            raise SystemExit("bench_lora.py needs the GPU: a CPU timing says nothing about these kernels")
        lines = step_e2e() if args.step == "e2e" else step_kernels(int(args.step.split(":")[1]))
        if args.out:
            with open(args.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return 0
    steps = [f"kernels:{bs}" for bs in BATCHES] + (["e2e"] if args.e2e else [])
    if args.out:
        with open(args.out, "a") as f:
            f.write("# tools/bench_lora.py: us per projection (shrink + expands), graph-replayed over 32 layer buffers, "
                    "median of 5 rounds\n")
    for step in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step] + (["--out", args.out] if args.out else [])
        try:
            rc = subprocess.run(cmd, timeout=STEP_TIMEOUT_S * (3 if step == "e2e" else 1)).returncode
        except subprocess.TimeoutExpired:
            print(f"step {step}: time limit reached; stopping", flush=True)
            return 124
        if rc != 0:
            print(f"step {step}: exit status {rc}; stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
