"""Tensor-parallel forward on the GPU kernels: world_size 2 and 4 ranks share cuda:0 and talk
over gloo (the box has one GPU; RCCL refuses two ranks on one device), each rank holding its
shard of the heads, of the KV pool and of the linears exactly as on a TP node
(linear.py:696-760, 1033-1155; model_runner.py:420-429).  Every rank's gathered logits must equal
the unsharded oracle's for a ragged prefill and a decode step.

Every multi-rank test also has ONE-DEVICE-PER-RANK parametrisations at world 2, 4 and 8 (RCCL over xGMI, the direct
all-reduce across devices, collectives captured in HIP graphs, config 4's real head counts at TP = 8).  They are
skipped where the box has fewer GPUs than ranks - every box of this pool so far - and run as they are on a TP node
(distributed/parallel_state.py:256-353, device_communicators/pynccl.py:108-130)."""
import os
import socket
import traceback

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _needs(n):
    return pytest.mark.skipif(torch.cuda.device_count() < n, reason=f"needs >= {n} GPUs (one device per rank)")


# (world, one device per rank): ranks sharing cuda:0 exercise the protocol through IPC within one device; the
# per-device cases are the real transport (peer mappings over xGMI) and are skipped on a one-GPU box
PLACEMENTS = [pytest.param(2, False, id="2-ranks-on-one-gpu"), pytest.param(4, False, id="4-ranks-on-one-gpu"),
              pytest.param(2, True, marks=_needs(2), id="2-gpus"), pytest.param(4, True, marks=_needs(4), id="4-gpus"),
              pytest.param(8, True, marks=_needs(8), id="8-gpus")]


def _run_ranks(target, world, extra, timeout=300):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port, q) + tuple(extra)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=timeout) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    for rank, err in results:
        assert err is None, f"rank {rank}:\n{err}"


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _family_case(family, case):
    """(shape, full weights, ModelConfig, the unsharded oracle's forward) of a tiny fixture"""
    from scratchpad_amd.model_runner import ModelConfig
    if family != "llama":
        from tests import apertus_oracle, qwen3_oracle
        oracle = {"qwen3": qwen3_oracle, "apertus": apertus_oracle}[family]
        g, pfx, shape, w = oracle.load_case(case)
        return shape, w, oracle.model_config(shape), oracle.forward
    from oracle import llama as ollama
    from tests import smoke_impl
    g, pfx, shape, w = smoke_impl.load_case(case)
    scaling = None
    if shape.rope_scaling is not None:
        f = shape.rope_scaling
        scaling = {"rope_type": "llama3", "factor": f[0], "low_freq_factor": f[1], "high_freq_factor": f[2],
                   "original_max_position_embeddings": int(f[3])}
    cfg = ModelConfig(shape.hidden, shape.inter, shape.layers, shape.Hq, shape.Hkv, shape.vocab, context_len=60,
                      rms_norm_eps=shape.rms_eps, rope_theta=shape.rope_theta, rope_scaling=scaling,
                      max_position_embeddings=shape.max_pos, tie_word_embeddings=shape.tie)
    return shape, w, cfg, ollama.forward


def _rank_main(rank, world, port, case, q, custom_ar=False, family="llama"):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        os.environ["SP_CUSTOM_ALLREDUCE"] = "1" if custom_ar else "0"
        os.environ["SP_CUSTOM_ALLREDUCE_FUSE_NORM"] = "1" if custom_ar else "0"     # (a second opt-in)
        from oracle import llama as ollama, ops
        from scratchpad_amd import distributed as d
        from scratchpad_amd.forward_info import ForwardMode, ModelWorkerBatch
        from scratchpad_amd.model_runner import ModelRunner, ServerArgs, TpModelWorker
        d.init_distributed_environment(world, rank, f"tcp://127.0.0.1:{port}", 0, backend="gloo")
        d.initialize_model_parallel(world, backend="gloo", local_rank=0)
        shape, w, cfg, oracle_forward = _family_case(family, case)
        mr = ModelRunner(cfg, ServerArgs(max_total_tokens=96, max_running_requests=3, disable_cuda_graph=True),
                         tp_rank=rank, tp_size=world, dtype=torch.float32, gpu_id=0, init_weights=False)
        assert mr.token_to_kv_pool.head_num == max(1, shape.Hkv // world), "each rank pools only its KV heads"
        assert (d.get_tp_group().ca_comm is not None) == custom_ar
        mr.model.load_full_state_dict({k: v.to(mr.device) for k, v in w.items()})
        worker = TpModelWorker(mr)
        dev = mr.device
        gen = torch.Generator().manual_seed(5)
        lens = [7, 4]
        ids = torch.randint(0, shape.vocab, (sum(lens),), generator=gen)
        loc = torch.arange(1, 1 + sum(lens))
        table = mr.req_to_token_pool.req_to_token
        table[0, :7] = loc[:7].to(torch.int32).to(dev)
        table[1, :4] = loc[7:].to(torch.int32).to(dev)
        req = torch.tensor([0, 1])
        batch = ModelWorkerBatch(bid=1, forward_mode=ForwardMode.EXTEND, input_ids=ids.to(dev),
                                 req_pool_indices=req.to(dev), seq_lens=torch.tensor(lens).to(dev),
                                 out_cache_loc=loc.to(dev), seq_lens_sum=sum(lens), extend_num_tokens=sum(lens),
                                 extend_seq_lens=lens, extend_prefix_lens=[0, 0])
        out, nxt = worker.forward_batch_generation(batch)
        okv = ollama.OracleKV(shape, 96, 4, 64)
        okv.req_to_token.copy_(table.cpu())
        ext = torch.tensor(lens, dtype=torch.int32)
        pos, start = ops.compute_position(torch.zeros(2, dtype=torch.int32), ext)
        ref = oracle_forward(shape, w, okv, mode="extend", input_ids=ids, positions=pos, req_pool_indices=req,
                             seq_lens=torch.tensor(lens), out_cache_loc=loc, extend_seq_lens=ext, extend_start_loc=start)
        rel = lambda a, b: float((a.float().cpu() - b).abs().max() / b.abs().max())
        with pytest.raises(RuntimeError, match="gather_full_logits"):
            out.next_token_logits          # a collective never hides behind an attribute read under TP
        out.gather_full_logits()           # explicit, on every rank
        assert out.next_token_logits.shape == ref.shape
        assert rel(out.next_token_logits, ref) <= 1e-4, ("prefill", rank, rel(out.next_token_logits, ref))
        assert torch.equal(nxt.cpu(), ref.argmax(-1))
        # vocab-parallel greedy (one (value, index) pair per row exchanged) == argmax of the gathered logits
        from scratchpad_amd import _native
        assert out.shard_logits.shape[1] * world >= shape.vocab and out.shard_logits.shape[0] == 2
        assert torch.equal(out.greedy_token_ids(), _native.argmax(out.next_token_logits))
        # decode step
        loc2 = torch.tensor([20, 21])
        table[0, 7] = 20
        table[1, 4] = 21
        seq2 = torch.tensor([8, 5])
        batch = ModelWorkerBatch(bid=2, forward_mode=ForwardMode.DECODE, input_ids=nxt, req_pool_indices=req.to(dev),
                                 seq_lens=seq2.to(dev), out_cache_loc=loc2.to(dev), seq_lens_sum=13)
        out2, _ = worker.forward_batch_generation(batch)
        out2.gather_full_logits()
        okv.req_to_token.copy_(table.cpu())
        ref2 = oracle_forward(shape, w, okv, mode="decode", input_ids=nxt.cpu(), positions=ops.clamp_position(seq2),
                              req_pool_indices=req, seq_lens=seq2, out_cache_loc=loc2)
        assert rel(out2.next_token_logits, ref2) <= 1e-4, ("decode", rank, rel(out2.next_token_logits, ref2))
        torch.distributed.barrier()
        q.put((rank, None))
    except Exception:
        q.put((rank, traceback.format_exc()))


@pytest.mark.parametrize("world,case,custom_ar", [(2, "a", False), (2, "b", False), (4, "a", False), (2, "b", True),
                                                  (4, "a", True)],
                         ids=["tp2-kv-replicated", "tp2-kv-sharded", "tp4-kv-replicated", "tp2-direct-all-reduce",
                              "tp4-direct-all-reduce-fused-norm"])
def test_sharded_forward_matches_unsharded_oracle(world, case, custom_ar):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, world, port, case, q, custom_ar)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    for rank, err in results:
        assert err is None, f"rank {rank}:\n{err}"


def _family_main(rank, world, port, q, case, family):
    _rank_main(rank, world, port, case, q, family=family)


@pytest.mark.parametrize("family", ["qwen3", "apertus"])
def test_qwen3_and_apertus_run_the_shared_deferred_all_reduce_protocol(family):
    """Fixture "a" of each (Hq 4 / Hkv 2, the KV heads sharded at world 2; Qwen3 D 128, Apertus inter 96), fp32, the
    ragged prefill [7, 4] plus one decode step against the unsharded oracle, at the bound of the fp32 Llama cases
    above.  Their layers inherit LlamaDecoderLayer.forward: two layers, so the second enters with partial sums and
    pays the previous down_proj's all-reduce in its first norm; two requests make the batch ragged."""
    _run_ranks(_family_main, 2, ("a", family), timeout=300)


def _ar_main(rank, world, port, q, per_device=False):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        from scratchpad_amd import distributed as d
        from scratchpad_amd.custom_all_reduce import CustomAllReduce
        dev = rank if per_device else 0
        torch.cuda.set_device(dev)
        d.init_distributed_environment(world, rank, f"tcp://127.0.0.1:{port}", dev, backend="gloo")
        d.initialize_model_parallel(world, backend="gloo", local_rank=dev)
        tp = d.get_tp_group()
        ca = CustomAllReduce(tp, max_bytes=4 << 20)
        tp.ca_comm = ca
        gen = torch.Generator().manual_seed(100)        # the same stream on every rank: rank r's input is slice r
        for dtype, shape in ((torch.bfloat16, (128, 8192)), (torch.float16, (3, 4096)), (torch.float32, (7, 1024)),
                             (torch.bfloat16, (1, 8)), (torch.bfloat16, (256, 4096))):
            for rep in range(3):
                allx = torch.randn(world, *shape, generator=gen).to(dtype)
                x = allx[rank].cuda()
                want = allx.float().sum(0)
                assert ca.should_custom_ar(x)
                y = d.tensor_model_parallel_all_reduce(x)       # goes through ca_comm
                torch.cuda.synchronize()
                eps = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 1e-6}[dtype]
                err = (y.float().cpu() - want).abs()
                assert bool((err <= eps * want.abs() + 1e-5).all()), (rank, dtype, shape, float(err.max()))
                gathered = [None] * world
                torch.distributed.all_gather_object(gathered, y.cpu(), group=tp.cpu_group)
                assert all(torch.equal(gathered[0], t) for t in gathered), "every rank holds the same bits"
        big = torch.zeros(4 << 20, dtype=torch.float32, device="cuda")      # 16 MiB > max_bytes -> library path
        assert not ca.should_custom_ar(big) and ca.custom_all_reduce(big) is None
        # the launch carries no per-call argument (epoch counters are device state), so it can be captured
        # into a HIP graph and replayed: every replay must still meet its peers at the right epoch
        xs = torch.zeros(128, 8192, dtype=torch.bfloat16, device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            d.tensor_model_parallel_all_reduce(xs)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with ca.capture(), torch.cuda.graph(graph):
            ys = d.tensor_model_parallel_all_reduce(xs)
            ys2 = d.tensor_model_parallel_all_reduce(ys)            # two dependent calls in one graph
        for rep in range(4):
            allx = torch.randn(world, 128, 8192, generator=gen).to(torch.bfloat16)
            xs.copy_(allx[rank])
            graph.replay()
            torch.cuda.synchronize()
            want = allx.float().sum(0)
            err = (ys.float().cpu() - want).abs()
            assert bool((err <= 2.0 ** -8 * want.abs() + 1e-5).all()), ("graph replay", rank, rep, float(err.max()))
            assert torch.equal(ys2.float().cpu(), (ys.float().cpu() * world).to(torch.bfloat16).float())
            y_eager = d.tensor_model_parallel_all_reduce(xs)        # eager calls interleave with replays
            torch.cuda.synchronize()
            assert torch.equal(y_eager, ys)
        ca.check()                                                  # no barrier timed out
        assert not ca.failed and ca.calls > 0
        torch.distributed.barrier()
        ca.close()
        q.put((rank, None))
    except Exception:
        q.put((rank, traceback.format_exc()))


@pytest.mark.parametrize("world,per_device", PLACEMENTS)
def test_direct_all_reduce_through_ipc_regions(world, per_device):
    """csrc/allreduce.hip in the ca_comm seam: one-shot (small) and two-shot (large) sums, eager and replayed from a
    HIP graph.  Ranks that share this GPU map each other's regions through IPC within one device - NOT a test of
    xGMI transport; the one-device-per-rank cases are (system-scope flags and data across peer mappings)."""
    _run_ranks(_ar_main, world, (per_device,), timeout=240)


def _fused_main(rank, world, port, q, per_device=False):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        os.environ["SP_CUSTOM_ALLREDUCE_FUSE_NORM"] = "1"
        from scratchpad_amd import _native, distributed as d
        from scratchpad_amd.custom_all_reduce import CustomAllReduce
        dev = rank if per_device else 0
        torch.cuda.set_device(dev)
        d.init_distributed_environment(world, rank, f"tcp://127.0.0.1:{port}", dev, backend="gloo")
        d.initialize_model_parallel(world, backend="gloo", local_rank=dev)
        tp = d.get_tp_group()
        ca = CustomAllReduce(tp, max_bytes=4 << 20)
        tp.ca_comm = ca
        gen = torch.Generator().manual_seed(200)        # the same stream on every rank: rank r's input is slice r
        eps = 1e-5
        # (dtype, T, hidden): two-shot at 70B's [128, 8192], one-shot below 256 KiB, fewer rows than ranks, rows
        # that do not divide by the world size, fp16 / fp32, Llama-3-8B's width
        cases = ((torch.bfloat16, 128, 8192), (torch.bfloat16, 8, 8192), (torch.bfloat16, 1, 8192),
                 (torch.bfloat16, 3, 4096), (torch.bfloat16, 130, 8192), (torch.float16, 40, 4096),
                 (torch.float32, 7, 1024), (torch.float32, 70, 2048), (torch.bfloat16, 256, 4096))
        for dtype, T, H in cases:
            for rep in range(2):
                allx = (torch.randn(world, T, H, generator=gen) * 2.0).to(dtype)
                res0 = (torch.randn(T, H, generator=gen) * 3.0).to(dtype).cuda()     # replicated, like the residual stream
                w = (1.0 + 0.25 * torch.randn(H, generator=gen)).to(dtype).cuda()
                # the two-step form: all-reduce (direct kernel), then the fused-add RMSNorm kernel
                y = ca.custom_all_reduce(allx[rank].cuda())
                res_ref = res0.clone()
                _native.fused_add_rmsnorm(y, res_ref, w, eps)
                # the one-kernel form, in place on the partial sums and the residual
                x = allx[rank].cuda()
                res = res0.clone()
                assert tp.fused_all_reduce_add_rmsnorm(x, res, w, eps) is True
                torch.cuda.synchronize()
                assert torch.equal(res, res_ref), ("residual", rank, dtype, T, H, rep)
                assert torch.equal(x, y), ("normed", rank, dtype, T, H, rep,
                                           float((x.float() - y.float()).abs().max()))
                # and against plain torch on the host: sum in fp32, one rounding, add, norm
                s = allx.float().sum(0).to(dtype).float() + res0.float().cpu()
                want = (s * torch.rsqrt(s.pow(2).mean(-1, keepdim=True) + eps)).to(dtype).float() * w.float().cpu()
                tol = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10, torch.float32: 1e-5}[dtype]
                err = (x.float().cpu() - want).abs()
                assert bool((err <= tol * want.abs() + tol).all()), (rank, dtype, T, H, float(err.max()))
        # shapes the fused kernel does not take are refused on every rank alike, nothing touched
        odd = torch.zeros(4, 8200, dtype=torch.bfloat16, device="cuda")
        assert tp.fused_all_reduce_add_rmsnorm(odd, odd.clone(), torch.ones(8200, dtype=torch.bfloat16, device="cuda"), eps) is False
        # captured into a HIP graph next to a plain all-reduce, replayed with fresh inputs, eager calls in between
        T, H = 128, 8192
        xs = torch.zeros(T, H, dtype=torch.bfloat16, device="cuda")
        rs = torch.zeros(T, H, dtype=torch.bfloat16, device="cuda")
        w = (1.0 + 0.25 * torch.randn(H, generator=gen)).to(torch.bfloat16).cuda()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            tp.fused_all_reduce_add_rmsnorm(xs, rs, w, eps)
            d.tensor_model_parallel_all_reduce(xs)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with ca.capture(), torch.cuda.graph(graph):
            tp.fused_all_reduce_add_rmsnorm(xs, rs, w, eps)
            again = d.tensor_model_parallel_all_reduce(xs)          # a dependent plain all-reduce in the same graph
        for rep in range(3):
            allx = torch.randn(world, T, H, generator=gen).to(torch.bfloat16)
            res0 = torch.randn(T, H, generator=gen).to(torch.bfloat16).cuda()
            y = ca.custom_all_reduce(allx[rank].cuda())
            res_ref = res0.clone()
            _native.fused_add_rmsnorm(y, res_ref, w, eps)
            xs.copy_(allx[rank])
            rs.copy_(res0)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(rs, res_ref) and torch.equal(xs, y), ("graph replay", rank, rep)
            assert torch.equal(again.float(), (y.float() * world).to(torch.bfloat16).float())
        ca.poll()
        ca.check()
        assert not ca.failed and ca.fused_calls > 0
        torch.distributed.barrier()
        ca.close()
        q.put((rank, None))
    except Exception:
        q.put((rank, traceback.format_exc()))


@pytest.mark.parametrize("world,per_device", PLACEMENTS)
def test_fused_all_reduce_add_rmsnorm_is_bit_identical_to_the_two_step_form(world, per_device):
    """sp_fused_allreduce_add_rmsnorm (the TP path of config 4: o_proj / down_proj all-reduce + the next
    RMSNorm(x, residual), linear.py:1148-1149 -> llama.py:216/222) against sp_custom_all_reduce followed by
    sp_fused_add_rmsnorm: bit-identical x and residual, one-shot and two-shot, eager and replayed from a HIP
    graph.  Ranks sharing this GPU: IPC within one device, NOT a test of xGMI transport (the per-device cases are)."""
    _run_ranks(_fused_main, world, (per_device,))


def _timeout_main(rank, world, port, q):
    try:
        import time
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        os.environ["SP_CUSTOM_ALLREDUCE_TIMEOUT_S"] = "0.5"
        from scratchpad_amd import distributed as d
        from scratchpad_amd.custom_all_reduce import CustomAllReduce
        d.init_distributed_environment(world, rank, f"tcp://127.0.0.1:{port}", 0, backend="gloo")
        d.initialize_model_parallel(world, backend="gloo", local_rank=0)
        torch.cuda.set_device(0)
        tp = d.get_tp_group()
        ca = CustomAllReduce(tp, max_bytes=1 << 20)
        x = torch.ones(64, 1024, dtype=torch.bfloat16, device="cuda")
        y = ca.custom_all_reduce(x)                     # a healthy call first
        torch.cuda.synchronize()
        assert float(y[0, 0]) == world
        ca.poll()
        tp.barrier()
        if rank == 0:
            # rank 1 does not show up for this call: the barrier gives up after 0.5 s of WALL CLOCK, publishes the
            # failure to both regions and to this rank's host word
            t0 = time.perf_counter()
            ca.custom_all_reduce(x)
            torch.cuda.synchronize()
            waited = time.perf_counter() - t0
            assert 0.3 <= waited <= 10.0, f"time-out of 0.5 s took {waited:.2f} s"
            with pytest.raises(RuntimeError, match="timed out"):
                ca.poll()                               # no synchronisation needed: a pinned host word
            assert ca.failed
            with pytest.raises(RuntimeError, match="failed earlier"):
                ca.custom_all_reduce(x)                 # no silent change of transport on one rank
        tp.barrier()
        if rank == 1:
            # the peer's failure reached this rank's region: its next launch does not wait, raises the host word
            t0 = time.perf_counter()
            ca.custom_all_reduce(x)
            torch.cuda.synchronize()
            assert time.perf_counter() - t0 < 0.3, "a launch after a published failure must not wait for the peer"
            with pytest.raises(RuntimeError, match="timed out"):
                ca.poll()
        tp.barrier()
        try:
            ca.close()
        except RuntimeError:
            pass                                        # close() checks the region once more: failed, as expected
        q.put((rank, None))
    except Exception:
        q.put((rank, traceback.format_exc()))


def test_direct_all_reduce_timeout_is_published_to_every_rank():
    """a barrier time-out must not stay rank-local and silent.  Rank 1 skips a collective;
    rank 0's kernel gives up after the configured wall-clock bound, raises both regions' status words and its
    host word; poll() (a host-memory read) raises on rank 0, and rank 1 learns of it at its next launch."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_timeout_main, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = [q.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    for rank, err in results:
        assert err is None, f"rank {rank}:\n{err}"


# config 4's attention at its real head counts (Llama-3-70B: 64 query / 8 KV heads of 128, hidden 8192 - per rank
# at TP = 8: 8 query heads over 1 KV head, the shape of decode_mfma_kernel's split-keys path), two layers, MLP and
# vocabulary cut down so the unsharded fp32 oracle stays in test time
WIDE = dict(hidden=8192, inter=2048, layers=2, Hq=64, Hkv=8, vocab=2048)


def _wide_weights(seed=9):
    """fan-in-scaled weights, the same on every rank (full, unsharded state dict; load_full_state_dict shards it)"""
    g = torch.Generator().manual_seed(seed)
    H, I, V, D = WIDE["hidden"], WIDE["inter"], WIDE["vocab"], 128
    rnd = lambda rows, cols, gain=1.0: torch.randn(rows, cols, generator=g) * (gain / cols ** 0.5)
    w = {"model.embed_tokens.weight": torch.randn(V, H, generator=g), "model.norm.weight": torch.ones(H),
         "lm_head.weight": rnd(V, H, 3.0)}
    for l in range(WIDE["layers"]):
        pre = f"model.layers.{l}."
        w[pre + "self_attn.qkv_proj.weight"] = rnd((WIDE["Hq"] + 2 * WIDE["Hkv"]) * D, H)
        w[pre + "self_attn.o_proj.weight"] = rnd(H, WIDE["Hq"] * D)
        w[pre + "mlp.gate_up_proj.weight"] = rnd(2 * I, H)
        w[pre + "mlp.down_proj.weight"] = rnd(H, I)
        w[pre + "input_layernorm.weight"] = torch.ones(H)
        w[pre + "post_attention_layernorm.weight"] = torch.ones(H)
    return w


def _rccl_main(rank, world, port, q, custom_ar, wide=False, dt="f32", backend="nccl"):
    """TP over RCCL with one GPU per rank: sharded forward vs the unsharded oracle, eager and under
    HIP-graph replay with the all-reduces captured inside the graph.  wide: config 4's head counts (WIDE).
    backend "gloo": the same flow with all ranks on cuda:0 (what a one-GPU box can run of it; the graph part only
    with the direct all-reduce - gloo collectives cannot be captured)."""
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        os.environ["SP_CUSTOM_ALLREDUCE"] = "1" if custom_ar else "0"
        os.environ["SP_CUSTOM_ALLREDUCE_FUSE_NORM"] = "1" if custom_ar else "0"
        from oracle import llama as ollama, ops
        from scratchpad_amd import distributed as d
        from scratchpad_amd.forward_info import ForwardMode, ModelWorkerBatch
        from scratchpad_amd.model_runner import ModelConfig, ModelRunner, ServerArgs, TpModelWorker
        from tests import smoke_impl
        dtype = {"f32": torch.float32, "bf16": torch.bfloat16}[dt]
        gpu = rank if backend == "nccl" else 0
        torch.cuda.set_device(gpu)
        d.init_distributed_environment(world, rank, f"tcp://127.0.0.1:{port}", gpu, backend=backend)
        d.initialize_model_parallel(world, backend=backend, local_rank=gpu)
        if wide:
            shape = ollama.LlamaShape(WIDE["hidden"], WIDE["inter"], WIDE["layers"], WIDE["Hq"], WIDE["Hkv"],
                                      WIDE["vocab"], False, 500000.0, None, 512, 1e-5)
            w = _wide_weights()
            lens, ctx_len, pool = [70, 37], 128, 256          # > 64 keys: the decode step splits and merges
        else:
            g, pfx, shape, w = smoke_impl.load_case("b")
            lens, ctx_len, pool = [7, 4], 60, 96
        cfg = ModelConfig(shape.hidden, shape.inter, shape.layers, shape.Hq, shape.Hkv, shape.vocab, context_len=ctx_len,
                          rms_norm_eps=shape.rms_eps, rope_theta=shape.rope_theta, max_position_embeddings=shape.max_pos,
                          tie_word_embeddings=shape.tie)
        mr = ModelRunner(cfg, ServerArgs(max_total_tokens=pool, max_running_requests=4, cuda_graph_bs=[2],
                                         cuda_graph_max_bs=2),
                         tp_rank=rank, tp_size=world, dtype=dtype, gpu_id=gpu, init_weights=False)
        assert mr.token_to_kv_pool.head_num == max(1, shape.Hkv // world)
        mr.model.load_full_state_dict({k: v.to(mr.device) for k, v in w.items()})
        if dtype != torch.float32:                            # the oracle on the values the model holds
            w = {k: v.to(dtype).float() for k, v in w.items()}
        # fp32: the VALU kernels, 1e-4 of the logit scale; bf16: the matrix-core kernels against the fp32 oracle on
        # bf16-rounded weights (what torch's own bf16 evaluation of two layers deviates by: test_gpu_llama_real_width)
        bound = 1e-4 if dtype == torch.float32 else 3e-2
        worker = TpModelWorker(mr)
        dev = mr.device
        gen = torch.Generator().manual_seed(5)
        n0, n1 = lens
        ids = torch.randint(0, shape.vocab, (sum(lens),), generator=gen)
        loc = torch.arange(1, 1 + sum(lens))
        table = mr.req_to_token_pool.req_to_token
        table[0, :n0] = loc[:n0].to(torch.int32).to(dev)
        table[1, :n1] = loc[n0:].to(torch.int32).to(dev)
        req = torch.tensor([0, 1])
        batch = ModelWorkerBatch(bid=1, forward_mode=ForwardMode.EXTEND, input_ids=ids.to(dev),
                                 req_pool_indices=req.to(dev), seq_lens=torch.tensor(lens).to(dev),
                                 out_cache_loc=loc.to(dev), seq_lens_sum=sum(lens), extend_num_tokens=sum(lens),
                                 extend_seq_lens=lens, extend_prefix_lens=[0, 0])
        out, nxt = worker.forward_batch_generation(batch)
        okv = ollama.OracleKV(shape, pool, table.shape[0], table.shape[1])
        okv.req_to_token.copy_(table.cpu())
        ext = torch.tensor(lens, dtype=torch.int32)
        pos, start = ops.compute_position(torch.zeros(2, dtype=torch.int32), ext)
        ref = ollama.forward(shape, w, okv, mode="extend", input_ids=ids, positions=pos, req_pool_indices=req,
                             seq_lens=torch.tensor(lens), out_cache_loc=loc, extend_seq_lens=ext, extend_start_loc=start)
        rel = lambda a, b: float((a.float().cpu() - b).abs().max() / b.abs().max())
        assert rel(out.gather_full_logits(), ref) <= bound, ("prefill over RCCL", rank, rel(out.gather_full_logits(), ref))
        if dtype == torch.float32:
            assert torch.equal(nxt.cpu(), ref.argmax(-1))
        nxt = ref.argmax(-1).to(dev)                          # every rank continues from the oracle's tokens
        loc2 = torch.tensor([sum(lens) + 9, sum(lens) + 10])
        table[0, n0] = int(loc2[0])
        table[1, n1] = int(loc2[1])
        seq2 = torch.tensor([n0 + 1, n1 + 1])
        okv.req_to_token.copy_(table.cpu())
        ref2 = ollama.forward(shape, w, okv, mode="decode", input_ids=nxt.cpu(), positions=ops.clamp_position(seq2),
                              req_pool_indices=req, seq_lens=seq2, out_cache_loc=loc2)

        def decode_once():
            b2 = ModelWorkerBatch(bid=2, forward_mode=ForwardMode.DECODE, input_ids=nxt, req_pool_indices=req.to(dev),
                                  seq_lens=seq2.to(dev), out_cache_loc=loc2.to(dev), seq_lens_sum=int(seq2.sum()))
            return worker.forward_batch_generation(b2)
        out2, n2 = decode_once()                              # eager
        assert rel(out2.gather_full_logits(), ref2) <= bound, ("eager decode over RCCL", rank, rel(out2.gather_full_logits(), ref2))
        if backend == "nccl" or custom_ar:
            mr.init_cuda_graphs()                             # collectives captured inside the graph
            for _ in range(3):
                out3, n3 = decode_once()
                assert rel(out3.gather_full_logits(), ref2) <= bound, ("graph decode over RCCL", rank)
                assert torch.equal(n3, n2)
        ca = d.get_tp_group().ca_comm
        assert (ca is not None) == custom_ar
        if ca is not None:
            ca.check()
            assert ca.calls > 0 and (ca.fused_calls > 0) == ca.fuse_norm
            ca.close()
        torch.distributed.barrier()
        q.put((rank, None))
    except Exception:
        q.put((rank, traceback.format_exc()))


@pytest.mark.parametrize("custom_ar", [False, True], ids=["rccl", "direct-all-reduce"])
@pytest.mark.parametrize("world,wide,dt", [
    pytest.param(2, False, "f32", marks=_needs(2), id="tp2-tiny"),
    pytest.param(2, True, "f32", marks=_needs(2), id="tp2-70b-heads-f32"),
    pytest.param(4, True, "f32", marks=_needs(4), id="tp4-70b-heads-f32"),
    pytest.param(4, True, "bf16", marks=_needs(4), id="tp4-70b-heads-bf16"),
    pytest.param(8, True, "f32", marks=_needs(8), id="tp8-70b-heads-f32"),
    pytest.param(8, True, "bf16", marks=_needs(8), id="tp8-70b-heads-bf16")])
def test_tp_over_rccl_matches_unsharded_oracle(world, wide, dt, custom_ar):
    """One GPU per rank, RCCL (= torch's "nccl" backend) or the direct all-reduce carrying the row-parallel sums:
    ragged prefill, eager decode and HIP-graph decode (collectives inside the graph) against the unsharded oracle.
    tp8-70b-heads is BASELINE config 4's partitioning at its real size: 64 / 8 heads of 128 over 8 ranks, each rank's
    decode attention on the Hq 8 / Hkv 1 shape.  RCCL refuses two ranks on one device, so nothing here runs on a
    one-GPU box (parallel_state.py:256-353, pynccl.py:108-130)."""
    _run_ranks(_rccl_main, world, (custom_ar, wide, dt), timeout=900)


@pytest.mark.parametrize("world,dt,custom_ar", [(2, "bf16", True)], ids=["tp2-bf16-direct-all-reduce-graph"])
def test_70b_head_counts_sharded_on_one_gpu(world, dt, custom_ar):
    """The flow of test_tp_over_rccl_matches_unsharded_oracle's 70b-heads cases with the ranks sharing cuda:0 over
    gloo: everything of config 4's partitioning except the transport (64 / 8 heads of 128 sharded 2 ways: per
    rank Hq 32 / Hkv 4; a TP 4 fp32 variant of this ran green in round 4 and was dropped for its 53 s of four time-sliced
    ranks), so that the cases a TP node will run are not first executed there."""
    _run_ranks(_rccl_main, world, (custom_ar, True, dt, "gloo"), timeout=900)


def _rccl_graph_main(rank, world, port, q):
    """RCCL all-reduce and all-gather captured inside a HIP graph at world >= 2, replayed with fresh inputs and
    with eager collectives between the replays (cuda_graph_runner.py:400-420 captures the model's collectives the
    same way; pynccl.py:108-130 is the call being captured)."""
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        import torch.distributed as dist
        torch.cuda.set_device(rank)
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", world_size=world, rank=rank,
                                device_id=torch.device("cuda", rank))
        gen = torch.Generator().manual_seed(77)            # the same stream on every rank: rank r's input is slice r
        T, H = 128, 8192                                    # config 4's message: [bs 128, hidden 8192] bf16 = 2 MiB
        xs = torch.zeros(T, H, dtype=torch.bfloat16, device="cuda")
        gs = torch.zeros(T, 256, dtype=torch.bfloat16, device="cuda")
        gathered = torch.zeros(world * T, 256, dtype=torch.bfloat16, device="cuda")
        dist.all_reduce(xs)                                 # communicator set-up outside the capture
        dist.all_gather_into_tensor(gathered, gs)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            dist.all_reduce(xs.clone())
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            ys = xs * 2
            dist.all_reduce(ys)
            zs = ys + 1
            dist.all_reduce(zs)                             # two dependent collectives in one graph
            dist.all_gather_into_tensor(gathered, gs)
        for rep in range(4):
            allx = torch.randn(world, T, H, generator=gen).to(torch.bfloat16)
            allg = torch.randn(world, T, 256, generator=gen).to(torch.bfloat16)
            xs.copy_(allx[rank])
            gs.copy_(allg[rank])
            graph.replay()
            torch.cuda.synchronize()
            want = (allx.float() * 2).sum(0)
            err = (ys.float().cpu() - want).abs()
            assert bool((err <= 2.0 ** -7 * want.abs() + 1e-2).all()), ("all-reduce in graph", rank, rep, float(err.max()))
            want2 = (ys.float().cpu() + 1).to(torch.bfloat16).float() * world
            err2 = (zs.float().cpu() - want2).abs()
            assert bool((err2 <= 2.0 ** -7 * want2.abs() + 1e-2).all()), ("second all-reduce in graph", rank, rep)
            assert torch.equal(gathered.cpu(), allg.reshape(world * T, 256)), ("all-gather in graph", rank, rep)
            eager = xs.clone()
            dist.all_reduce(eager)                          # an eager collective between replays
            torch.cuda.synchronize()
            e2 = (eager.float().cpu() - allx.float().sum(0)).abs()
            assert bool((e2 <= 2.0 ** -7 * allx.float().sum(0).abs() + 1e-2).all())
            outs = [None] * world
            dist.all_gather_object(outs, ys.cpu())
            assert all(torch.equal(outs[0], t) for t in outs), "every rank holds the same reduced bits"
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, None))
    except Exception:
        q.put((rank, traceback.format_exc()))


@pytest.mark.parametrize("world", [pytest.param(2, marks=_needs(2)), pytest.param(4, marks=_needs(4)),
                                   pytest.param(8, marks=_needs(8))])
def test_rccl_collectives_inside_a_hip_graph(world):
    """What the single-rank test below cannot show: a captured RCCL all-reduce / all-gather that really exchanges
    data between devices, replayed (needs one GPU per rank: skipped on this pool's one-GPU boxes)."""
    _run_ranks(_rccl_graph_main, world, (), timeout=600)


def _rccl_single_main(port, q):
    """One rank, an RCCL communicator of size 1, collectives forced through the library: the RCCL
    all-reduce inside a captured HIP graph replays (what a 1-GPU box can check of RCCL-in-graph)."""
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        import torch.distributed as dist
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", world_size=1, rank=0,
                                device_id=torch.device("cuda", 0))
        x = torch.randn(128, 8192, device="cuda").to(torch.bfloat16)
        want = x.clone()
        dist.all_reduce(x)                                    # creates the communicator outside capture
        torch.cuda.synchronize()
        assert torch.equal(x, want)
        xs = torch.zeros_like(x)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            dist.all_reduce(xs)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        # thread-local capture mode, as HipGraphRunner uses: the process group's watchdog thread keeps
        # polling events while this thread captures (global mode makes that an error)
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            ys = xs * 2
            dist.all_reduce(ys)
            zs = ys + 1
        for rep in range(3):
            xs.copy_(torch.randn(128, 8192, device="cuda").to(torch.bfloat16))
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(zs, xs * 2 + 1), rep
        dist.destroy_process_group()
        q.put((0, None))
    except Exception:
        q.put((0, traceback.format_exc()))


def test_rccl_all_reduce_inside_a_hip_graph_single_rank():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_rccl_single_main, args=(_free_port(), q))
    p.start()
    import queue as _queue
    err = "no result"
    for _ in range(120):                     # <= 2 minutes, and notice a dead child at once
        try:
            _, err = q.get(timeout=1)
            break
        except _queue.Empty:
            if not p.is_alive():
                err = f"the rank process died (exit code {p.exitcode})"
                break
    p.join(timeout=30)
    if p.is_alive():
        p.kill()
    assert err is None, err
