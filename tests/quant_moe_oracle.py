"""Oracle of the quantised mixture-of-experts kernels (csrc/quant_moe.hip) and of the Llama-Quant-MoE models (TEST
INFRASTRUCTURE ONLY).

The reference cannot produce golden vectors for this model: it hands the expert products to triteia (not part of its
tree) over Marlin-ordered buffers.  Part 1 is therefore the three statements of include/scratchpad_hip.h evaluated in
fp64 on the SAME stored values - the 16-bit x, scales and weights and the integer codes, unpacked by
tests/delta_oracle.dense_codes - with routing by tests/moe_oracle.route / sort_pairs (``rnd`` = to fp32, then to the
activation dtype):

    gate_up   h[p, n]      = rnd(rnd(silu(rnd(sg[n] G))) * rnd(su[n] U))       p: a sorted position of pair t K + k
              G = sum_k x[t, k] q_e[n, k], U the same over row I + n
    down      tmp[pair, n] = rnd(rnd(s[n] sum_k h[p, k] q_e[n, k]) * w[t, k])
    combine   acc = +0; acc = rnd(acc + tmp[t K + j]) over the K pairs in the chosen order; out[t] = rnd(acc + base[t])
              order 0: ascending expert index, ties by k; order 1: j = 0 .. K-1; ids outside [0, E) are skipped

Error model (derived, not fitted).  The products x q are exact in fp32 (an 11-bit by a 4-bit significand).  The kernel
sums them in sp_delta_mm's order, which K alone fixes (tests/delta_oracle.py): super-steps of 256 columns dealt
round-robin to 8 partial sums, a partial sum one chain of v_mfma_f32_16x16x32 (8 per super-step, each counted as 33
sequential fp32 roundings), the 8 partial sums folded in order (7 roundings), one multiplication by the scale and one
spare unit for the second-order terms - delta_oracle's chain without its y_old addition:

    c(K) = 264 ceil(ceil(K / 256) / 8) + 9        eP = c(K) 2^-23 |s| sum |x| |q|       for a product P = s sum x q

The interval is then carried through tests/stream_gemm_oracle.silu_mul_of and down_of unchanged; into the down product
it is carried as tests/moe_oracle.experts does (|W| . eh on top of its own term, |W| = |s| |q|), and through the
combine additions with ``rerr``.  Where the bound is 0 the kernel must match bit for bit.

Part 2 - the whole model in plain torch (``forward``): tests/moe_oracle.forward with the feed-forward block replaced
by the two variants' statements (llama_quant_moe.py:204-257 with the un-sort as intended, llama_naive_quant_moe.py:
140-163), in h's dtype, on the unpacked experts plus the dense base MLP.

Nothing in part 1 imports the package under test."""
import math
from typing import Dict, Optional

import torch

from oracle import ops
from oracle.llama import OracleKV
from tests import delta_oracle, moe_oracle
from tests.helpers import rerr, rnd
from tests.stream_gemm_oracle import down_of, silu_mul_of

ORDER_EXPERT, ORDER_RANK = 0, 1


def depth(K: int) -> int:
    return 264 * math.ceil(math.ceil(K / 256) / 8) + 9


def unpack(packed):
    """(q fp64 [E, N, K] of integers code - 8, s fp64 [E, N]) of a stacked (codes, meta, scales) triple; every
    statement below takes either form"""
    if len(packed) == 2:            # already unpacked: tests that reuse one set of experts unpack it once
        return packed
    codes, meta, scales = packed
    return delta_oracle.dense_codes(codes, meta), scales.detach().cpu().double()


def sort_valid(ids: torch.Tensor, E: int):
    """moe_oracle.sort_pairs over the pairs whose id lies in [0, E): (expert_offsets [E + 1], sorted_pos of those
    pairs).  A pair with any other id is in no group (sp_moe_route never writes one; an integrator's ids may hold one)"""
    flat = ids.reshape(-1).long()
    key = torch.where((flat >= 0) & (flat < E), flat, torch.full_like(flat, E))
    offsets, pos = moe_oracle.sort_pairs(key, E + 1)
    return offsets[: E + 1], pos[: int(offsets[E])]


def product(a64: torch.Tensor, q: torch.Tensor, s: torch.Tensor, ea: Optional[torch.Tensor] = None):
    """(P, eP) fp64 [rows, N] of P = s * (a . q^T): a [rows, K] known to within ea, q [N, K], s [N]"""
    K = a64.shape[1]
    P = (a64 @ q.T) * s
    mag = a64.abs() if ea is None else a64.abs() + ea
    eP = depth(K) * 2.0 ** -23 * s.abs() * (mag @ q.abs().T)
    if ea is not None:
        eP = eP + ea @ (q.abs() * s.abs()[:, None]).T
    return P, eP


def gate_up(x: torch.Tensor, packed13, ids: torch.Tensor):
    """(h, eh) fp64 [T K, I] by SORTED POSITION; rows past the last valid pair are zero with bound 0"""
    dtype = x.dtype
    q13, s13 = unpack(packed13)
    E, inter = q13.shape[0], q13.shape[1] // 2
    x64 = x.detach().cpu().double()
    T, K = ids.shape
    offsets, pos = sort_valid(ids, E)
    h = torch.zeros(T * K, inter, dtype=torch.float64)
    eh = torch.zeros_like(h)
    for e in range(E):
        lo, hi = int(offsets[e]), int(offsets[e + 1])
        if lo == hi:
            continue
        rows = x64[pos[lo:hi] // K]
        G, eG = product(rows, q13[e, :inter], s13[e, :inter])
        U, eU = product(rows, q13[e, inter:], s13[e, inter:])
        h[lo:hi], eh[lo:hi] = silu_mul_of(G, eG, U, eU, dtype)
    return h, eh


def down(h: torch.Tensor, packed2, ids: torch.Tensor, wts: torch.Tensor, dtype, eh: Optional[torch.Tensor] = None):
    """(tmp, et) fp64 [T K, H] by PAIR from h [T K, I] by sorted position (fp64 or stored 16-bit values) known to
    within eh; wts fp32 [T, K] holding values of ``dtype``"""
    q2, s2 = unpack(packed2)
    E, H = q2.shape[0], q2.shape[1]
    h64 = h.detach().cpu().double()
    T, K = ids.shape
    offsets, pos = sort_valid(ids, E)
    w64 = wts.detach().cpu().double().reshape(-1)
    tmp = torch.zeros(T * K, H, dtype=torch.float64)
    et = torch.zeros_like(tmp)
    for e in range(E):
        lo, hi = int(offsets[e]), int(offsets[e + 1])
        if lo == hi:
            continue
        D, eD = product(h64[lo:hi], q2[e], s2[e], None if eh is None else eh[lo:hi])
        pairs = pos[lo:hi]
        tmp[pairs], et[pairs] = down_of(D, eD, w64[pairs], dtype)
    return tmp, et


def combine_order(ids_row, E: int, order: int):
    """the k indices of one token in the order their rows are added"""
    ks = [k for k, e in enumerate(ids_row) if 0 <= int(e) < E]
    return sorted(ks, key=lambda k: (int(ids_row[k]), k)) if order == ORDER_EXPERT else ks


def combine(tmp: torch.Tensor, ids: torch.Tensor, E: int, base: torch.Tensor, order: int, dtype,
            et: Optional[torch.Tensor] = None):
    """(out, bound) fp64 [T, H]; tmp [T K, H] by pair known to within et"""
    t64, b64 = tmp.detach().cpu().double(), base.detach().cpu().double()
    T, K = ids.shape
    out = torch.zeros(T, t64.shape[1], dtype=torch.float64)
    bound = torch.zeros_like(out)
    rows = ids.cpu().tolist()
    for t in range(T):
        acc = torch.zeros(t64.shape[1], dtype=torch.float64)
        b = torch.zeros_like(acc)
        for k in combine_order(rows[t], E, order):
            pre = acc + t64[t * K + k]
            e = b if et is None else b + et[t * K + k]
            acc, b = rnd(pre, dtype), rerr(pre, e, dtype)
        pre = acc + b64[t]
        out[t], bound[t] = rnd(pre, dtype), rerr(pre, b, dtype)
    return out, bound


def experts(x, packed13, packed2, ids, wts, base, order: int):
    """(out, bound) fp64 [T, H] of the whole block behind the router and the base MLP"""
    dtype = x.dtype
    packed13, packed2 = unpack(packed13), unpack(packed2)
    E = packed13[0].shape[0]
    h, eh = gate_up(x, packed13, ids)
    tmp, et = down(h, packed2, ids, wts, dtype, eh)
    return combine(tmp, ids, E, base, order, dtype, et)


def random_packed(E: int, N: int, K: int, dtype, seed: int, scale: float = 0.02):
    """seeded random VALID packed experts written from the format's statement: codes 0..15, every meta nibble p0 < p1,
    positive scales around ``scale``"""
    g = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, 256, (E, N, K // 4), generator=g).to(torch.uint8)
    nib = torch.tensor([p0 | (p1 << 2) for p0 in range(4) for p1 in range(p0 + 1, 4)])
    lo = nib[torch.randint(0, 6, (E, N, K // 8), generator=g)]
    hi = nib[torch.randint(0, 6, (E, N, K // 8), generator=g)]
    meta = (lo | (hi << 4)).to(torch.uint8)
    scales = (scale * (0.5 + torch.rand(E, N, generator=g))).to(dtype)
    return codes, meta, scales


# --------------------------------------------------------------------------- the model
def qlinear(x: torch.Tensor, q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """rnd(s * (x . q^T)) in x's dtype: q [N, K] the integers code - 8, s [N]"""
    return ((x.float() @ q.float().T) * s.float()).to(x.dtype)


def expert_mlp(x, q13, s13, q2, s2):
    return qlinear(ops.silu_and_mul(qlinear(x, q13, s13)), q2, s2)


def base_mlp(x, w13, w2):
    return torch.nn.functional.linear(ops.silu_and_mul(torch.nn.functional.linear(x, w13)), w2)


def sbmm_block(h, gate, base13, base2, q13, s13, q2, s2, top_k: int):
    """LlamaMoE.forward of llama_quant_moe.py:204-257 in h's dtype, the un-sort as intended: token t receives its own
    k-th expert's output times its own k-th weight.  Returns (output, router logits, selected experts)"""
    base_y = base_mlp(h, base13, base2)
    logits = torch.nn.functional.linear(h, gate)
    p = torch.softmax(logits, dim=-1, dtype=torch.float)
    pk, sel = torch.topk(p, top_k)
    wt = (pk / pk.sum(-1, keepdim=True)).to(h.dtype)
    final = torch.zeros_like(h)
    for k in range(top_k):
        y = torch.zeros_like(h)
        for e in range(q13.shape[0]):
            tok = torch.where(sel[:, k] == e)[0]
            if tok.numel():
                y[tok] = expert_mlp(h[tok], q13[e], s13[e], q2[e], s2[e])
        final += wt[:, k:k + 1] * y
    return final + base_y, logits, sel


def naive_block(h, gate, base13, base2, q13, s13, q2, s2, top_k: int):
    """LlamaMoE.forward of llama_naive_quant_moe.py:140-163 in h's dtype"""
    base_y = base_mlp(h, base13, base2)
    logits = torch.nn.functional.linear(h, gate)
    vals, sel = torch.topk(logits, top_k)
    wt = torch.softmax(vals, dim=-1, dtype=torch.float).to(h.dtype)
    results = torch.zeros_like(h)
    for e in range(q13.shape[0]):
        tok, k = torch.where(sel == e)
        if tok.numel() == 0:
            continue
        results[tok] += expert_mlp(h[tok], q13[e], s13[e], q2[e], s2[e]) * wt[tok, k].unsqueeze(-1)
    return results + base_y, logits, sel


BLOCKS = {"llama_quant_moe": sbmm_block, "llama_naive_quant_moe": naive_block}
BASE_SEED = 2


def quant_weights(w: Dict[str, torch.Tensor], shape, seed: int = BASE_SEED) -> Dict[str, torch.Tensor]:
    """The tiny Llama-MoE fixture as a Llama-Quant-MoE checkpoint in the sbmm variant's names: every non-expert tensor
    as it is, the experts ``pack_delta(fixture expert.float(), fp16)`` stacked over E, and a dense base MLP drawn from
    ``torch.Generator().manual_seed(seed)`` - per layer, in order, randn(2 I, H) * 0.05 then randn(H, I) * 0.05, both
    cast to fp16."""
    from scratchpad_amd.delta import pack_delta
    out = {k: v for k, v in w.items() if ".moe.mlp." not in k}
    g = torch.Generator().manual_seed(seed)
    for i in range(shape.layers):
        p = f"model.layers.{i}.moe."
        out[p + "base_mlp.gate_up_proj.weight"] = (torch.randn(2 * shape.inter, shape.hidden, generator=g) * 0.05).half()
        out[p + "base_mlp.down_proj.weight"] = (torch.randn(shape.hidden, shape.inter, generator=g) * 0.05).half()
        for proj in ("gate_up_proj", "down_proj"):
            parts = [pack_delta(w[p + f"mlp.{e}.{proj}.weight"].float(), torch.float16) for e in range(shape.E)]
            for j, leaf in enumerate(("codes", "meta", "scales")):
                out[p + f"mlp.{proj}.{leaf}"] = torch.stack([t[j] for t in parts])
    return out


def naive_names(w: Dict[str, torch.Tensor], E: int) -> Dict[str, torch.Tensor]:
    """the same checkpoint under the naive variant's per-expert names"""
    out = {}
    for k, v in w.items():
        if ".moe.mlp." in k:
            head, rest = k.split(".moe.mlp.")
            for e in range(E):
                out[f"{head}.moe.mlp.{e}.{rest}"] = v[e]
        else:
            out[k] = v
    return out


def swap_experts(w, layer=0, a=0, b=1):
    """the (sbmm-named) checkpoint with experts a and b of ``layer`` exchanged, gate rows left alone"""
    w = dict(w)
    for k in list(w):
        if k.startswith(f"model.layers.{layer}.moe.mlp."):
            v = w[k].clone()
            v[a], v[b] = w[k][b], w[k][a]
            w[k] = v
    return w


def forward(shape, w, kv: OracleKV, block, *, mode, input_ids, positions, req_pool_indices, seq_lens, out_cache_loc,
            extend_seq_lens=None, extend_start_loc=None, trace=None, dtype=torch.float32) -> torch.Tensor:
    """tests/moe_oracle.forward with the feed-forward block replaced by ``block`` (sbmm_block / naive_block); ``w`` in
    quant_weights' names, its floating tensors already in ``dtype``"""
    D, Hq, Hkv = shape.D, shape.Hq, shape.Hkv
    cache = ops.rope_cos_sin_cache(shape.max_pos, shape.rope_theta, D, None, dtype)
    scale = D ** -0.5
    lin = torch.nn.functional.linear
    h = torch.nn.functional.embedding(input_ids, w["model.embed_tokens.weight"])
    residual = None
    for i in range(shape.layers):
        p = f"model.layers.{i}."
        if residual is None:
            residual = h
            h = ops.rmsnorm(h, w[p + "input_layernorm.weight"], shape.rms_eps)
        else:
            h, residual = ops.rmsnorm(h, w[p + "input_layernorm.weight"], shape.rms_eps, residual)
        q, k, v = lin(h, w[p + "self_attn.qkv_proj.weight"]).split([Hq * D, Hkv * D, Hkv * D], dim=-1)
        q, k = ops.rotary_embedding(positions, q, k, D, cache, True)
        ops.kv_store(kv.k[i], kv.v[i], out_cache_loc, k.reshape(-1, Hkv, D), v.reshape(-1, Hkv, D))
        q3 = q.reshape(-1, Hq, D)
        if mode == "decode":
            a = ops.decode_attention(q3, kv.k[i], kv.v[i], kv.req_to_token, req_pool_indices, seq_lens, scale)
        else:
            a = ops.extend_attention(q3, kv.k[i], kv.v[i], kv.req_to_token, req_pool_indices, seq_lens,
                                     extend_seq_lens, extend_start_loc, scale)
        h = lin(a.reshape(-1, Hq * D), w[p + "self_attn.o_proj.weight"])
        h, residual = ops.rmsnorm(h, w[p + "post_attention_layernorm.weight"], shape.rms_eps, residual)
        m = p + "moe."
        q13 = delta_oracle.dense_codes(w[m + "mlp.gate_up_proj.codes"], w[m + "mlp.gate_up_proj.meta"])
        q2 = delta_oracle.dense_codes(w[m + "mlp.down_proj.codes"], w[m + "mlp.down_proj.meta"])
        h, logits, sel = block(h, w[m + "gate.weight"], w[m + "base_mlp.gate_up_proj.weight"],
                               w[m + "base_mlp.down_proj.weight"], q13, w[m + "mlp.gate_up_proj.scales"], q2,
                               w[m + "mlp.down_proj.scales"], shape.K)
        if trace is not None:
            trace.append((logits.float(), sel))
    h, _ = ops.rmsnorm(h, w["model.norm.weight"], shape.rms_eps, residual)
    if mode == "extend":
        h = h[torch.cumsum(extend_seq_lens.long(), 0) - 1]
    head = w["model.embed_tokens.weight"] if shape.tie else w["lm_head.weight"]
    return torch.matmul(h.to(head.dtype), head.T)[:, : shape.vocab].float()


_RUNS = {}


def oracle_run(arch: str, dtype=torch.float32, w=None, name: str = "a"):
    """(prefill logits, decode logits, prefill trace, decode trace) of ``forward`` over the fixture's two steps; runs
    on the unmodified checkpoint are computed once and shared"""
    key = (arch, dtype, name)
    if w is None and key in _RUNS:
        return _RUNS[key]
    g, pfx, shape, w0 = moe_oracle.load_case(name)
    wq = w if w is not None else quant_weights(w0, shape)
    wq = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in wq.items()}
    kv = OracleKV(shape, 96, 4, 64, dtype)
    as_t = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(a)
    ext, req, loc = as_t(g[pfx + "extend_lens"]), as_t(g[pfx + "req_pool_indices"]), as_t(g[pfx + "out_cache_loc"])
    pre = torch.zeros_like(ext)
    ops.write_req_to_token(kv.req_to_token, req, pre, ext, ext, loc)
    positions, start = ops.compute_position(pre, ext)
    t1, t2 = [], []
    block = BLOCKS[arch]
    l1 = forward(shape, wq, kv, block, mode="extend", input_ids=as_t(g[pfx + "input_ids"]), positions=positions,
                 req_pool_indices=req, seq_lens=ext.long(), out_cache_loc=loc, extend_seq_lens=ext,
                 extend_start_loc=start, trace=t1, dtype=dtype)
    seq2 = ext.long() + 1
    dloc = as_t(g[pfx + "decode_out_cache_loc"])
    ops.write_req_to_token(kv.req_to_token, req, ext.long(), seq2, torch.ones_like(seq2), dloc)
    l2 = forward(shape, wq, kv, block, mode="decode", input_ids=as_t(g[pfx + "next_ids"]),
                 positions=ops.clamp_position(seq2), req_pool_indices=req, seq_lens=seq2, out_cache_loc=dloc, trace=t2,
                 dtype=dtype)
    res = (l1, l2, t1, t2)
    if w is None:
        _RUNS[key] = res
    return res


def router_gap(trace, top_k: int) -> float:
    """moe_oracle.min_gap: the smallest distance between the K-th and the (K+1)-th router logit of a trace"""
    return moe_oracle.min_gap(trace, top_k)


def model_config(shape, arch: str):
    from scratchpad_amd.model_runner import ModelConfig
    return ModelConfig(shape.hidden, shape.inter, shape.layers, shape.Hq, shape.Hkv, shape.vocab, context_len=60,
                       head_dim=shape.D, rms_norm_eps=shape.rms_eps, rope_theta=shape.rope_theta,
                       max_position_embeddings=shape.max_pos, tie_word_embeddings=shape.tie, architecture=arch,
                       num_experts=shape.E, experts_per_token=shape.K, expert_layout="sp_delta")


def run_case(arch: str, dtype, graph_bs=None, w=None, name: str = "a"):
    """The fixture's prefill and decode step through ModelRunner -> HipAttnBackend (moe_oracle.run_case's sequence).
    Returns (prefill logits, decode logits, model runner), logits as fp32 CPU tensors."""
    from scratchpad_amd import _native
    from scratchpad_amd.forward_info import ForwardMode, ModelWorkerBatch
    from scratchpad_amd.model_runner import ModelRunner, ServerArgs, TpModelWorker
    g, pfx, shape, w0 = moe_oracle.load_case(name)
    wq = w if w is not None else quant_weights(w0, shape)
    if arch == "llama_naive_quant_moe":
        wq = naive_names(wq, shape.E)
    args = ServerArgs(max_total_tokens=96, max_running_requests=3, disable_cuda_graph=graph_bs is None,
                      cuda_graph_bs=graph_bs)
    mr = ModelRunner(model_config(shape, arch), args, dtype=dtype, init_weights=False)
    mr.model.load_full_state_dict({k: v.to(mr.device) for k, v in wq.items()})
    if graph_bs is not None:
        mr.init_cuda_graphs()
    worker = TpModelWorker(mr)
    dev = mr.device
    ext = torch.from_numpy(g[pfx + "extend_lens"])
    req = torch.from_numpy(g[pfx + "req_pool_indices"]).to(dev)
    loc = torch.from_numpy(g[pfx + "out_cache_loc"]).to(dev)
    ids = torch.from_numpy(g[pfx + "input_ids"]).to(dev)
    seq = ext.long().to(dev)
    _native.write_req_to_token(mr.req_to_token_pool.req_to_token, req, torch.zeros_like(seq), seq, seq, loc)
    batch = ModelWorkerBatch(bid=1, forward_mode=ForwardMode.EXTEND, input_ids=ids, req_pool_indices=req,
                             seq_lens=seq, out_cache_loc=loc, seq_lens_sum=int(ext.sum()),
                             extend_num_tokens=int(ext.sum()), extend_seq_lens=ext.tolist(),
                             extend_prefix_lens=[0] * len(ext))
    out, _ = worker.forward_batch_generation(batch)
    prefill = out.next_token_logits.float().cpu()
    dloc = torch.from_numpy(g[pfx + "decode_out_cache_loc"]).to(dev)
    seq2 = seq + 1
    mr.req_to_token_pool.write((req, seq), dloc.to(torch.int32))
    nxt_in = torch.from_numpy(g[pfx + "next_ids"]).to(dev)
    batch2 = ModelWorkerBatch(bid=2, forward_mode=ForwardMode.DECODE, input_ids=nxt_in, req_pool_indices=req,
                              seq_lens=seq2, out_cache_loc=dloc, seq_lens_sum=int(seq2.sum()))
    out2, _ = worker.forward_batch_generation(batch2)
    return prefill, out2.next_token_logits.float().cpu(), mr
