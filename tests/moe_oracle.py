"""Oracle of the mixture-of-experts kernels and of the Llama-MoE model (TEST INFRASTRUCTURE ONLY).

Part 1 - the four operations of csrc/moe.hip, stated in fp64 on the SAME stored inputs with the reference's rounding
points (nn/models/llama/llama_moe.py:98-120; ``rnd`` = to fp32, then to the activation dtype):

    route     ids[t, :K] = the K largest logits, largest first, the lower index among equals (NaN counts as largest);
              w[t, k] = rnd(exp(l_k - l_0) / sum_j exp(l_j - l_0)), the sum taken in k order
    gate_up   h[p]   = rnd(rnd(silu(rnd(x[t] . Wg[e]))) * rnd(x[t] . Wu[e]))        p: a (token, k) pair of expert e
    down      tmp[p] = rnd(rnd(h[p] . W2[e]) * w[t, k])
    combine   out[t] = the K rows of token t added from zero in ascending expert index, rnd after every addition

Error model (derived, not fitted).  The kernels differ from this statement only in that the two products are summed in
fp32, in an order of their own: a sum of n products carries at most  n 2^-24 sum|a||b|  of error, and silu evaluated in
fp32 at most 8 2^-24 |g|.  Every other step is exact in fp32 (a product of two 16-bit values) or a rounding.  Rounding
is monotone, so a value v known to within e rounds to within  rerr(v, e) = max(|rnd(v + e) - rnd(v)|, |rnd(v) - rnd(v -
e)|)  of rnd(v): ZERO unless v lies within e of a rounding boundary.  The bound of every element is this interval
carried through the chain (silu has slope at most 1.1; a product a b moves by at most ea |b| + eb |a| + ea eb; the down
product by eh . |W2| on top of its own accumulation term).  Where no boundary is near, the bound is 0 and the kernel
must match bit for bit.

Part 2 - the whole model in plain torch (``forward``), the restatement the model tests compare against: llama.py's
oracle with the MLP replaced by the reference's router / top-k / softmax / per-expert loop.  Pinned by
tests/golden/tiny_llama_moe.npz, the logits of the reference's own LlamaMoEForCausalLM (tests/test_moe_host.py).

Nothing in part 1 imports the package under test."""
from typing import Dict, List, Optional

import torch

from oracle import ops
from oracle.llama import LlamaShape, OracleKV
from tests import golden
from tests.helpers import rerr, rnd  # noqa: F401  (shared with tests/stream_gemm_oracle.py)

U32 = 2.0 ** -24


# --------------------------------------------------------------------------- route
def route(logits: torch.Tensor, top_k: int):
    """(ids int64 [T, K], weights fp32 [T, K]) from logits [T, E] of any of the three dtypes"""
    dtype = logits.dtype
    v = logits.detach().cpu().double()
    key = torch.where(torch.isnan(v), torch.full_like(v, float("inf")), v)
    order = torch.sort(-key, dim=1, stable=True).indices          # descending, the lower index first among equals
    ids = order[:, :top_k].contiguous()
    sel = v.gather(1, ids)
    ex = torch.exp(sel - sel[:, :1])
    s = torch.zeros(v.shape[0], dtype=torch.float64)
    for j in range(top_k):
        s = s + ex[:, j]
    w = (ex / s[:, None]).to(torch.float32).to(dtype).to(torch.float32)
    return ids, w


def sort_pairs(ids: torch.Tensor, num_experts: int):
    """(expert_offsets [E + 1], sorted_pos [T K]): the stable sort of the pairs t K + k by expert"""
    flat = ids.reshape(-1).long()
    pos = torch.sort(flat, stable=True).indices
    counts = torch.bincount(flat, minlength=num_experts)
    offsets = torch.zeros(num_experts + 1, dtype=torch.int64)
    offsets[1:] = torch.cumsum(counts, 0)
    return offsets, pos


# --------------------------------------------------------------------------- the grouped MLP
def silu64(g: torch.Tensor) -> torch.Tensor:
    return g / (1.0 + torch.exp(-g))


def experts(x: torch.Tensor, w13: torch.Tensor, w2: torch.Tensor, ids: torch.Tensor, wts: torch.Tensor):
    """(out, bound) fp64 [T, H]: the statement above and the derived bound of every element.  x [T, H], w13 [E, 2 I,
    H], w2 [E, H, I] in the activation dtype; ids [T, K]; wts fp32 [T, K] holding values of that dtype."""
    dtype = x.dtype
    x64, w13_64, w2_64 = x.cpu().double(), w13.cpu().double(), w2.cpu().double()
    T, H = x64.shape
    inter = w2_64.shape[2]
    K = ids.shape[1]
    out = torch.zeros(T, H, dtype=torch.float64)
    bound = torch.zeros(T, H, dtype=torch.float64)
    ids = ids.cpu().long()
    w64 = wts.cpu().double()
    for t in range(T):
        for k in sorted(range(K), key=lambda j: (int(ids[t, j]), j)):         # ascending expert index
            e = int(ids[t, k])
            xa, wg, wu, wd = x64[t], w13_64[e, :inter], w13_64[e, inter:], w2_64[e]
            G, U = wg @ xa, wu @ xa
            eG, eU = H * U32 * (wg.abs() @ xa.abs()), H * U32 * (wu.abs() @ xa.abs())
            g, eg = rnd(G, dtype), rerr(G, eG, dtype)
            u, eu = rnd(U, dtype), rerr(U, eU, dtype)
            s = silu64(g)
            es = 1.1 * eg + 8 * U32 * g.abs()
            sr, esr = rnd(s, dtype), rerr(s, es, dtype)
            prod = sr * u
            eprod = esr * u.abs() + eu * sr.abs() + esr * eu
            h, eh = rnd(prod, dtype), rerr(prod, eprod, dtype)
            D = wd @ h
            eD = wd.abs() @ eh + inter * U32 * (wd.abs() @ (h.abs() + eh))
            d, ed = rnd(D, dtype), rerr(D, eD, dtype)
            scaled = d * w64[t, k]
            tmp, et = rnd(scaled, dtype), rerr(scaled, ed * w64[t, k].abs(), dtype)
            acc = out[t] + tmp
            out[t], bound[t] = rnd(acc, dtype), rerr(acc, bound[t] + et, dtype)
    return out, bound


# --------------------------------------------------------------------------- the model
class MoEShape(LlamaShape):
    """LlamaShape plus the head size the fixture records and the two MoE figures"""

    def __init__(self, hidden, inter, layers, Hq, Hkv, vocab, head_dim, tie, rope_theta, max_pos, rms_eps, E, K):
        super().__init__(hidden, inter, layers, Hq, Hkv, vocab, tie, rope_theta, None, max_pos, rms_eps)
        assert head_dim == self.D
        self.E, self.K = E, K


def moe_block(h: torch.Tensor, gate: torch.Tensor, w13: List[torch.Tensor], w2: List[torch.Tensor], top_k: int):
    """LlamaMoE.forward (llama_moe.py:98-120) in h's dtype; returns (output, router logits, selected experts)"""
    logits = torch.nn.functional.linear(h, gate)
    vals, sel = torch.topk(logits, top_k)
    wt = torch.softmax(vals, dim=-1, dtype=torch.float).to(h.dtype)
    out = torch.zeros_like(h)
    for e in range(len(w13)):
        tok, k = torch.where(sel == e)
        if tok.numel() == 0:
            continue
        act = ops.silu_and_mul(torch.nn.functional.linear(h[tok], w13[e]))
        out[tok] += torch.nn.functional.linear(act, w2[e]) * wt[tok, k].unsqueeze(-1)
    return out, logits, sel


def forward(shape: MoEShape, w: Dict[str, torch.Tensor], kv: OracleKV, *, mode: str, input_ids, positions,
            req_pool_indices, seq_lens, out_cache_loc, extend_seq_lens: Optional[torch.Tensor] = None,
            extend_start_loc: Optional[torch.Tensor] = None, trace: Optional[list] = None) -> torch.Tensor:
    """One forward pass (llama_moe.py:170-192, 219-240, 259-269); next-token logits [bs, vocab] fp32.  ``trace``
    collects (router logits, selected experts) of every layer.  Arguments as oracle.llama.forward."""
    dtype = w["model.embed_tokens.weight"].dtype
    D, Hq, Hkv = shape.D, shape.Hq, shape.Hkv
    cache = ops.rope_cos_sin_cache(shape.max_pos, shape.rope_theta, D, None, dtype)
    scale = D ** -0.5
    h = torch.nn.functional.embedding(input_ids, w["model.embed_tokens.weight"])
    residual = None
    for i in range(shape.layers):
        p = f"model.layers.{i}."
        if residual is None:
            residual = h
            h = ops.rmsnorm(h, w[p + "input_layernorm.weight"], shape.rms_eps)
        else:
            h, residual = ops.rmsnorm(h, w[p + "input_layernorm.weight"], shape.rms_eps, residual)
        qkv = torch.nn.functional.linear(h, w[p + "self_attn.qkv_proj.weight"])
        q, k, v = qkv.split([Hq * D, Hkv * D, Hkv * D], dim=-1)
        q, k = ops.rotary_embedding(positions, q, k, D, cache, True)
        ops.kv_store(kv.k[i], kv.v[i], out_cache_loc, k.reshape(-1, Hkv, D), v.reshape(-1, Hkv, D))
        q3 = q.reshape(-1, Hq, D)
        if mode == "decode":
            a = ops.decode_attention(q3, kv.k[i], kv.v[i], kv.req_to_token, req_pool_indices, seq_lens, scale)
        else:
            a = ops.extend_attention(q3, kv.k[i], kv.v[i], kv.req_to_token, req_pool_indices, seq_lens,
                                     extend_seq_lens, extend_start_loc, scale)
        h = torch.nn.functional.linear(a.reshape(-1, Hq * D), w[p + "self_attn.o_proj.weight"])
        h, residual = ops.rmsnorm(h, w[p + "post_attention_layernorm.weight"], shape.rms_eps, residual)
        h, logits, sel = moe_block(h, w[p + "moe.gate.weight"],
                                   [w[p + f"moe.mlp.{e}.gate_up_proj.weight"] for e in range(shape.E)],
                                   [w[p + f"moe.mlp.{e}.down_proj.weight"] for e in range(shape.E)], shape.K)
        if trace is not None:
            trace.append((logits.float(), sel))
    h, _ = ops.rmsnorm(h, w["model.norm.weight"], shape.rms_eps, residual)
    if mode == "extend":
        h = h[torch.cumsum(extend_seq_lens.long(), 0) - 1]
    head = w["model.embed_tokens.weight"] if shape.tie else w["lm_head.weight"]
    return torch.matmul(h.to(head.dtype), head.T)[:, : shape.vocab].float()


def min_gap(trace, top_k: int) -> float:
    """the smallest distance between the K-th and the (K+1)-th router logit over every decision of a trace"""
    gap = float("inf")
    for logits, _ in trace:
        s = torch.sort(logits.double(), dim=-1, descending=True).values
        gap = min(gap, float((s[:, top_k - 1] - s[:, top_k]).min()))
    return gap


# --------------------------------------------------------------------------- the fixture
_FIXTURE = None


def load_case(name):
    global _FIXTURE
    if _FIXTURE is None:
        _FIXTURE = golden.load("tiny_llama_moe")
    g, pfx = _FIXTURE, name + "_"
    hidden, inter, nl, Hq, Hkv, vocab, tie, D, E, K = (int(x) for x in g[pfx + "cfg"])
    shape = MoEShape(hidden, inter, nl, Hq, Hkv, vocab, D, bool(tie), float(g[pfx + "rope_theta"]),
                     int(g[pfx + "max_pos"]), float(g[pfx + "rms_eps"]), E, K)
    w = {k[len(pfx) + 3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith(pfx + "w::")}
    return g, pfx, shape, w


def run_steps(shape, w, g, pfx, dtype=torch.float32):
    """(prefill logits, decode logits, kv, prefill trace, decode trace) of ``forward`` over the fixture's two steps"""
    w = {k: v.to(dtype) for k, v in w.items()}
    kv = OracleKV(shape, 96, 4, 64, dtype)
    as_t = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(a)
    ext, req, loc = as_t(g[pfx + "extend_lens"]), as_t(g[pfx + "req_pool_indices"]), as_t(g[pfx + "out_cache_loc"])
    pre = torch.zeros_like(ext)
    ops.write_req_to_token(kv.req_to_token, req, pre, ext, ext, loc)
    positions, start = ops.compute_position(pre, ext)
    t1, t2 = [], []
    l1 = forward(shape, w, kv, mode="extend", input_ids=as_t(g[pfx + "input_ids"]), positions=positions,
                 req_pool_indices=req, seq_lens=ext.long(), out_cache_loc=loc, extend_seq_lens=ext,
                 extend_start_loc=start, trace=t1)
    seq2 = ext.long() + 1
    dloc = as_t(g[pfx + "decode_out_cache_loc"])
    ops.write_req_to_token(kv.req_to_token, req, ext.long(), seq2, torch.ones_like(seq2), dloc)
    nxt = as_t(g[pfx + "next_ids"]) if pfx + "next_ids" in g else torch.argmax(l1, -1)
    l2 = forward(shape, w, kv, mode="decode", input_ids=nxt, positions=ops.clamp_position(seq2),
                 req_pool_indices=req, seq_lens=seq2, out_cache_loc=dloc, trace=t2)
    return l1, l2, kv, t1, t2


def oracle_run(name, dtype=torch.float32, w=None):
    g, pfx, shape, w0 = load_case(name)
    return run_steps(shape, w or w0, g, pfx, dtype)


def swap_experts(w, layer=0, a=0, b=1):
    """the weights with experts a and b of ``layer`` exchanged, gate rows left alone"""
    w = dict(w)
    for proj in ("gate_up_proj", "down_proj"):
        ka, kb = (f"model.layers.{layer}.moe.mlp.{e}.{proj}.weight" for e in (a, b))
        w[ka], w[kb] = w[kb], w[ka]
    return w


def model_config(shape: MoEShape):
    from scratchpad_amd.model_runner import ModelConfig
    return ModelConfig(shape.hidden, shape.inter, shape.layers, shape.Hq, shape.Hkv, shape.vocab, context_len=60,
                       head_dim=shape.D, rms_norm_eps=shape.rms_eps, rope_theta=shape.rope_theta,
                       max_position_embeddings=shape.max_pos, tie_word_embeddings=shape.tie,
                       architecture="llama_moe", num_experts=shape.E, experts_per_token=shape.K)


def run_case(name, dtype, graph_bs=None, w=None):
    """The fixture's prefill and decode step through ModelRunner -> HipAttnBackend, as the scheduler hands them over.
    Returns (prefill logits, decode logits, next ids, model runner), logits as fp32 CPU tensors."""
    from scratchpad_amd import _native
    from scratchpad_amd.forward_info import ForwardMode, ModelWorkerBatch
    from scratchpad_amd.model_runner import ModelRunner, ServerArgs, TpModelWorker
    g, pfx, shape, w0 = load_case(name)
    args = ServerArgs(max_total_tokens=96, max_running_requests=3, disable_cuda_graph=graph_bs is None,
                      cuda_graph_bs=graph_bs)
    mr = ModelRunner(model_config(shape), args, dtype=dtype, init_weights=False)
    mr.model.load_full_state_dict({k: v.to(mr.device) for k, v in (w or w0).items()})
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
    out, nxt = worker.forward_batch_generation(batch)
    prefill = out.next_token_logits.float().cpu()
    dloc = torch.from_numpy(g[pfx + "decode_out_cache_loc"]).to(dev)
    seq2 = seq + 1
    mr.req_to_token_pool.write((req, seq), dloc.to(torch.int32))
    nxt_in = torch.from_numpy(g[pfx + "next_ids"]).to(dev)       # the reference's sampled ids
    batch2 = ModelWorkerBatch(bid=2, forward_mode=ForwardMode.DECODE, input_ids=nxt_in, req_pool_indices=req,
                              seq_lens=seq2, out_cache_loc=dloc, seq_lens_sum=int(seq2.sum()))
    out2, _ = worker.forward_batch_generation(batch2)
    return prefill, out2.next_token_logits.float().cpu(), nxt.cpu(), mr
