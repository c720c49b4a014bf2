"""GPU parity (through the C ABI) of paged decode attention and ragged extend attention.

Bars (tests/helpers.py `tol`): fp32 2e-5, fp16 1e-3 relative (the north-star bar), bf16 1e-3 +
2^-8 output quantisation; KV slot indexing is checked bit-exactly through permutation tests."""
import math

import numpy as np
import pytest
import torch

from oracle import ops
from tests import golden
from tests.helpers import assert_attn_close, attn_error_units, DTYPES, T, assert_close, cpu, paged_problem

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def nat():
    from scratchpad_amd import _native
    _native.load()
    return _native


@pytest.fixture(params=["auto", "valu", "mfma"])
def decode_kernel(request, nat):
    """run a test under the library's own kernel choice and with each decode kernel forced
    (sp_debug_set("decode_kernel"); fp32 always takes the VALU kernel)"""
    nat.debug_set("decode_kernel", {"auto": 0, "valu": 1, "mfma": 2}[request.param])
    yield request.param
    nat.debug_set("decode_kernel", 0)


def run_decode(nat, p, scale, cap=0.0, chunk=64, max_len=None, kv_start=None, idx_dtype=None, use_plan=True, ranges=0,
               items=True, k_scale=None, v_scale=None):
    """use_plan (what HipAttnBackend does): the per-step plan + the separate merge launch; without: the static
    (request, split) grid.  ranges > 0: the plan carries the range geometry with that many pieces and the launch is given
    it - THE SHIPPED FORM where the range kernel takes the launch (HipAttnBackend passes sp_decode_ranges()).
    items=False: the plan is built WITHOUT the (request, split) items (max_slots = 0), as the backend builds it for a model
    whose layers all take the range kernel.  k_scale / v_scale: the layer scales of a byte pool."""
    q = p["q"]
    bs, Hq, D = q.shape
    seq, req = p["seq_lens"], p["req_pool_indices"]
    if idx_dtype is not None:
        seq, req = seq.to(idx_dtype), req.to(idx_dtype)
    if max_len is None:
        max_len = int(p["seq_lens"].max())
    slots = None if items else 0
    ws = torch.empty(nat.decode_workspace_bytes(bs, Hq, D, max_len, chunk, slots, ranges), dtype=torch.uint8, device=DEV)
    o = torch.full_like(q, float("nan"))
    plan = None
    if use_plan:   # the per-step plan the backend builds in init_forward_metadata
        plan = torch.empty(nat.decode_plan_bytes(bs, max_len, chunk, slots, ranges) // 4, dtype=torch.int32, device=DEV)
        nat.decode_plan(plan, seq, max_len, chunk, slots, ranges)
    nat.decode_attention(o, q, p["k_buffer"], p["v_buffer"], p["req_to_token"], req, seq, scale, cap,
                         max_len, chunk, ws, kv_start, plan, k_scale=k_scale, v_scale=v_scale, max_slots=slots,
                         ranges=ranges)
    return o


RANGE_KERNEL, ITEM_KERNELS = 3, (1, 2)          # sp_debug_get("decode_last_kernel")


def check_vs_oracle(o, dtype, what, v, fn, rows=None):
    """o against fn(V) under the attention error model (helpers.attn_error_units; A = fn(|V|)); fp32
    outputs keep the plain tolerance of assert_close."""
    sel = (lambda t: t) if rows is None else (lambda t: t[rows])
    ref = fn(v)
    if dtype == torch.float32:
        assert_close(sel(o), sel(ref), dtype, what=what)
        return
    assert_attn_close(sel(o), sel(ref), sel(fn(v.abs())), dtype, what=what)


def check_decode(o, p, scale, dtype, what, cap=0.0, kv_start=None, rows=None):
    c = cpu(p)
    fn = lambda v: ops.decode_attention(c["q"].float(), c["k_buffer"].float(), v, c["req_to_token"],
                                        c["req_pool_indices"], c["seq_lens"], scale, cap,
                                        None if kv_start is None else kv_start.cpu())
    check_vs_oracle(o, dtype, what, c["v_buffer"].float(), fn, rows)


def oracle_decode(p, scale, cap=0.0, kv_start=None, abs_v=False):
    """abs_v: the same attention with |V| (the A of helpers.attn_error_units)"""
    c = cpu(p)
    v = c["v_buffer"].float()
    return ops.decode_attention(c["q"].float(), c["k_buffer"].float(), v.abs() if abs_v else v,
                                c["req_to_token"], c["req_pool_indices"], c["seq_lens"], scale, cap,
                                None if kv_start is None else kv_start.cpu())


def golden_decode_case(g, i, dtype):
    p = dict(q=T(g[f"c{i}_q"], DEV, dtype), k_buffer=T(g[f"c{i}_k_buffer"], DEV, dtype),
             v_buffer=T(g[f"c{i}_v_buffer"], DEV, dtype), req_to_token=T(g[f"c{i}_req_to_token"], DEV),
             req_pool_indices=T(g[f"c{i}_req_pool_indices"], DEV), seq_lens=T(g[f"c{i}_seq_lens"], DEV))
    return p, float(g[f"c{i}_sm_scale"]), float(g[f"c{i}_logit_cap"])


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("chunk", [16, 64, 512])
def test_decode_golden(nat, dt, chunk, decode_kernel):
    """the reference's own Triton decode outputs (decode_attention.py:547-608 run under the interpreter by
    tests/golden/gen_golden.py) through the (request, split) items; inputs are exact in every dtype"""
    dtype = DTYPES[dt]
    g = golden.load("decode_attention")
    for i in range(int(g["num_cases"])):
        p, scale, cap = golden_decode_case(g, i, dtype)
        o = run_decode(nat, p, scale, cap, chunk)
        if dtype == torch.float32:
            assert_close(o, T(g[f"c{i}_o"]), dtype, what=f"decode golden c{i} {dt} chunk={chunk}")
        else:   # the reference's own output is the target; A (same attention over |V|) comes from the oracle
            aref = oracle_decode(p, scale, cap, abs_v=True)
            assert_attn_close(o, T(g[f"c{i}_o"]), aref, dtype, what=f"decode golden c{i} {dt} chunk={chunk}")


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("ranges", [0, 1, 3, "auto"])
@pytest.mark.parametrize("items", [True, False], ids=["items+ranges", "ranges-only"])
def test_decode_golden_through_the_shipped_range_kernel(nat, dt, ranges, items):
    """the reference's own decode vectors through the kernel a default decode step launches.  The same
    five cases (D 64 / 128, groups 1 - 8, decode_attention.py:547-608's outputs) with the plan's range geometry at 1 and 3
    pieces and at the count sp_decode_ranges() asks for - what HipAttnBackend passes - and the launch PROVEN to have been
    the range kernel (sp_debug_get("decode_last_kernel") == 3); the plan built as the backend builds it for Llama / Mllama
    (range section alone) and with the items beside it.  Case 4 carries a logit soft-cap, which the range kernel does not
    take: with the items in the plan the launch falls back to them and gives the bits of ranges = 0; from a plan WITHOUT
    items it is refused (RuntimeError) instead of computing nothing.  ranges = 0 is the item geometry (the anchor)."""
    dtype = DTYPES[dt]
    g = golden.load("decode_attention")
    for i in range(int(g["num_cases"])):
        p, scale, cap = golden_decode_case(g, i, dtype)
        bs, Hq, D = p["q"].shape
        n = nat.decode_ranges(Hq, p["k_buffer"].shape[1], D, dtype) if ranges == "auto" else ranges
        what = f"decode golden c{i} {dt} ranges={n}{'' if items else ' (plan without items)'}"
        if n == 0 and not items:
            continue                                    # (a plan with neither section: nothing to launch)
        if ranges == "auto":
            assert n > 0, "every golden head shape is one the range kernel takes"
        if not items and cap > 0:
            with pytest.raises(RuntimeError, match="sp_decode_attention"):
                run_decode(nat, p, scale, cap, 64, ranges=n, items=False)
            continue
        o = run_decode(nat, p, scale, cap, 64, ranges=n, items=items)
        ran = nat.debug_get("decode_last_kernel")
        if n > 0 and cap == 0:
            assert ran == RANGE_KERNEL, f"{what}: launched kernel {ran}, not the range kernel"
        else:
            assert ran in ITEM_KERNELS, f"{what}: launched kernel {ran}"
            if n > 0:           # the soft-cap case behind a range plan: the bits of the items
                assert torch.equal(o, run_decode(nat, p, scale, cap, 64, ranges=0)), what
        aref = oracle_decode(p, scale, cap, abs_v=True)
        assert_attn_close(o, T(g[f"c{i}_o"]), aref, dtype, what=what)


@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("Hq,Hkv,D", [(32, 8, 128), (8, 1, 128), (32, 8, 64), (8, 8, 128), (4, 2, 64),
                                      (16, 2, 128), (6, 6, 64)])
def test_decode_vs_oracle_ragged(nat, dt, Hq, Hkv, D, decode_kernel):
    dtype = DTYPES[dt]
    lens = [1, 2, 63, 64, 65, 127, 128, 129, 255, 257, 300, 511, 513, 1000, 5, 17]
    p = paged_problem(11, len(lens), Hq, Hkv, D, lens, dtype, DEV)
    scale = 1.0 / math.sqrt(D)
    ref = oracle_decode(p, scale)
    if dtype == torch.float32:
        check = lambda o, what: assert_close(o, ref, dtype, what=what)
    else:       # 16-bit: the tight error model, no allowance scaled by the tensor maximum
        aref = oracle_decode(p, scale, abs_v=True)
        check = lambda o, what: assert_attn_close(o, ref, aref, dtype, what=f"decode {dt} G={Hq // Hkv} D={D} {what}")
    for chunk in (64, 128, 512):
        check(run_decode(nat, p, scale, chunk=chunk), f"chunk {chunk}")
    # graph-mode calling convention: int32 indices, max_seq_len = context length (over-estimate)
    o = run_decode(nat, p, scale, chunk=128, max_len=4096, idx_dtype=torch.int32)
    check(o, "int32 idx / static max_len")


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_decode_properties_production_shape(nat, dt, decode_kernel):
    """Llama-3-8B head shape at batch 64 with contexts up to 4096: size-independent properties."""
    dtype = DTYPES[dt]
    gen = torch.Generator().manual_seed(5)
    bs = 64
    lens = torch.randint(128, 4097, (bs,), generator=gen).tolist()
    lens[0], lens[1] = 4096, 128
    p = paged_problem(6, bs, 32, 8, 128, lens, dtype, DEV)
    scale = 128 ** -0.5
    o512 = run_decode(nat, p, scale, chunk=512)
    # (a) split invariance: any chunking gives the same softmax
    for chunk in (64, 256):
        assert_close(run_decode(nat, p, scale, chunk=chunk), o512.float(), dtype, what=f"split {chunk}",
                     both_rounded=True)
    # (b) spot-check 6 rows against the oracle
    rows = [0, 1, 7, 20, 41, 63]
    sub = {k: (v[rows] if k in ("q", "req_pool_indices", "seq_lens") else v) for k, v in p.items()}
    check_decode(o512[rows], sub, scale, dtype, f"production shape {dt}: rows vs oracle")
    # (c) slot-permutation invariance: relocating every KV row (and the table) changes nothing, bit for bit
    P1 = p["k_buffer"].shape[0]
    perm = torch.randperm(P1 - 1, generator=gen).to(DEV) + 1
    perm = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), perm])     # slot 0 stays the dummy
    p2 = dict(p)
    p2["k_buffer"] = torch.empty_like(p["k_buffer"]); p2["k_buffer"][perm] = p["k_buffer"]
    p2["v_buffer"] = torch.empty_like(p["v_buffer"]); p2["v_buffer"][perm] = p["v_buffer"]
    p2["req_to_token"] = perm[p["req_to_token"].long()].to(torch.int32)
    assert torch.equal(run_decode(nat, p2, scale, chunk=512), o512), "KV page indexing must be bit-exact"
    # (d) convexity: every output lies inside the range of the V rows it attends to
    vmax = p["v_buffer"].float().abs().max()
    assert float(o512.float().abs().max()) <= float(vmax) * (1 + 1e-2)
    # (e) V-linearity: attention(q, K, a*V) == a*attention(q, K, V)  (a = 2: exact in binary fp)
    p3 = dict(p); p3["v_buffer"] = p["v_buffer"] * 2
    o2 = run_decode(nat, p3, scale, chunk=512)
    normal = o512.float().abs() >= 2.0 ** -13          # fp16 subnormals do not scale exactly
    assert torch.equal(o2[normal], (o512 * 2)[normal])
    assert float((o2.float() - 2 * o512.float()).abs().max()) <= 2.0 ** -23


def test_decode_edge_cases(nat, decode_kernel):
    dtype = torch.bfloat16
    scale = 0.1
    # padded graph rows: seq_len = fill value 1 pointing at the dummy slot 0 (req row all zeros)
    p = paged_problem(7, 4, 8, 2, 128, [9, 1, 1, 33], dtype, DEV)
    p["req_to_token"][p["req_pool_indices"][1]] = 0
    p["req_to_token"][p["req_pool_indices"][2]] = 0
    o = run_decode(nat, p, scale, chunk=64)
    assert torch.isfinite(o.float()).all()
    check_decode(o, p, scale, dtype, "padded rows")
    # a zero-length row is left untouched and must not disturb its neighbours
    p = paged_problem(8, 3, 8, 2, 128, [40, 5, 70], dtype, DEV)
    p["seq_lens"][1] = 0
    o = run_decode(nat, p, scale, chunk=64)
    check_decode(o, p, scale, dtype, "neighbours of empty row", rows=[0, 2])
    assert torch.isnan(o[1].float()).all(), "empty row: output untouched (caller pre-filled NaN)"
    # batch of one, one token
    p = paged_problem(9, 1, 32, 8, 128, [1], dtype, DEV)
    o = run_decode(nat, p, scale)
    check_decode(o, p, scale, dtype, "bs=1 len=1")
    # kv_start: encoder-decoder self-attention window [enc, enc+seq)
    p = paged_problem(10, 3, 8, 2, 64, [50, 90, 20], dtype, DEV)
    enc = torch.tensor([7, 0, 13], device=DEV)
    p["seq_lens"] = p["seq_lens"] - enc
    o = run_decode(nat, p, scale, kv_start=enc)
    check_decode(o, p, scale, dtype, "kv_start", kv_start=enc)
    # soft-cap
    p = paged_problem(12, 3, 8, 2, 128, [50, 90, 200], dtype, DEV, scale=3.0)
    check_decode(run_decode(nat, p, scale, cap=20.0), p, scale, dtype, "cap", cap=20.0)
    # large-magnitude scores: online-softmax rescale path (scores jump by > 100 between batches)
    p = paged_problem(13, 2, 4, 1, 128, [300, 77], torch.float32, DEV)
    p["k_buffer"][p["req_to_token"][p["req_pool_indices"][0], 200].long()] *= 40
    assert_close(run_decode(nat, p, 1.0, chunk=512), oracle_decode(p, 1.0), torch.float32, what="spike")


def test_decode_plan_is_exact_and_changes_nothing(nat):
    """plan = the non-empty (request, split) items, full splits first; same bits with or without"""
    lens = [1, 64, 65, 128, 500, 0, 129, 1000, 3, 640]
    p = paged_problem(16, len(lens), 32, 8, 128, [max(l, 1) for l in lens], torch.bfloat16, DEV)
    p["seq_lens"] = torch.tensor(lens, device=DEV)
    chunk = 64
    plan = torch.empty(nat.decode_plan_bytes(len(lens), 1000, chunk) // 4, dtype=torch.int32, device=DEV)
    nat.decode_plan(plan, p["seq_lens"], 1000, chunk)
    pl = plan.cpu().tolist()
    want_full = [(b, c) for b, l in enumerate(lens) for c in range(l // chunk)]
    want_tail = []          # ragged last splits, longest quarter-of-a-chunk class first
    for cls in (3, 2, 1, 0):
        want_tail += [(b, l // chunk) for b, l in enumerate(lens)
                      if l % chunk and ((l % chunk) * 4 - 1) // chunk == cls]
    n, nb = pl[0], len(lens)
    assert n == len(want_full) + len(want_tail) and pl[1] == chunk
    assert pl[2] == n, "word 2: the items the lengths need (= listed: no overflow)"
    assert pl[3] == sum(lens), "word 3: the keys the step gathers per kv head"
    # slot0[b] = first partial slot of request b: the exclusive scan of the requests' split counts
    nsplit = [-(-l // chunk) for l in lens]
    assert pl[4:4 + nb] == [sum(nsplit[:b]) for b in range(nb)]
    got = [(pl[4 + nb + 2 * i], pl[5 + nb + 2 * i]) for i in range(n)]
    assert got == want_full + want_tail
    # 700 requests: the scan crosses several 256-request tiles
    gen = torch.Generator().manual_seed(17)
    seq = torch.randint(0, 900, (700,), generator=gen)
    plan = torch.empty(nat.decode_plan_bytes(700, 900, 128) // 4, dtype=torch.int32, device=DEV)
    nat.decode_plan(plan, seq.to(DEV), 900, 128)
    pl = plan.cpu()
    assert int(pl[0]) == int(((seq + 127) // 128).sum())
    assert torch.equal(pl[4:704].long(), torch.cumsum((seq + 127) // 128, 0) - (seq + 127) // 128)
    items = pl[704:704 + 2 * int(pl[0])].view(-1, 2)
    key = items[:, 0].long() * 100 + items[:, 1].long()
    want = torch.cat([b * 100 + torch.arange((int(l) + 127) // 128) for b, l in enumerate(seq.tolist())])
    assert torch.equal(torch.sort(key).values, torch.sort(want).values), "every item exactly once"
    a = run_decode(nat, p, 0.1, chunk=chunk, use_plan=True)
    b = run_decode(nat, p, 0.1, chunk=chunk, use_plan=False)
    keep = [i for i, l in enumerate(lens) if l > 0]
    assert torch.equal(a[keep], b[keep])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_decode_split_size_travels_in_the_plan(nat, dtype):
    """ABI 4: with a plan the kernels read the split size from the plan, partials go to compact slots
    (slot0[b] + c) and the launch covers `max_slots` items.  One launch geometry (host chunk 64, a slot budget
    from sum(seq_lens)) must give the same bits whatever split size the plan was built with - what graph replay
    relies on when it rebuilds only the plan - and the slot budget is the one derived from sum(seq_lens), far
    below batch x context."""
    lens = [700, 64, 1, 130, 513, 2048, 33]
    bs, Hq, Hkv, D = len(lens), 8, 2, 128
    p = paged_problem(31, bs, Hq, Hkv, D, lens, dtype, DEV)
    q, seq, req = p["q"], p["seq_lens"], p["req_pool_indices"]
    ctx = 131072                                   # the model's context length: the bound the kernels clamp to
    ref = run_decode(nat, p, 0.11, chunk=64, use_plan=False)
    check_decode(ref, p, 0.11, dtype, "static grid")
    static_slots = nat.decode_plan_slots(bs, ctx, 64)
    for chunk in (64, 128, 512, 4096):
        slots = nat.decode_plan_slots(bs, ctx, chunk, kv_tokens=sum(lens))
        assert slots == sum(lens) // chunk + bs and slots * 100 < static_slots
        ws = torch.empty(nat.decode_workspace_bytes(bs, Hq, D, ctx, 64, slots), dtype=torch.uint8, device=DEV)
        plan = torch.empty(nat.decode_plan_bytes(bs, ctx, 64, slots) // 4, dtype=torch.int32, device=DEV)
        nat.decode_plan(plan, seq, ctx, chunk, slots)
        assert int(plan[0]) == sum(-(-l // chunk) for l in lens) <= slots and int(plan[1]) == chunk
        o = torch.full_like(q, float("nan"))
        nat.decode_attention(o, q, p["k_buffer"], p["v_buffer"], p["req_to_token"], req, seq, 0.11, 0.0,
                             ctx, 64, ws, None, plan, max_slots=slots)
        check_decode(o, p, 0.11, dtype, f"plan chunk {chunk}")
        if chunk == 64:
            assert torch.equal(o, ref), "same split size: same bits as the static grid"
    # a slot budget the lengths do not fit at chunk 64 (a broken host bound): the plan kernel doubles the split size
    # until every item fits (ABI 10) - the bits of a plan built at that size with ample slots, and nothing is written
    # past the workspace
    slots = max(8, bs)
    ws = torch.full((nat.decode_workspace_bytes(bs, Hq, D, ctx, 64, slots) + 4096,), 0x7f, dtype=torch.uint8, device=DEV)
    plan = torch.empty(nat.decode_plan_bytes(bs, ctx, 64, slots) // 4, dtype=torch.int32, device=DEV)
    nat.decode_plan(plan, seq, ctx, 64, slots)
    grown = int(plan[1])
    assert grown > 64 and grown & (grown - 1) == 0, f"split size {grown}: 64 x 2^k"
    assert sum(-(-l // (grown // 2)) for l in lens) > slots, "the smallest such size"
    assert int(plan[0]) == int(plan[2]) == sum(-(-l // grown) for l in lens) <= slots
    o = torch.full_like(q, float("nan"))
    nat.decode_attention(o, q, p["k_buffer"], p["v_buffer"], p["req_to_token"], req, seq, 0.11, 0.0,
                         ctx, 64, ws[:nat.decode_workspace_bytes(bs, Hq, D, ctx, 64, slots)], None, plan, max_slots=slots)
    torch.cuda.synchronize()
    assert bool((ws[-4096:] == 0x7f).all()), "nothing written past the workspace"
    check_decode(o, p, 0.11, dtype, f"split size grown to {grown}")
    ample = nat.decode_plan_slots(bs, ctx, grown, kv_tokens=sum(lens))
    ws = torch.empty(nat.decode_workspace_bytes(bs, Hq, D, ctx, 64, ample), dtype=torch.uint8, device=DEV)
    ref_plan = torch.empty(nat.decode_plan_bytes(bs, ctx, 64, ample) // 4, dtype=torch.int32, device=DEV)
    nat.decode_plan(ref_plan, seq, ctx, grown, ample)
    n = 4 + bs + 2 * int(plan[0])
    assert torch.equal(plan[:n].cpu(), ref_plan[:n].cpu()), "the plan of that split size, item for item"
    o_ref = torch.full_like(q, float("nan"))
    nat.decode_attention(o_ref, q, p["k_buffer"], p["v_buffer"], p["req_to_token"], req, seq, 0.11, 0.0,
                         ctx, 64, ws, None, ref_plan, max_slots=ample)
    assert torch.equal(o, o_ref), "the bits of a plan built at the grown split size with ample slots"


def test_decode_rejects_bad_arguments(nat):
    p = paged_problem(14, 2, 8, 2, 128, [5, 9], torch.bfloat16, DEV)
    with pytest.raises(RuntimeError, match="workspace"):
        nat.decode_attention(torch.empty_like(p["q"]), p["q"], p["k_buffer"], p["v_buffer"],
                             p["req_to_token"], p["req_pool_indices"], p["seq_lens"], 0.1, 0.0, 4096, 64,
                             torch.empty(16, dtype=torch.uint8, device=DEV))
    p96 = paged_problem(15, 1, 4, 4, 96, [5], torch.bfloat16, DEV)
    with pytest.raises(RuntimeError, match="unsupported"):
        run_decode(nat, p96, 0.1)


# ----------------------------------------------------------------------------------- extend
def run_extend(nat, q, kb, vb, r2t, req, seq, ext, start, scale, cap=0.0, causal=True, kv_start=None,
               window_left=-1, plan=None, k_scale=None, v_scale=None):
    T_, Hq, D = q.shape
    ws = torch.empty(nat.extend_workspace_bytes(T_, len(seq), Hq, D, q.dtype), dtype=torch.uint8, device=DEV)
    o = torch.full_like(q, float("nan"))
    nat.extend_attention(o, q, kb, vb, r2t, req, seq, ext, start, scale, cap, causal,
                         int(ext.max()), int(seq.max()), ws, kv_start, window_left=window_left, k_scale=k_scale,
                         v_scale=v_scale, plan=plan)
    return o


@pytest.mark.parametrize("Hq,Hkv,D,rows", [(32, 8, 128, 64), (8, 1, 128, 64), (6, 3, 64, 128), (5, 5, 64, 256)])
def test_extend_plan_lists_every_row_block_once_and_changes_nothing(nat, Hq, Hkv, D, rows):
    """sp_extend_plan: every (request, row block) item exactly once; requests longest first, a
    request's row blocks together and last rows first; and the kernel's output with the plan is
    bit-identical to the unplanned launch (the plan only decides which workgroup computes which rows)."""
    dtype = torch.bfloat16
    pre = [0, 64, 300, 0, 5, 129, 0, 700]
    ext = [130, 1, 70, 1, 257, 33, 512, 64]
    p, q, ext_t, start = extend_problem(33, Hq, Hkv, D, pre, ext, dtype)
    plan = nat.extend_plan(ext_t, p["seq_lens"], sum(ext), Hq, Hkv, True)
    host = plan.cpu().tolist()
    count, bm = host[0], host[1]
    assert bm == rows
    assert host[2:6] == [Hq, Hkv, sum(ext), len(ext)], "header: what the plan was built for"
    items = [(host[8 + 2 * i], host[9 + 2 * i]) for i in range(count)]
    want = [(b, rb) for b, e in enumerate(ext) for rb in range((e + bm - 1) // bm)]
    assert sorted(items) == sorted(want) and count == len(want)
    order = []                                   # requests in plan order, each one's blocks contiguous
    for b, rb in items:
        if not order or order[-1][0] != b:
            assert all(b != o[0] for o in order), "a request's row blocks stay together"
            order.append((b, []))
        order[-1][1].append(rb)
    assert all(rbs == sorted(rbs, reverse=True) for _, rbs in order), "last rows first"
    cls = [(pre[b] + ext[b] + 63) // 64 for b, _ in order]
    assert cls == sorted(cls, reverse=True), "longest requests first"
    args = (q, p["k_buffer"], p["v_buffer"], p["req_to_token"], p["req_pool_indices"], p["seq_lens"], ext_t, start,
            D ** -0.5)
    o_plain = run_extend(nat, *args)
    o_plan = run_extend(nat, *args, plan=plan)
    assert torch.isfinite(o_plan.float()).all() and torch.equal(o_plan, o_plain)
    # a stale or foreign plan must never drop rows.  The kernel checks the plan's header against its
    # own launch and, on a mismatch, derives each workgroup's rows by walking the requests: same bits.
    if rows != 64:                                   # built for other head counts (another block size)
        other = nat.extend_plan(ext_t, p["seq_lens"], sum(ext), 32, 8, True)
        if other.numel() >= plan.numel():
            assert torch.equal(run_extend(nat, *args, plan=other), o_plain), "foreign plan: walked, not dropped"
    # built for ANOTHER STEP with the same head counts: other lengths, same token count -> other items
    ext2 = list(reversed(ext))
    ext2_t = torch.tensor(ext2, dtype=torch.int32, device=DEV)
    seq2 = torch.tensor([a + b for a, b in zip(pre, ext2)], device=DEV)
    stale = nat.extend_plan(ext2_t, seq2, sum(ext2), Hq, Hkv, True)
    assert stale.numel() == plan.numel()
    hdr = stale.clone()
    hdr[4] += 1                                       # ... and a plan whose recorded token count differs
    assert torch.equal(run_extend(nat, *args, plan=hdr), o_plain), "plan of another step (header differs)"
    # a plan buffer too small for the launch's grid is refused on the host
    with pytest.raises(RuntimeError, match="workspace"):
        run_extend(nat, *args, plan=plan[:8])


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_extend_deferred_maximum_agrees_with_exact_running_maximum(nat, dt):
    """The extend kernel advances its running row maximum only when a row's maximum grew by more than
    2^6 (the O rescale becomes a rare branch).  Forcing the branch at every growth (threshold 0) and
    with a spike that must trigger it late in the row gives the same result up to the rounding of P."""
    dtype = DTYPES[dt]
    Hq, Hkv, D = 8, 2, 128
    pre, ext = [0, 300], [700, 257]
    p, q, ext_t, start = extend_problem(52, Hq, Hkv, D, pre, ext, dtype)
    # spike: one late key of request 0 matches one late query far better than anything before it
    req0 = int(p["req_pool_indices"][0])
    slot = int(p["req_to_token"][req0, 650])
    p["k_buffer"][slot] = (q[660, :Hkv].float() * 3.0).to(dtype)
    args = (q, p["k_buffer"], p["v_buffer"], p["req_to_token"], p["req_pool_indices"], p["seq_lens"], ext_t, start,
            D ** -0.5)
    try:
        nat.debug_set("extend_defer_x10", 0)
        o_exact = run_extend(nat, *args)
        nat.debug_set("extend_defer_x10", 120)        # P up to 2^12 before a rescale is forced
        o_never = run_extend(nat, *args)
    finally:
        nat.debug_set("extend_defer_x10", -1)
    o_ship = run_extend(nat, *args)
    c = cpu(p)
    fn = lambda v: ops.extend_attention(q.cpu().float(), c["k_buffer"].float(), v, c["req_to_token"],
                                        c["req_pool_indices"], c["seq_lens"], ext_t.cpu(), start.cpu(), D ** -0.5)
    for name, o in (("threshold 0", o_exact), ("shipped", o_ship), ("threshold 12", o_never)):
        check_vs_oracle(o, dtype, f"extend deferred max {dt}, {name}", c["v_buffer"].float(), fn)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("causal_window", [(-1, 0.0), (300, 0.0), (-1, 30.0)])
@pytest.mark.parametrize("D", [128, 64])
def test_extend_dma_ring_and_register_staging_give_the_same_bits(nat, dt, causal_window, D):
    """16-bit pools, D = 128 and (round 3) D = 64: the K/V tiles reach LDS by LDS-DMA into a swizzled four-buffer
    ring (256-byte rows swizzled by the row, 128-byte rows by the row PAIR); byte pools (and either shape with
    sp_debug_set("extend_dma", 0)) stage them through registers into padded rows.  Same tile order, same
    arithmetic: the outputs must be identical, ragged prefixes, sliding window and logit cap included (a wrong
    swizzle or a miscounted wait is what this would catch)."""
    dtype = DTYPES[dt]
    window, cap = causal_window
    Hq, Hkv = 8, 2
    pre, ext = [0, 513, 64, 1], [700, 257, 64, 1]
    p, q, ext_t, start = extend_problem(61, Hq, Hkv, D, pre, ext, dtype)
    args = (q, p["k_buffer"], p["v_buffer"], p["req_to_token"], p["req_pool_indices"], p["seq_lens"], ext_t, start,
            D ** -0.5)
    kw = dict(cap=cap, window_left=window)
    try:
        nat.debug_set("extend_dma", 0)
        o_reg = run_extend(nat, *args, **kw)
    finally:
        nat.debug_set("extend_dma", 1)
    for _ in range(3):     # a miscounted wait shows as run-to-run differences
        o_dma = run_extend(nat, *args, **kw)
        assert torch.equal(o_dma, o_reg)


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
def test_extend_golden(nat, dt):
    dtype = DTYPES[dt]
    g = golden.load("extend_attention")
    for i in range(int(g["num_cases"])):
        args = [T(g[f"c{i}_{n}"], DEV, dtype) for n in ("q", "k_buffer", "v_buffer")]
        idx = [T(g[f"c{i}_{n}"], DEV) for n in ("req_to_token", "req_pool_indices", "seq_lens",
                                                "extend_seq_lens", "extend_start_loc")]
        o = run_extend(nat, *args, *idx, float(g[f"c{i}_sm_scale"]), float(g[f"c{i}_logit_cap"]))
        if dtype == torch.float32:
            assert_close(o, T(g[f"c{i}_o"]), dtype, what=f"extend golden c{i} {dt}")
        else:   # target = the reference's own Triton output; A = the oracle's attention over |V|
            ci = [t.cpu() for t in idx]
            aref = ops.extend_attention(args[0].cpu().float(), args[1].cpu().float(), args[2].cpu().float().abs(),
                                        ci[0], ci[1], ci[2], ci[3], ci[4], float(g[f"c{i}_sm_scale"]),
                                        float(g[f"c{i}_logit_cap"]))
            assert_attn_close(o, T(g[f"c{i}_o"]), aref, dtype, what=f"extend golden c{i} {dt}")


def extend_problem(seed, Hq, Hkv, D, pre, ext, dtype):
    bs = len(pre)
    seq = [a + b for a, b in zip(pre, ext)]
    p = paged_problem(seed, bs, Hq, Hkv, D, seq, dtype, DEV)
    g = torch.Generator().manual_seed(seed + 1)
    q = torch.randn(sum(ext), Hq, D, generator=g).to(dtype).to(DEV)
    ext_t = torch.tensor(ext, dtype=torch.int32, device=DEV)
    start = torch.zeros(bs, dtype=torch.int32, device=DEV)
    start[1:] = torch.cumsum(ext_t[:-1], 0)
    return p, q, ext_t, start


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("Hq,Hkv,D", [(32, 8, 128), (8, 1, 128), (8, 2, 64), (4, 4, 64)])
def test_extend_vs_oracle(nat, dt, Hq, Hkv, D):
    dtype = DTYPES[dt]
    pre = [0, 64, 300, 0, 5, 129]
    ext = [130, 1, 70, 1, 257, 33]            # includes MIXED-style rows (extend_len 1)
    p, q, ext_t, start = extend_problem(21, Hq, Hkv, D, pre, ext, dtype)
    scale = D ** -0.5
    o = run_extend(nat, q, p["k_buffer"], p["v_buffer"], p["req_to_token"], p["req_pool_indices"],
                   p["seq_lens"], ext_t, start, scale)
    c = cpu(p)
    ref = ops.extend_attention(q.cpu().float(), c["k_buffer"].float(), c["v_buffer"].float(),
                               c["req_to_token"], c["req_pool_indices"], c["seq_lens"], ext_t.cpu(),
                               start.cpu(), scale)
    aref = ops.extend_attention(q.cpu().float(), c["k_buffer"].float(), c["v_buffer"].float().abs(),
                                c["req_to_token"], c["req_pool_indices"], c["seq_lens"], ext_t.cpu(),
                                start.cpu(), scale)
    assert_attn_close(o, ref, aref, dtype, what=f"extend ragged {dt} G={Hq // Hkv} D={D}")


def test_extend_cross_attention_and_kv_start(nat):
    """non-causal rows over the encoder slots [0, enc) and causal rows over [enc, enc+seq)
    (flashinfer_backend.py:792-828)"""
    dtype = torch.bfloat16
    Hq, Hkv, D = 8, 2, 128
    enc = [40, 0, 77]
    pre = [3, 10, 0]
    ext = [20, 5, 31]
    seq_dec = [a + b for a, b in zip(pre, ext)]
    total = [e + s for e, s in zip(enc, seq_dec)]
    p = paged_problem(31, 3, Hq, Hkv, D, total, dtype, DEV)
    g = torch.Generator().manual_seed(32)
    q = torch.randn(sum(ext), Hq, D, generator=g).to(dtype).to(DEV)
    ext_t = torch.tensor(ext, dtype=torch.int32, device=DEV)
    start = torch.zeros(3, dtype=torch.int32, device=DEV)
    start[1:] = torch.cumsum(ext_t[:-1], 0)
    enc_t = torch.tensor(enc, dtype=torch.int64, device=DEV)
    seq_t = torch.tensor(seq_dec, dtype=torch.int64, device=DEV)
    c = cpu(p)
    # cross attention: lens = encoder_lens, kv_start = 0, non-causal; request 1 has no encoder tokens
    o = run_extend(nat, q, p["k_buffer"], p["v_buffer"], p["req_to_token"], p["req_pool_indices"], enc_t,
                   ext_t, start, 0.1, causal=False)
    rows = torch.cat([torch.arange(0, 20), torch.arange(25, 56)])      # rows of requests with enc > 0
    check_vs_oracle(o, dtype, "cross", c["v_buffer"].float(),
                    lambda v: ops.extend_attention(q.cpu().float(), c["k_buffer"].float(), v, c["req_to_token"],
                                                   c["req_pool_indices"], enc_t.cpu(), ext_t.cpu(), start.cpu(), 0.1,
                                                   causal=False), rows)
    assert torch.all(o[20:25] == 0), "a request without encoder tokens: its rows are written as zeros"
    # decoder self-attention behind the encoder slots
    o = run_extend(nat, q, p["k_buffer"], p["v_buffer"], p["req_to_token"], p["req_pool_indices"], seq_t,
                   ext_t, start, 0.1, causal=True, kv_start=enc_t)
    check_vs_oracle(o, dtype, "self behind encoder", c["v_buffer"].float(),
                    lambda v: ops.extend_attention(q.cpu().float(), c["k_buffer"].float(), v, c["req_to_token"],
                                                   c["req_pool_indices"], seq_t.cpu(), ext_t.cpu(), start.cpu(), 0.1,
                                                   causal=True, kv_start=enc_t.cpu()))


def test_extend_last_row_equals_decode(nat):
    """the last new token of a request sees exactly what a decode step at that length sees"""
    dtype = torch.float16
    pre, ext = [100, 0], [28, 300]
    p, q, ext_t, start = extend_problem(41, 32, 8, 128, pre, ext, dtype)
    o = run_extend(nat, q, p["k_buffer"], p["v_buffer"], p["req_to_token"], p["req_pool_indices"],
                   p["seq_lens"], ext_t, start, 0.09)
    last = torch.cumsum(ext_t.long(), 0) - 1
    pd = dict(p); pd["q"] = q[last].contiguous()
    od = run_decode(nat, pd, 0.09, chunk=64)
    assert_close(o[last], od.float(), dtype, what="extend last row vs decode")


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("window", [0, 7, 64, 200, 4096])
def test_extend_sliding_window(nat, dt, window):
    """window_left (flashinfer_backend.py:413): the row at kv position p sees [p - window, p].
    fp32 runs the row-stream path, 16-bit the MFMA kernel (first tile / lower mask / skipped tiles)."""
    dtype = DTYPES[dt]
    Hq, Hkv, D = 8, 2, 128
    pre = [0, 64, 300, 0, 5, 129]
    ext = [130, 1, 70, 1, 257, 33]
    p, q, ext_t, start = extend_problem(41, Hq, Hkv, D, pre, ext, dtype)
    scale = D ** -0.5
    o = run_extend(nat, q, p["k_buffer"], p["v_buffer"], p["req_to_token"], p["req_pool_indices"],
                   p["seq_lens"], ext_t, start, scale, window_left=window)
    c = cpu(p)
    check_vs_oracle(o, dtype, f"extend window {window} {dt}", c["v_buffer"].float(),
                    lambda v: ops.extend_attention(q.cpu().float(), c["k_buffer"].float(), v, c["req_to_token"],
                                                   c["req_pool_indices"], c["seq_lens"], ext_t.cpu(), start.cpu(), scale,
                                                   window_left=window))
    if window >= 4096:      # wider than every sequence: identical to no window at all
        full = run_extend(nat, q, p["k_buffer"], p["v_buffer"], p["req_to_token"], p["req_pool_indices"],
                          p["seq_lens"], ext_t, start, scale)
        assert torch.equal(o, full)
    if window == 0:         # only itself: the output is its own V row
        tok = 0
        for b in range(len(ext)):
            req = int(c["req_pool_indices"][b])
            for t in range(ext[b]):
                slot = int(c["req_to_token"][req, pre[b] + t])
                want = c["v_buffer"][slot].float().repeat_interleave(Hq // Hkv, dim=0)
                assert torch.allclose(o[tok].float().cpu(), want, atol=0, rtol=0)
                tok += 1


def test_backend_sliding_window_layers_decode_and_extend():
    """HipAttnBackend with a runner-level sliding_window_size: windowed layers read the last
    window + 1 keys in decode (kv_start = seq_len - len, flashinfer_backend.py:559-577) with their own
    split plan, full layers are unaffected; extend passes window_left."""
    from types import SimpleNamespace
    from scratchpad_amd.attention import HipAttnBackend, RadixAttention
    from scratchpad_amd.forward_info import ForwardMode
    dtype = torch.bfloat16
    Hq, Hkv, D, W = 8, 2, 128, 37
    seq = [5, 38, 39, 500, 120]
    bs = len(seq)
    p = paged_problem(51, bs, Hq, Hkv, D, seq, dtype, DEV)
    pool = SimpleNamespace(dtype=dtype, get_value_buffer=lambda l: p["v_buffer"],
                           get_kv_buffer=lambda l: (p["k_buffer"], p["v_buffer"]))
    cfg = SimpleNamespace(num_attention_heads=Hq, head_dim=D, context_len=1024,
                          get_num_kv_heads=lambda tp: Hkv)
    mr = SimpleNamespace(model_config=cfg, tp_size=1, token_to_kv_pool=pool, device=DEV, sliding_window_size=W)
    be = HipAttnBackend(mr)
    local = RadixAttention(Hq, D, D ** -0.5, Hkv, layer_id=0, sliding_window_size=W)
    full = RadixAttention(Hq, D, D ** -0.5, Hkv, layer_id=1)
    r2t_pool = SimpleNamespace(req_to_token=p["req_to_token"])
    fb = SimpleNamespace(forward_mode=ForwardMode.DECODE, batch_size=bs, seq_lens=p["seq_lens"],
                         seq_lens_cpu=p["seq_lens"].cpu(), seq_lens_sum=sum(seq), encoder_lens=None,
                         encoder_lens_cpu=None, req_pool_indices=p["req_pool_indices"],
                         token_to_kv_pool=pool, req_to_token_pool=r2t_pool, out_cache_loc=None)
    be.init_forward_metadata(fb)
    c = cpu(p)
    q = p["q"]
    o_local = be.forward_decode(q.reshape(bs, -1), None, None, local, fb, save_kv_cache=False).view(bs, Hq, D)
    o_full = be.forward_decode(q.reshape(bs, -1), None, None, full, fb, save_kv_cache=False).view(bs, Hq, D)
    lens = torch.clamp(c["seq_lens"], max=W + 1)
    ref_local = ops.decode_attention(q.cpu().float(), c["k_buffer"].float(), c["v_buffer"].float(), c["req_to_token"],
                                     c["req_pool_indices"], lens, D ** -0.5, kv_start=c["seq_lens"] - lens)
    ref_full = ops.decode_attention(q.cpu().float(), c["k_buffer"].float(), c["v_buffer"].float(), c["req_to_token"],
                                    c["req_pool_indices"], c["seq_lens"], D ** -0.5)
    assert_close(o_local, ref_local, dtype, what="windowed decode layer")
    assert_close(o_full, ref_full, dtype, what="full decode layer next to it")
    assert torch.equal(o_local[:2], o_full[:2]), "sequences shorter than the window are untouched"

    # extend through the same backend: each request's last 3 tokens are new
    ext = [3] * bs
    ext_t = torch.tensor(ext, dtype=torch.int32, device=DEV)
    start = torch.arange(0, 3 * bs, 3, dtype=torch.int32, device=DEV)
    qe = torch.randn(3 * bs, Hq, D, generator=torch.Generator().manual_seed(52)).to(dtype).to(DEV)
    fbe = SimpleNamespace(forward_mode=ForwardMode.EXTEND, batch_size=bs, seq_lens=p["seq_lens"],
                          seq_lens_cpu=p["seq_lens"].cpu(), seq_lens_sum=sum(seq), encoder_lens=None,
                          encoder_lens_cpu=None, req_pool_indices=p["req_pool_indices"],
                          token_to_kv_pool=pool, req_to_token_pool=r2t_pool, out_cache_loc=None,
                          extend_seq_lens=ext_t, extend_start_loc=start, extend_seq_lens_cpu=ext,
                          extend_prefix_lens_cpu=[s - 3 for s in seq], extend_num_tokens=3 * bs)
    be.init_forward_metadata(fbe)
    oe = be.forward_extend(qe.reshape(3 * bs, -1), None, None, local, fbe, save_kv_cache=False).view(-1, Hq, D)
    ref = ops.extend_attention(qe.cpu().float(), c["k_buffer"].float(), c["v_buffer"].float(), c["req_to_token"],
                               c["req_pool_indices"], c["seq_lens"], ext_t.cpu(), start.cpu(), D ** -0.5,
                               window_left=W)
    assert_close(oe, ref, dtype, what="windowed extend layer")


def test_backend_plans_items_only_for_a_model_with_a_soft_cap_layer(nat):
    """HipAttnBackend.plan_items (round 6): a model whose layers all take the range kernel gets plans without the
    (request, split) items; ONE layer with a logit soft-cap (Gemma-2 style) makes the backend plan them too - that layer's
    launches run the items, its neighbours stay on the range kernel, both against the oracle - and a backend told there are
    no items refuses the capped launch instead of computing nothing."""
    from types import SimpleNamespace
    from scratchpad_amd.attention import HipAttnBackend, RadixAttention
    from scratchpad_amd.forward_info import ForwardMode
    dtype = torch.bfloat16
    Hq, Hkv, D = 8, 2, 128
    seq = [5, 380, 39, 900, 120, 1]
    bs = len(seq)
    p = paged_problem(61, bs, Hq, Hkv, D, seq, dtype, DEV, scale=2.0)
    pool = SimpleNamespace(dtype=dtype, get_value_buffer=lambda l: p["v_buffer"],
                           get_kv_buffer=lambda l: (p["k_buffer"], p["v_buffer"]))
    cfg = SimpleNamespace(num_attention_heads=Hq, head_dim=D, context_len=1024, get_num_kv_heads=lambda tp: Hkv)
    plain = RadixAttention(Hq, D, D ** -0.5, Hkv, layer_id=0)
    capped = RadixAttention(Hq, D, D ** -0.5, Hkv, layer_id=1, logit_cap=20.0)
    fb = SimpleNamespace(forward_mode=ForwardMode.DECODE, batch_size=bs, seq_lens=p["seq_lens"], seq_lens_cpu=None,
                         seq_lens_sum=sum(seq), encoder_lens=None, encoder_lens_cpu=None,
                         req_pool_indices=p["req_pool_indices"], token_to_kv_pool=pool,
                         req_to_token_pool=SimpleNamespace(req_to_token=p["req_to_token"]), out_cache_loc=None)
    q = p["q"].reshape(bs, -1)

    def backend(layers):
        model = torch.nn.Module()
        model.layers = torch.nn.ModuleList(layers)
        return HipAttnBackend(SimpleNamespace(model_config=cfg, tp_size=1, token_to_kv_pool=pool, device=DEV,
                                              dtype=dtype, model=model))

    be = backend([plain])
    assert be.decode_ranges > 0 and be.plan_items is False
    be.init_forward_metadata(fb)
    plan, slots, _, ranges = be.forward_metadata[3][0]
    assert slots == 0 and ranges == be.decode_ranges and plan[:4].tolist()[0] == 0, "the range section alone"
    o = be.forward_decode(q, None, None, plain, fb, save_kv_cache=False).view(bs, Hq, D)
    assert nat.debug_get("decode_last_kernel") == RANGE_KERNEL
    check_decode(o, p, D ** -0.5, dtype, "plain layer, plan without items")
    with pytest.raises(RuntimeError, match="plans no .request, split. items"):
        be.forward_decode(q, None, None, capped, fb, save_kv_cache=False)       # no items were planned for it

    be = backend([plain, capped])
    assert be.plan_items is True
    be.init_forward_metadata(fb)
    assert be.forward_metadata[3][0][1] > 0, "the items are planned beside the ranges"
    o = be.forward_decode(q, None, None, plain, fb, save_kv_cache=False).view(bs, Hq, D)
    assert nat.debug_get("decode_last_kernel") == RANGE_KERNEL, "the plain layer keeps the range kernel"
    check_decode(o, p, D ** -0.5, dtype, "plain layer beside a capped one")
    oc = be.forward_decode(q, None, None, capped, fb, save_kv_cache=False).view(bs, Hq, D)
    assert nat.debug_get("decode_last_kernel") in ITEM_KERNELS
    check_decode(oc, p, D ** -0.5, dtype, "capped layer on the items", cap=20.0)


def test_random_shapes_decode_and_extend_against_oracle(nat):
    """40 seeded random problems: head layout, head size, dtype, batch, ragged lengths (including
    empty prefixes, single keys, lengths straddling chunk/tile edges), soft cap, kv_start offsets,
    causal / cross form, sliding window, chunk size and plan on/off - each against the oracle."""
    import random
    rnd = random.Random(2024)
    layouts = [(32, 8), (8, 8), (8, 1), (16, 2), (4, 4), (8, 2), (16, 16)]
    for case in range(40):
        Hq, Hkv = rnd.choice(layouts)
        D = rnd.choice([64, 128])
        dt = rnd.choice(["bf16", "f16", "f32"] if case % 5 == 0 else ["bf16", "f16"])
        dtype = DTYPES[dt]
        bs = rnd.choice([1, 2, 3, 5, 9, 17])
        edge = [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 511, 512, 513, 700]
        cap = rnd.choice([0.0, 0.0, 30.0])
        scale = D ** -0.5 * rnd.choice([1.0, 0.5])
        what = f"case {case}: Hq{Hq} Hkv{Hkv} D{D} {dt} bs{bs} cap{cap}"
        if rnd.random() < 0.5:      # ---- decode
            lens = [rnd.choice(edge) for _ in range(bs)]
            off = [rnd.choice([0, 0, 3, 40]) for _ in range(bs)]
            p = paged_problem(1000 + case, bs, Hq, Hkv, D, [l + o for l, o in zip(lens, off)], dtype, DEV)
            p["seq_lens"] = torch.tensor(lens, device=DEV)
            kv_start = torch.tensor(off, device=DEV) if any(off) else None
            chunk = rnd.choice([64, 128, 512])
            o = run_decode(nat, p, scale, cap=cap, chunk=chunk, kv_start=kv_start, use_plan=rnd.random() < 0.7)
            check_decode(o, p, scale, dtype, what + f" decode chunk{chunk}", cap=cap, kv_start=kv_start)
        else:                       # ---- extend
            ext = [rnd.choice([1, 2, 31, 32, 33, 64, 127, 130, 200]) for _ in range(bs)]
            causal = rnd.random() < 0.75
            pre = [rnd.choice([0, 0, 1, 63, 64, 65, 300]) for _ in range(bs)]
            window = rnd.choice([-1, -1, 0, 5, 64, 100]) if causal else -1
            if causal:
                seq = [a + b for a, b in zip(pre, ext)]
            else:
                seq = [rnd.choice([0, 1, 64, 65, 300]) for _ in range(bs)]     # encoder lengths, may be empty
            p = paged_problem(2000 + case, bs, Hq, Hkv, D, [max(s, 1) for s in seq], dtype, DEV)
            p["seq_lens"] = torch.tensor(seq, device=DEV)
            g = torch.Generator().manual_seed(3000 + case)
            q = torch.randn(sum(ext), Hq, D, generator=g).to(dtype).to(DEV)
            ext_t = torch.tensor(ext, dtype=torch.int32, device=DEV)
            start = torch.zeros(bs, dtype=torch.int32, device=DEV)
            start[1:] = torch.cumsum(ext_t[:-1], 0)
            T_, = (sum(ext),)
            ws = torch.empty(nat.extend_workspace_bytes(T_, bs, Hq, D, dtype), dtype=torch.uint8, device=DEV)
            o = torch.zeros_like(q)            # rows without any visible key stay zero (cross-attention contract)
            nat.extend_attention(o, q, p["k_buffer"], p["v_buffer"], p["req_to_token"], p["req_pool_indices"],
                                 p["seq_lens"], ext_t, start, scale, cap, causal, max(ext), max(max(seq), 1), ws,
                                 None, window_left=window)
            c = cpu(p)
            check_vs_oracle(o, dtype, what + f" extend causal{causal} window{window}", c["v_buffer"].float(),
                            lambda v: ops.extend_attention(q.cpu().float(), c["k_buffer"].float(), v, c["req_to_token"],
                                                           c["req_pool_indices"], c["seq_lens"], ext_t.cpu(), start.cpu(),
                                                           scale, cap, causal=causal, window_left=window))


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("Hq,Hkv,D", [(16, 1, 128), (32, 2, 128), (12, 2, 64), (24, 8, 128), (10, 2, 128)])
def test_decode_wide_and_odd_groups_on_the_matrix_core_kernel(nat, dt, Hq, Hkv, D):
    """Query-head groups that are not 1/2/4/8 (up to 16 heads per KV head, e.g. Llama-3.1-405B's 128/8):
    the MFMA decode kernel carries the group as tile columns, so any width <= 16 works."""
    nat.debug_set("decode_kernel", 0)
    dtype = DTYPES[dt]
    lens = [1, 17, 64, 65, 300, 513, 1000, 129]
    p = paged_problem(81, len(lens), Hq, Hkv, D, lens, dtype, DEV)
    scale = D ** -0.5
    for chunk, use_plan in ((64, True), (256, False)):
        check_decode(run_decode(nat, p, scale, chunk=chunk, use_plan=use_plan), p, scale, dtype,
                     f"decode {dt} G={Hq // Hkv} chunk {chunk}")
    if Hq // Hkv > 8:
        with pytest.raises(RuntimeError, match="unsupported"):      # fp32 keeps the 8-head limit
            p32 = paged_problem(82, 2, Hq, Hkv, D, [5, 9], torch.float32, DEV)
            run_decode(nat, p32, scale)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("Hq,Hkv,D", [(16, 1, 128), (12, 2, 64), (24, 8, 128), (10, 2, 128), (32, 2, 128)])
def test_extend_wide_and_odd_groups(nat, dt, Hq, Hkv, D):
    """Group widths other than 1/2/4/8: the tile kernel takes 4, 2 or 1 heads per workgroup and spreads
    the remaining head blocks over the grid."""
    dtype = DTYPES[dt]
    pre = [0, 64, 300, 5]
    ext = [130, 1, 70, 257]
    p, q, ext_t, start = extend_problem(91, Hq, Hkv, D, pre, ext, dtype)
    scale = D ** -0.5
    o = run_extend(nat, q, p["k_buffer"], p["v_buffer"], p["req_to_token"], p["req_pool_indices"],
                   p["seq_lens"], ext_t, start, scale)
    c = cpu(p)
    check_vs_oracle(o, dtype, f"extend {dt} G={Hq // Hkv}", c["v_buffer"].float(),
                    lambda v: ops.extend_attention(q.cpu().float(), c["k_buffer"].float(), v, c["req_to_token"],
                                                   c["req_pool_indices"], c["seq_lens"], ext_t.cpu(), start.cpu(), scale))


def test_long_context_decode_and_extend(nat):
    """Contexts far beyond the headline range (40 k keys): many splits per request in decode, hundreds
    of key tiles per row block in extend, slot ids past 2^16."""
    dtype = torch.bfloat16
    Hq, Hkv, D = 32, 8, 128
    lens = [40000, 33001, 7]
    p = paged_problem(97, 3, Hq, Hkv, D, lens, dtype, DEV, scale=0.5)
    scale = D ** -0.5
    for chunk in (512, 64):
        check_decode(run_decode(nat, p, scale, chunk=chunk), p, scale, dtype, f"long decode chunk {chunk}")
    # extend: 300 new tokens behind a 39,700-token cached prefix, and a short companion request
    ext = [300, 5, 7]
    pre = [lens[0] - 300, lens[1] - 5, 0]
    g = torch.Generator().manual_seed(98)
    q = (torch.randn(sum(ext), Hq, D, generator=g) * 0.5).to(dtype).to(DEV)
    ext_t = torch.tensor(ext, dtype=torch.int32, device=DEV)
    start = torch.tensor([0, 300, 305], dtype=torch.int32, device=DEV)
    o = run_extend(nat, q, p["k_buffer"], p["v_buffer"], p["req_to_token"], p["req_pool_indices"], p["seq_lens"],
                   ext_t, start, scale)
    c = cpu(p)
    check_vs_oracle(o, dtype, "long-prefix extend", c["v_buffer"].float(),
                    lambda v: ops.extend_attention(q.cpu().float(), c["k_buffer"].float(), v, c["req_to_token"],
                                                   c["req_pool_indices"], c["seq_lens"], ext_t.cpu(), start.cpu(), scale))
    assert pre[0] == 39700


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_decode_plan_fuzz_planned_equals_static_bit_for_bit(nat, seed):
    """Randomised batches through the round-3 split geometry: up to 700 requests (the plan's scans cross several
    256-request tiles, slot0 is an exclusive scan over all of them), lengths 0 .. 900 with empty and one-token rows,
    a tight slot budget (sum / chunk + bs), int32 and int64 index tensors, a kv_start window.  The planned launch
    (items listed longest first, compact slots) must give the SAME BITS as the static (request, split) grid with the
    same split size, and the plan's header must agree with a host-side recount."""
    g = torch.Generator().manual_seed(100 + seed)
    bs = [37, 300, 700][seed]
    chunk = [64, 128, 256][seed]
    Hq, Hkv, D = [(8, 2, 128), (32, 8, 128), (4, 4, 64)][seed]
    lens = torch.randint(0, 901, (bs,), generator=g)
    lens[torch.randint(0, bs, (bs // 10,), generator=g)] = 0           # empty rows (left untouched by the kernels)
    lens[torch.randint(0, bs, (bs // 10,), generator=g)] = 1
    lens[0] = 900
    start = torch.randint(0, 5, (bs,), generator=g)                   # a small kv_start window in front of every row
    p = paged_problem(200 + seed, bs, Hq, Hkv, D, [int(l) + 5 for l in lens], torch.bfloat16, DEV)
    seq = lens.to(DEV)
    q, req = p["q"], p["req_pool_indices"]
    max_len = 900
    for idx_dtype in (torch.int64, torch.int32):
        s_, r_, k0 = seq.to(idx_dtype), req.to(idx_dtype), start.to(DEV).to(idx_dtype)
        ws = torch.empty(nat.decode_workspace_bytes(bs, Hq, D, max_len, chunk), dtype=torch.uint8, device=DEV)
        o_static = torch.zeros_like(q)
        nat.decode_attention(o_static, q, p["k_buffer"], p["v_buffer"], p["req_to_token"], r_, s_, 0.09, 0.0,
                             max_len, chunk, ws, k0, None)
        slots = nat.decode_plan_slots(bs, max_len, chunk, kv_tokens=int(lens.sum()))
        nsplit = (lens + chunk - 1) // chunk
        ws2 = torch.empty(nat.decode_workspace_bytes(bs, Hq, D, max_len, chunk, slots), dtype=torch.uint8, device=DEV)
        plan = torch.empty(nat.decode_plan_bytes(bs, max_len, chunk, slots) // 4, dtype=torch.int32, device=DEV)
        nat.decode_plan(plan, s_, max_len, chunk, slots)
        host = plan.cpu()
        assert int(host[0]) == int(host[2]) == int(nsplit.sum()) <= slots and int(host[1]) == chunk
        assert int(host[3]) == int(lens.sum())
        assert torch.equal(host[4:4 + bs].long(), torch.cumsum(nsplit, 0) - nsplit)
        for rep in range(2):                               # launch after launch on one plan, as the layers of a step
            ws2.fill_(0x7f)                                # stale partials of "another layer"
            o_plan = torch.zeros_like(q)
            nat.decode_attention(o_plan, q, p["k_buffer"], p["v_buffer"], p["req_to_token"], r_, s_, 0.09, 0.0,
                                 max_len, chunk, ws2, k0, plan, max_slots=slots)
            assert torch.isfinite(o_plan.float()).all() and torch.equal(o_plan, o_static), (seed, idx_dtype, rep)
        assert torch.equal(plan.cpu(), host), "a launch leaves its plan untouched (ABI 7: the plan is read-only)"
    # and against the oracle on a handful of rows (the longest, an empty one, a one-token one)
    rows = [0, int((lens == 0).nonzero()[0]), int((lens == 1).nonzero()[0]), bs - 1]
    c = cpu(p)
    ref = ops.decode_attention(c["q"].float(), c["k_buffer"].float(), c["v_buffer"].float(), c["req_to_token"],
                               c["req_pool_indices"], lens, 0.09, 0.0, start)
    live = [r for r in rows if int(lens[r]) > 0]
    assert_close(o_plan[live], ref[live], torch.bfloat16, what=f"decode fuzz seed {seed}")
    assert float(o_plan[rows[1]].float().abs().max()) == 0.0, "an empty row is left untouched"


@pytest.mark.parametrize("kv", ["same", "fp8"])
@pytest.mark.parametrize("Hq,Hkv,D", [(8, 1, 128), (32, 8, 128), (24, 4, 64), (6, 2, 64)])
def test_decode_streaming_gathers_change_no_bit(nat, kv, Hq, Hkv, D):
    """Non-temporal K/V gathers (chosen per launch from the plan's key count against sp_debug_set("decode_nt_min_mb")):
    the same loop with another cache policy on its loads - always, never and the default give the same bits, in both
    forms of the kernel (a wave per kv head / the waves split one head's keys) and on a byte pool; the clamp of a
    device-side length above max_seq_len counts the clamped length."""
    g = torch.Generator().manual_seed(Hq + 7 * Hkv)
    bs, chunk, max_len = 40, 128, 1500
    lens = torch.randint(1, 1200, (bs,), generator=g)
    lens[:3] = torch.tensor([1500, 1, 129])
    p = paged_problem(500 + Hq, bs, Hq, Hkv, D, lens.tolist(), torch.bfloat16, DEV)
    kb, vb, kw = p["k_buffer"], p["v_buffer"], {}
    if kv == "fp8":
        kb = kb.to(torch.float8_e5m2).view(torch.uint8)
        vb = vb.to(torch.float8_e5m2).view(torch.uint8)
        kw = dict(k_scale=1.0, v_scale=1.0)
    slots = nat.decode_plan_slots(bs, max_len, chunk, kv_tokens=int(lens.sum()))
    ws = torch.empty(nat.decode_workspace_bytes(bs, Hq, D, max_len, chunk, slots), dtype=torch.uint8, device=DEV)
    plan = torch.empty(nat.decode_plan_bytes(bs, max_len, chunk, slots) // 4, dtype=torch.int32, device=DEV)
    nat.decode_plan(plan, p["seq_lens"], max_len, chunk, slots)
    assert int(plan[3]) == int(lens.sum())
    outs = {}
    try:
        for name, mb in (("default", -2), ("always", 0), ("never", -1), ("1 MB", 1)):
            nat.debug_set("decode_nt_min_mb", mb)
            o = torch.zeros_like(p["q"])
            nat.decode_attention(o, p["q"], kb, vb, p["req_to_token"], p["req_pool_indices"], p["seq_lens"], 0.1, 0.0,
                                 max_len, chunk, ws, None, plan, max_slots=slots, **kw)
            outs[name] = o
    finally:
        nat.debug_set("decode_nt_min_mb", -2)
    assert torch.isfinite(outs["always"].float()).all()
    for name in ("always", "never", "1 MB"):
        assert torch.equal(outs[name], outs["default"]), name
    if kv == "same":
        check_decode(outs["always"], p, 0.1, torch.bfloat16, "streaming gathers")
    # a plan built with a smaller max_seq_len than the device-side lengths counts the CLAMPED keys
    nat.decode_plan(plan, p["seq_lens"], 100, chunk, slots)
    assert int(plan[3]) == int(lens.clamp(max=100).sum())


def range_plan_on_host(lens, max_len, ranges):
    """the range section of a decode plan (include/scratchpad_hip.h, ABI 8) recomputed in Python"""
    cost = 16
    lens = [min(int(l), max_len) if l > 0 else 0 for l in lens]
    pos = [0]
    for l in lens:
        pos.append(pos[-1] + (l + cost if l > 0 else 0))
    T = pos[-1]
    R = max(64, (T + ranges - 1) // ranges)
    rcount = (T + R - 1) // R if T > 0 else 0
    start = []
    for j in range(ranges):
        first = -1
        if j < rcount:
            for b, l in enumerate(lens):
                if l > 0 and pos[b] + l > j * R:              # the first request with a key at or after the cut
                    first = b if pos[b] < (j + 1) * R else -1
                    break
        start.append(first)
    return rcount, R, pos, start


@pytest.mark.parametrize("ranges", [1, 7, 384, 1000])
@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
def test_decode_range_plan_equals_a_host_recount(nat, ranges, idx_dtype):
    """sp_decode_plan(ranges > 0): positions, piece length, piece count and every piece's first request against a
    host-side recount - 700 requests (the scan crosses 256-request tiles) with empty and one-key rows, runs of empty
    rows, a length above max_seq_len (clamped), a negative length (empty); the item section in front is unchanged."""
    g = torch.Generator().manual_seed(ranges)
    bs, chunk, max_len = 700, 128, 900
    lens = torch.randint(0, 901, (bs,), generator=g)
    lens[torch.randint(0, bs, (70,), generator=g)] = 0
    lens[torch.randint(0, bs, (70,), generator=g)] = 1
    lens[100:140] = 0
    lens[0], lens[5], lens[6], lens[bs - 1] = 900, 5000, -3, 0
    seq = lens.to(idx_dtype).to(DEV)
    slots = nat.decode_plan_slots(bs, max_len, chunk, kv_tokens=int(lens.clamp(0, max_len).sum()))
    words = nat.decode_plan_bytes(bs, max_len, chunk, slots, ranges) // 4
    assert words == 4 + bs + 2 * slots + 4 + bs + 1 + ranges
    plan = torch.full((words,), -7, dtype=torch.int32, device=DEV)
    nat.decode_plan(plan, seq, max_len, chunk, slots, ranges)
    items_only = torch.full((nat.decode_plan_bytes(bs, max_len, chunk, slots) // 4,), -7, dtype=torch.int32, device=DEV)
    nat.decode_plan(items_only, seq, max_len, chunk, slots)
    host = plan.cpu()
    assert torch.equal(host[:items_only.numel()], items_only.cpu())
    rp = host[items_only.numel():].tolist()
    rcount, R, pos, start = range_plan_on_host(lens.tolist(), max_len, ranges)
    assert rp[:4] == [rcount, R, ranges, bs], "words 2, 3 (ABI 9): what the section was built for"
    assert rp[4:4 + bs + 1] == pos
    assert rp[4 + bs + 1:] == start
    assert rcount <= ranges and (rcount - 1) * R < pos[-1] <= rcount * R
    # ABI 9: max_slots = 0 builds the range section alone, behind the item header [0, chunk, 0, 0]
    words = nat.decode_plan_bytes(bs, max_len, chunk, 0, ranges) // 4
    assert words == 4 + 4 + bs + 1 + ranges
    alone = torch.full((words,), -7, dtype=torch.int32, device=DEV)
    nat.decode_plan(alone, seq, max_len, chunk, 0, ranges)
    assert alone.cpu().tolist() == [0, chunk, 0, 0] + rp


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("Hq,Hkv,D", [(32, 8, 128), (64, 8, 128), (64, 4, 128), (8, 8, 128), (16, 4, 64), (24, 4, 64),
                                      (8, 1, 128), (10, 2, 128), (18, 6, 64)])
def test_decode_range_geometry(nat, dt, Hq, Hkv, D):
    """The range kernel (decode_mfma.hip, round 5: one wave per (piece of the step's keys, kv head); a request cut by a
    piece boundary leaves partials in slots request + piece, parked in LDS until the piece is done) against the oracle,
    for 1, 3, 40 and 1000 pieces and the count sp_decode_ranges() asks for: requests of 1400 and 1025 keys cut many
    times, pieces holding dozens of short requests, one-key and empty rows, groups of 1 to 16 (four to one partials
    parked per wave), kv heads in fours (a workgroup = the four heads of one piece) and not (its waves walk different
    pieces; 1 x 10 waves leave the last workgroup half empty).  Per piece count the bits are the same on int32
    and int64 index tensors, launch after launch on one plan, over a workspace full of stale partials; behind a kv_start
    window.  sp_debug_set("decode_ranges", 0) sends the same call to the plan's (request, split) items: the bits of a
    plan without ranges."""
    dtype = DTYPES[dt]
    g = torch.Generator().manual_seed(Hq * 17 + Hkv + D)
    bs, chunk, max_len = 48, 64, 1400
    lens = torch.randint(1, 600, (bs,), generator=g)
    lens[:8] = torch.tensor([1400, 1025, 64, 65, 1, 0, 0, 1])
    lens[20:32] = torch.randint(1, 9, (12,), generator=g)     # a run of tiny requests: one piece walks many of them
    start = torch.randint(0, 4, (bs,), generator=g)
    p = paged_problem(700 + Hq + D, bs, Hq, Hkv, D, [int(l) + 4 for l in lens], dtype, DEV)
    q, req = p["q"], p["req_pool_indices"]
    seq = lens.to(DEV)
    auto = nat.decode_ranges(Hq, Hkv, D, dtype)
    assert auto > 0 and auto * Hkv >= 4 * 256, "the range kernel takes these shapes: at least a workgroup per CU"
    slots = nat.decode_plan_slots(bs, max_len, chunk, kv_tokens=int(lens.sum()))
    c = cpu(p)
    fn = lambda v: ops.decode_attention(c["q"].float(), c["k_buffer"].float(), v, c["req_to_token"],
                                        c["req_pool_indices"], lens, D ** -0.5, 0.0, start)
    live = [r for r in range(bs) if int(lens[r]) > 0]

    def launch(ranges, idx_dtype, fill):
        s_, r_, k0 = seq.to(idx_dtype), req.to(idx_dtype), start.to(DEV).to(idx_dtype)
        ws = torch.empty(nat.decode_workspace_bytes(bs, Hq, D, max_len, chunk, slots, ranges), dtype=torch.uint8, device=DEV)
        ws.fill_(fill)
        plan = torch.empty(nat.decode_plan_bytes(bs, max_len, chunk, slots, ranges) // 4, dtype=torch.int32, device=DEV)
        nat.decode_plan(plan, s_, max_len, chunk, slots, ranges)
        outs = []
        for rep in range(2):
            o = torch.zeros_like(q)
            nat.decode_attention(o, q, p["k_buffer"], p["v_buffer"], p["req_to_token"], r_, s_, D ** -0.5, 0.0,
                                 max_len, chunk, ws, k0, plan, max_slots=slots, ranges=ranges)
            outs.append(o)
        assert torch.equal(outs[0], outs[1]), (ranges, idx_dtype)
        return outs[0]

    items = launch(0, torch.int32, 0x7f)
    for ranges in (1, 3, 40, auto, 1000):
        o = launch(ranges, torch.int32, 0x7f)
        assert torch.isfinite(o.float()).all(), ranges
        assert torch.equal(o, launch(ranges, torch.int64, 0xff)), ranges
        assert float(o[5].float().abs().max()) == 0.0 and float(o[6].float().abs().max()) == 0.0, "empty rows stay untouched"
        check_vs_oracle(o, dtype, f"range decode {dt} Hq{Hq} Hkv{Hkv} D{D} ranges {ranges}", c["v_buffer"].float(), fn, rows=live)
    try:
        nat.debug_set("decode_ranges", 0)
        assert torch.equal(launch(auto, torch.int32, 0x7f), items)
    finally:
        nat.debug_set("decode_ranges", -1)


@pytest.mark.parametrize("seed", range(6))
def test_decode_range_geometry_fuzz(nat, seed):
    """Randomised steps through the range kernel against the oracle: batch sizes 1 .. 300, head shapes with the kv heads in
    fours and not, both head sizes and 16-bit dtypes, length mixes (uniform - cuts exactly between requests, ragged, mostly
    tiny, a few very long, many empty), piece counts from 1 to several times the batch size (pieces with no key at all,
    pieces of the minimum length, one piece for everything), int32 / int64 index tensors, a kv_start window; and the plan's
    range section against the host recount on every draw."""
    g = torch.Generator().manual_seed(4000 + seed)
    r = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))
    Hq, Hkv, D = [(32, 8, 128), (8, 1, 128), (16, 4, 64), (12, 2, 128), (64, 8, 128), (6, 3, 64)][seed]
    dtype = (torch.bfloat16, torch.float16)[seed % 2]
    for draw in range(4):
        bs = [r(1, 6), r(20, 60), r(100, 300), r(8, 40)][draw]
        kind = (seed + draw) % 5
        if kind == 0:
            lens = torch.full((bs,), r(1, 400))
        elif kind == 1:
            lens = torch.randint(1, 700, (bs,), generator=g)
        elif kind == 2:
            lens = torch.randint(1, 6, (bs,), generator=g)
            lens[r(0, bs - 1)] = r(300, 900)
        elif kind == 3:
            lens = torch.randint(0, 3, (bs,), generator=g) * torch.randint(1, 200, (bs,), generator=g)
            lens[r(0, bs - 1)] = r(1, 50)
        else:
            lens = torch.randint(1, 80, (bs,), generator=g)
            lens[: max(1, bs // 8)] = torch.randint(500, 1500, (max(1, bs // 8),), generator=g)
        max_len, chunk = int(lens.max()), 64
        ranges = [1, r(2, 9), r(10, 3 * bs + 10), nat.decode_ranges(Hq, Hkv, D, dtype)][(seed + draw) % 4]
        start = torch.randint(0, 3, (bs,), generator=g)
        p = paged_problem(5000 + 10 * seed + draw, bs, Hq, Hkv, D, [int(l) + 3 for l in lens], dtype, DEV)
        idt = (torch.int32, torch.int64)[draw % 2]
        seq, req, k0 = lens.to(idt).to(DEV), p["req_pool_indices"].to(idt), start.to(idt).to(DEV)
        slots = nat.decode_plan_slots(bs, max_len, chunk, kv_tokens=int(lens.sum()))
        ws = torch.empty(nat.decode_workspace_bytes(bs, Hq, D, max_len, chunk, slots, ranges), dtype=torch.uint8, device=DEV)
        ws.fill_(0x7f)
        plan = torch.empty(nat.decode_plan_bytes(bs, max_len, chunk, slots, ranges) // 4, dtype=torch.int32, device=DEV)
        nat.decode_plan(plan, seq, max_len, chunk, slots, ranges)
        rcount, R, pos, first = range_plan_on_host(lens.tolist(), max_len, ranges)
        rp = plan.cpu()[4 + bs + 2 * slots:].tolist()
        what = f"fuzz seed {seed} draw {draw}: bs {bs} Hq{Hq} Hkv{Hkv} D{D} kind {kind} ranges {ranges} R {R} pieces {rcount}"
        assert rp[:2] == [rcount, R] and rp[4:4 + bs + 1] == pos and rp[4 + bs + 1:] == first, what
        o = torch.zeros_like(p["q"])
        nat.decode_attention(o, p["q"], p["k_buffer"], p["v_buffer"], p["req_to_token"], req, seq, D ** -0.5, 0.0,
                             max_len, chunk, ws, k0, plan, max_slots=slots, ranges=ranges)
        assert torch.isfinite(o.float()).all(), what
        c = cpu(p)
        fn = lambda v: ops.decode_attention(c["q"].float(), c["k_buffer"].float(), v, c["req_to_token"],
                                            c["req_pool_indices"], lens, D ** -0.5, 0.0, start)
        live = [i for i in range(bs) if int(lens[i]) > 0]
        dead = [i for i in range(bs) if int(lens[i]) == 0]
        check_vs_oracle(o, dtype, what, c["v_buffer"].float(), fn, rows=live)
        if dead:
            assert float(o[dead].float().abs().max()) == 0.0, what + ": empty rows stay untouched"


def test_decode_ranges_where_the_range_kernel_does_not_apply(nat):
    """sp_decode_ranges() is 0 for fp32, groups wider than 16 and head sizes other than 64 / 128; an fp32 launch - or one
    with a logit soft-cap - that is handed a plan with ranges uses the plan's (request, split) items: the bits of a plan
    without."""
    # (two workgroups per CU on a 16-bit pool, three on a byte pool - a tile in flight is half the bytes there)
    assert 2 * nat.decode_ranges(32, 8, 128, torch.bfloat16, torch.uint8) == 3 * nat.decode_ranges(32, 8, 128, torch.bfloat16) > 0
    assert nat.decode_ranges(32, 8, 128, torch.float32) == 0
    assert nat.decode_ranges(32, 1, 128, torch.bfloat16) == 0 and nat.decode_ranges(32, 8, 256, torch.bfloat16) == 0
    # a wave per (piece, kv head): the fewer heads, the more pieces
    assert nat.decode_ranges(32, 8, 128, torch.bfloat16) == 2 * nat.decode_ranges(64, 16, 128, torch.bfloat16)
    assert nat.decode_ranges(16, 2, 128, torch.bfloat16) == 4 * nat.decode_ranges(32, 8, 128, torch.bfloat16)
    assert nat.decode_ranges(8, 1, 128, torch.bfloat16) == 1024          # (capped: a single head's pieces are short already)
    bs, chunk, max_len = 24, 64, 700
    g = torch.Generator().manual_seed(3)
    lens = torch.randint(1, 700, (bs,), generator=g)
    for Hq, Hkv, cap, dtype in ((8, 2, 0.0, torch.float32), (32, 8, 30.0, torch.bfloat16)):
        p = paged_problem(900 + Hq, bs, Hq, Hkv, 128, lens.tolist(), dtype, DEV)
        slots = nat.decode_plan_slots(bs, max_len, chunk, kv_tokens=int(lens.sum()))
        outs = []
        for ranges in (0, 96):
            ws = torch.empty(nat.decode_workspace_bytes(bs, Hq, 128, max_len, chunk, slots, ranges), dtype=torch.uint8, device=DEV)
            plan = torch.empty(nat.decode_plan_bytes(bs, max_len, chunk, slots, ranges) // 4, dtype=torch.int32, device=DEV)
            nat.decode_plan(plan, p["seq_lens"], max_len, chunk, slots, ranges)
            o = torch.zeros_like(p["q"])
            nat.decode_attention(o, p["q"], p["k_buffer"], p["v_buffer"], p["req_to_token"], p["req_pool_indices"],
                                 p["seq_lens"], 0.09, cap, max_len, chunk, ws, None, plan, max_slots=slots, ranges=ranges)
            outs.append(o)
        assert torch.isfinite(outs[0].float()).all() and torch.equal(outs[0], outs[1]), (Hq, Hkv, cap)
        check_decode(outs[1], p, 0.09, dtype, f"items behind a range plan Hq{Hq} Hkv{Hkv} cap{cap}", cap=cap)


def test_a_launch_must_be_given_what_its_plan_was_built_with(nat):
    """VERDICT r5 next 3 / ADVICE r5: a range plan says what it was built for and the launch checks it.
    (a) the wrapper: a plan built with 40 pieces launched with 20 (or with another max_slots, or another batch size)
        raises RuntimeError on the host - before round 6 the launch silently skipped the tail pieces;
    (b) the C ABI underneath, called with the mismatch directly: the range section's words 2, 3 differ from the launch's,
        the range kernel and its merge do NOTHING (`out` keeps its NaN fill, no fault), and a plan buffer shorter than
        (batch size, max_slots, ranges) describe is refused with SP_ERR_WORKSPACE before any launch;
    (c) the matching launch on the same buffers is right."""
    import ctypes
    bs, Hq, Hkv, D, chunk, max_len = 32, 32, 8, 128, 64, 900
    g = torch.Generator().manual_seed(77)
    lens = torch.randint(1, 900, (bs,), generator=g)
    p = paged_problem(771, bs, Hq, Hkv, D, lens.tolist(), torch.bfloat16, DEV)
    slots = nat.decode_plan_slots(bs, max_len, chunk, kv_tokens=int(lens.sum()))
    ws = torch.empty(nat.decode_workspace_bytes(bs, Hq, D, max_len, chunk, slots, 40), dtype=torch.uint8, device=DEV)
    plan = torch.empty(nat.decode_plan_bytes(bs, max_len, chunk, slots, 40) // 4, dtype=torch.int32, device=DEV)
    nat.decode_plan(plan, p["seq_lens"], max_len, chunk, slots, 40)

    def launch(ranges, max_slots=slots, rows=bs):
        o = torch.full_like(p["q"], float("nan"))
        nat.decode_attention(o[:rows], p["q"][:rows], p["k_buffer"], p["v_buffer"], p["req_to_token"],
                             p["req_pool_indices"][:rows], p["seq_lens"][:rows], 0.09, 0.0, max_len, chunk, ws, None, plan,
                             max_slots=max_slots, ranges=ranges)
        return o

    for kw in (dict(ranges=20), dict(ranges=0), dict(ranges=40, max_slots=slots - 1), dict(ranges=40, rows=bs - 1)):
        with pytest.raises(RuntimeError, match="plan was built for"):
            launch(**kw)
    good = launch(40)
    assert nat.debug_get("decode_last_kernel") == RANGE_KERNEL
    check_decode(good, p, 0.09, torch.bfloat16, "matching launch")

    # (b) the same mismatch at the C ABI (the wrapper's host-side memory of the plan is not in the way here)
    lib = nat.load()
    st = torch.cuda.current_stream().cuda_stream
    kb, vb, q = p["k_buffer"], p["v_buffer"], p["q"]

    def raw(ranges, plan_bytes, out):
        return lib.sp_decode_attention(
            out.data_ptr(), q.data_ptr(), kb.data_ptr(), vb.data_ptr(), p["req_to_token"].data_ptr(),
            p["req_to_token"].stride(0), p["req_pool_indices"].data_ptr(), p["seq_lens"].data_ptr(), None, 1, bs, Hq, Hkv,
            D, q.stride(0), out.stride(0), kb.stride(0), 0.09, 0.0, 1.0, 1.0, max_len, chunk, slots, ranges,
            ws.data_ptr(), ws.numel(), plan.data_ptr(), plan_bytes, nat.SP_BF16, nat.SP_BF16, st)

    o = torch.full_like(q, float("nan"))
    assert raw(20, plan.numel() * 4, o) == 0, "the launch itself is well-formed"
    torch.cuda.synchronize()
    assert torch.isnan(o.float()).all(), "a range launch on a plan built for another piece count must not compute anything"
    assert raw(40, plan.numel() * 4 - 4, o) == nat.SP_ERR_WORKSPACE, "plan buffer shorter than its sections"
    o = torch.full_like(q, float("nan"))
    assert raw(40, plan.numel() * 4, o) == 0
    torch.cuda.synchronize()
    assert torch.equal(o, good)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("Hq,Hkv,D", [(8, 1, 128), (16, 2, 128), (16, 1, 128), (32, 8, 128), (4, 4, 128), (24, 4, 64),
                                      (6, 2, 64)])
def test_decode_merge_of_many_splits(nat, dt, Hq, Hkv, D):
    """The merge launch on requests of 41 and 17 splits (its online groups of 16), of one and of two splits, in a ragged
    batch, on a workspace full of another launch's partials: the planned launch gives the bits of the static
    (request, split) grid, launch after launch on one plan, and both kernel forms (a wave per kv head where Hkv % 4 == 0,
    else four waves sharing a head) agree with the oracle."""
    dtype = DTYPES[dt]
    g = torch.Generator().manual_seed(Hq * 131 + Hkv)
    bs, chunk, max_len = 96, 64, 2600
    lens = torch.randint(1, 700, (bs,), generator=g)
    lens[:4] = torch.tensor([2600, 1025, 64, 65])          # 41 and 17 splits; one split; two
    p = paged_problem(300 + Hq, bs, Hq, Hkv, D, lens.tolist(), dtype, DEV)
    q, seq, req = p["q"], p["seq_lens"], p["req_pool_indices"]
    slots = nat.decode_plan_slots(bs, max_len, chunk, kv_tokens=int(lens.sum()))
    ws = torch.empty(nat.decode_workspace_bytes(bs, Hq, D, max_len, chunk, slots), dtype=torch.uint8, device=DEV)
    plan = torch.empty(nat.decode_plan_bytes(bs, max_len, chunk, slots) // 4, dtype=torch.int32, device=DEV)
    nat.decode_plan(plan, seq, max_len, chunk, slots)
    outs = []
    for rep in range(3):
        ws.fill_(0x7f if rep % 2 else 0)
        o = torch.full_like(q, float("nan"))
        nat.decode_attention(o, q, p["k_buffer"], p["v_buffer"], p["req_to_token"], req, seq, D ** -0.5, 0.0,
                             max_len, chunk, ws, None, plan, max_slots=slots)
        outs.append(o)
    base = run_decode(nat, p, D ** -0.5, chunk=chunk, max_len=max_len, use_plan=False)
    assert torch.isfinite(base.float()).all()
    for rep, o in enumerate(outs):
        assert torch.equal(o, base), rep
    check_decode(base, p, D ** -0.5, dtype, f"many splits {dt} Hq{Hq} Hkv{Hkv} D{D}")


# ----------------------------------------------------------------------------------- extend, 4 waves x 64 rows
@pytest.fixture
def w64(nat):
    """sp_debug_set("extend_w64", 2): the one-wave-per-SIMD kernel wherever it applies (D = 128, 16-bit, plain attention,
    query-head group a multiple of 4); 0 = never.  "extend_w64_persist": its persistent form for launches with a plan
    (2 = wherever the kernel applies, 0 = never).  The shipped modes (1, 1) pick by launch shape."""
    def set_mode(m, persist=0):
        nat.debug_set("extend_w64", m)
        nat.debug_set("extend_w64_persist", persist)
    yield set_mode
    nat.debug_set("extend_w64", 1)
    nat.debug_set("extend_w64_persist", 1)


W64_CASES = {
    # name: (Hq, Hkv, prefix lengths, extend lengths)
    "one tile, ragged": (32, 8, [0, 0, 0, 0], [64, 1, 37, 63]),
    "diagonal on a tile edge": (8, 2, [0, 64, 128, 192], [128, 64, 192, 65]),
    "prefix off the tile grid": (32, 8, [37, 100, 513, 1], [130, 64, 257, 700]),
    "long": (8, 2, [0, 3000, 11], [2100, 70, 1500]),
    "every ring position": (4, 1, [0] * 9, [64 * k + 5 for k in range(1, 10)]),
    "group of 8, one kv head": (8, 1, [5, 250], [300, 129]),
    # enough workgroups to keep every compute unit busy for many rounds: a wait that leaves a piece in flight too long
    # (a barrier dropped from the way in did) only shows under this kind of memory load
    "many short prompts": (8, 2, [0] * 1536, [64 + (i * 37) % 90 for i in range(1536)]),
    # the persistent form's item loop: a dozen items per workgroup with one to nine tiles each, requests without new
    # tokens in between, prefixes that start the masked tiles early
    "mixed lengths, many items": (8, 2, [(i * 53) % 300 for i in range(400)], [(i * 97) % 520 if i % 11 else 0 for i in range(400)]),
    "long and short": (16, 4, [0, 0, 1000, 0, 7] + [0] * 60, [4096, 64, 200, 1300, 2500] + [65 + 3 * i for i in range(60)]),
}


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("case", list(W64_CASES))
def test_extend_w64_equals_the_eight_wave_kernel_bit_for_bit(nat, w64, dt, case):
    """Same tiles, same lane layouts, same arithmetic per element (scores, deferred maxima, exponentials, P rounded
    once, O^T accumulation order over the keys): the two kernels must agree to the last bit - and from run to run (a
    miscounted wait, a missing hazard distance or a register the compiler also uses shows up as a difference here).
    The w64 kernel sums a row's probabilities in tile order, the eight-wave kernel in register order: the sums differ
    in their last fp32 bits, the bf16 / fp16 outputs do not.  One case is allowed to differ: with a 4096-token prompt
    among short ones, ~20 outputs per million come out a few units in the last place apart (a wave of this kernel votes
    on the deferred maximum over 64 rows of one head, a wave of the other over its own rows: where the votes differ,
    P is rounded against another maximum).  The two forms of the w64 kernel share every instruction of the
    arithmetic: they agree exactly, always."""
    dtype = DTYPES[dt]
    Hq, Hkv, pre, ext = W64_CASES[case]
    p, q, ext_t, start = extend_problem(73, Hq, Hkv, 128, pre, ext, dtype)
    args = (q, p["k_buffer"], p["v_buffer"], p["req_to_token"], p["req_pool_indices"], p["seq_lens"], ext_t, start, 128 ** -0.5)
    plan = nat.extend_plan(ext_t, p["seq_lens"], int(ext_t.sum()), Hq, Hkv, True)
    w64(0)
    ref8 = run_extend(nat, *args, plan=plan)
    w64(2, 0)
    ref = run_extend(nat, *args, plan=plan)
    if not torch.equal(ref, ref8):
        # a few elements per 100,000, a few units in the last place of outputs that are small sums of large terms
        a_, b_ = ref.float(), ref8.float()
        off = a_ != b_
        assert case == "long and short" and float(off.float().mean()) < 1e-4 and float((a_ - b_).abs().max()) < 2e-3, \
            f"{case} {dt}: max |diff| {float((a_ - b_).abs().max()):.3e} on {int(off.sum())} elements"
    for persist in (0, 2):     # one workgroup per item / persistent workgroups drawing items by ticket
        w64(2, persist)
        for _ in range(3):
            got = run_extend(nat, *args, plan=plan)
            assert torch.equal(got, ref), f"{case} {dt} persist={persist}: max |diff| {float((got.float() - ref.float()).abs().max()):.3e}"
    assert torch.equal(run_extend(nat, *args), ref), "without a plan (grid over every possible row block)"
    # ... and with 32-bit request indices / sequence lengths (the kernels read them through one switch)
    if dt == "bf16":
        a32 = list(args)
        a32[4], a32[5] = args[4].to(torch.int32), args[5].to(torch.int32)
        plan32 = nat.extend_plan(ext_t, a32[5], int(ext_t.sum()), Hq, Hkv, True)
        assert torch.equal(run_extend(nat, *a32, plan=plan32), ref)
    # the persistent form's counters behind the plan's items are zero again: the next launch starts from ticket 0
    assert int(plan[-512:].abs().sum()) == 0
    # a plan of another step (same sizes, header differs): its items are walked, its counters left alone
    stale = plan.clone()
    stale[4] += 1
    stale[-512:] = 7
    assert torch.equal(run_extend(nat, *args, plan=stale), ref) and int((stale[-512:] != 7).sum()) == 0


def test_extend_w64_against_the_oracle_and_non_causal(nat, w64):
    """The error bound of the attention tests, and cross-attention rows (non-causal over a kv_start window): the masked
    form of the body then only cuts the ragged last tile."""
    dtype = torch.bfloat16
    Hq, Hkv, D = 32, 8, 128
    pre, ext = [0, 129, 700], [200, 64, 1031]
    p, q, ext_t, start = extend_problem(77, Hq, Hkv, D, pre, ext, dtype)
    c = cpu(p)
    w64(2)
    o = run_extend(nat, q, p["k_buffer"], p["v_buffer"], p["req_to_token"], p["req_pool_indices"], p["seq_lens"], ext_t, start,
                   D ** -0.5)
    a_ = (q.cpu().float(), c["k_buffer"].float())
    b_ = (c["req_to_token"], c["req_pool_indices"], c["seq_lens"], ext_t.cpu(), start.cpu(), D ** -0.5)
    assert_attn_close(o, ops.extend_attention(*a_, c["v_buffer"].float(), *b_),
                      ops.extend_attention(*a_, c["v_buffer"].float().abs(), *b_), dtype, what="w64 ragged extend")
    # non-causal: every new row sees keys [kv_start, kv_start + seq_len) of its request's row
    enc = torch.tensor([70, 1, 333], dtype=torch.int64, device=DEV)
    kv_start = torch.tensor([3, 0, 64], dtype=torch.int64, device=DEV)
    w64(0)
    ref = run_extend(nat, q, p["k_buffer"], p["v_buffer"], p["req_to_token"], p["req_pool_indices"], enc, ext_t, start, D ** -0.5,
                     causal=False, kv_start=kv_start)
    w64(2)
    got = run_extend(nat, q, p["k_buffer"], p["v_buffer"], p["req_to_token"], p["req_pool_indices"], enc, ext_t, start, D ** -0.5,
                     causal=False, kv_start=kv_start)
    assert torch.equal(got, ref)
    # ... through the persistent form, with a request that has no encoder tokens at all (rows of zeros, no tile)
    enc0 = torch.tensor([70, 0, 333], dtype=torch.int64, device=DEV)
    plan = nat.extend_plan(ext_t, enc0, int(ext_t.sum()), Hq, Hkv, False)
    w64(0)
    ref = run_extend(nat, q, p["k_buffer"], p["v_buffer"], p["req_to_token"], p["req_pool_indices"], enc0, ext_t, start, D ** -0.5,
                     causal=False, kv_start=kv_start, plan=plan)
    w64(2, 2)
    for _ in range(2):
        got = run_extend(nat, q, p["k_buffer"], p["v_buffer"], p["req_to_token"], p["req_pool_indices"], enc0, ext_t, start,
                         D ** -0.5, causal=False, kv_start=kv_start, plan=plan)
        assert torch.equal(got, ref)


def test_extend_w64_persistent_form_replays_in_a_graph(nat, w64):
    """Captured once, replayed: every replay starts from ticket 0 (the last workgroup of a launch zeroes the counters behind
    the plan's items - no memset node, nothing on the host), and the same plan then serves an eager launch."""
    dtype = torch.bfloat16
    Hq, Hkv = 8, 2
    pre = [(i * 31) % 200 for i in range(300)]
    ext = [64 + (i * 41) % 200 for i in range(300)]
    p, q, ext_t, start = extend_problem(83, Hq, Hkv, 128, pre, ext, dtype)
    plan = nat.extend_plan(ext_t, p["seq_lens"], int(ext_t.sum()), Hq, Hkv, True)
    ws = torch.empty(nat.extend_workspace_bytes(q.shape[0], len(ext), Hq, 128, dtype), dtype=torch.uint8, device=DEV)
    args = (q, p["k_buffer"], p["v_buffer"], p["req_to_token"], p["req_pool_indices"], p["seq_lens"], ext_t, start, 128 ** -0.5,
            0.0, True, max(ext), int(p["seq_lens"].max()), ws)
    w64(2, 0)
    ref = torch.full_like(q, float("nan"))
    nat.extend_attention(ref, *args, plan=plan)
    w64(2, 2)
    out = torch.full_like(q, float("nan"))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        nat.extend_attention(out, *args, plan=plan)          # warm (kernel attributes are set outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        nat.extend_attention(out, *args, plan=plan)
    for _ in range(3):
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ref)
        assert int(plan[-512:].abs().sum()) == 0
    out.fill_(float("nan"))
    nat.extend_attention(out, *args, plan=plan)
    assert torch.equal(out, ref)


def test_extend_w64_is_selected_for_long_prompts_only(nat, w64):
    """mode 1 (shipped): long prompts or a long cached prefix take the w64 kernel, short ones the eight-wave kernel -
    observable through the foreign-plan path: both give the same bits, so the selection is checked by timing order
    only in tools/ab_extend.py; here: mode 1 runs and agrees with both."""
    dtype = torch.bfloat16
    for pre, ext in (([0, 0], [100, 90]), ([0, 0], [1500, 1200]), ([2000, 1500], [64, 64])):
        p, q, ext_t, start = extend_problem(79, 8, 2, 128, pre, ext, dtype)
        args = (q, p["k_buffer"], p["v_buffer"], p["req_to_token"], p["req_pool_indices"], p["seq_lens"], ext_t, start, 128 ** -0.5)
        plan = nat.extend_plan(ext_t, p["seq_lens"], int(ext_t.sum()), 8, 2, True)
        w64(0)
        ref = run_extend(nat, *args)
        w64(1, 1)
        assert torch.equal(run_extend(nat, *args), ref) and torch.equal(run_extend(nat, *args, plan=plan), ref)
