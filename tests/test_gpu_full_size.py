"""BASELINE.json's configurations at their FULL sizes, through size-independent properties plus spot
rows against the oracle (the oracle itself cannot run these sizes in test time):

  config 2  Llama-3-8B head shape, bs = 256 decode, contexts U[128, 4096], random slot permutation
  config 3  Llama-3-8B head shape, bs = 64 ragged prefill, prompt lengths U[128, 4096]
  config 4  Llama-3-70B at TP = 8, one rank's head shape (Hq 8 / Hkv 1), bs = 128 decode, contexts U[128, 4096]
  config 5  Mllama-11B text heads (Hq 32 / Hkv 8 / D 128), encoder_len 6404 (4 tiles x 1601 vision positions):
            bs = 32 decode (the cross launch over the encoder slots and the self launch behind them) and the
            image-token prefill (64 text rows x 6404 encoder keys per request, non-causal)

The decode cases run the form that SHIPS: split plan + separate merge launch, K/V as the two strided views of one
interleaved [P+1, 2, Hkv, D] arena, non-temporal gathers at the library's default.

16-bit outputs are held to the error model of helpers.attn_error_units (units of u * (|ref| + A))."""
import pytest
import torch

from oracle import ops
from tests.helpers import DTYPES, UNIT_ROUNDOFF, assert_attn_close, attn_error_units

pytestmark = pytest.mark.gpu
DEV = "cuda"
HQ, HKV, D = 32, 8, 128
SCALE = D ** -0.5


@pytest.fixture(scope="module")
def nat():
    from scratchpad_amd import _native
    _native.load()
    return _native


def big_pool(seed, lens, dtype, extra=64, hkv=HKV):
    """K/V pools and a fragmented req_to_token for the given context lengths, generated on the GPU.  The pool is
    what MHATokenToKVPool._create_buffers makes for one layer by default: ONE arena [P+1, 2, Hkv, D] (a token's K row
    and V row adjacent) whose two strided views are the K and the V buffer the kernels are handed."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    gc = torch.Generator().manual_seed(seed)
    total = sum(lens)
    P = total + extra
    arena = torch.empty(P + 1, 2, hkv, D, dtype=dtype, device=DEV)
    arena[:, 0].copy_(torch.empty(P + 1, hkv, D, dtype=dtype, device=DEV).normal_(0, 1, generator=g))
    arena[:, 1].copy_(torch.empty(P + 1, hkv, D, dtype=dtype, device=DEV).normal_(0, 1, generator=g))
    kb, vb = arena[:, 0], arena[:, 1]
    assert kb.stride(0) == vb.stride(0) == 2 * hkv * D and not kb.is_contiguous()
    perm = (torch.randperm(P, generator=gc) + 1).to(torch.int32)
    bs = len(lens)
    r2t = torch.zeros(bs, max(lens) + 8, dtype=torch.int32)
    off = 0
    for b, n in enumerate(lens):
        r2t[b, :n] = perm[off:off + n]
        off += n
    return kb, vb, r2t.to(DEV)


def relocate(kb, vb, r2t, gen):
    """every row of the pool (and the table) moved to another slot, in a second interleaved arena"""
    P1, hkv = kb.shape[0], kb.shape[1]
    perm = torch.randperm(P1 - 1, generator=gen).to(DEV) + 1
    perm = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), perm])
    arena2 = torch.empty(P1, 2, hkv, D, dtype=kb.dtype, device=DEV)
    arena2[perm, 0], arena2[perm, 1] = kb, vb
    return arena2[:, 0], arena2[:, 1], perm[r2t.long()].to(torch.int32)


def oracle_rows(q_rows, kb, vb, r2t, req_rows, seq_rows, abs_v=False, kv_start=None):
    """fp32 oracle for single query rows: row i attends to the seq_rows[i] keys of request req_rows[i] that start at
    position kv_start[i] (default 0) of its row of the table.  kb / vb may be CPU fp32 copies already (none is made)."""
    v = vb.float().cpu()
    return ops.decode_attention(q_rows.float().cpu(), kb.float().cpu(), v.abs() if abs_v else v, r2t.cpu(),
                                torch.tensor(req_rows), torch.tensor(seq_rows), SCALE,
                                kv_start=None if kv_start is None else torch.tensor(kv_start))


def run_decode(nat, q, kb, vb, r2t, req, seq, chunk, plan=True, ranges=0, kv_start=None, ws=None):
    """A plan built once per step, the matrix-core kernel writing partials, and the separate merge launch; non-temporal
    gathers as the library defaults them.  ranges > 0: THE SHIPPED FORM where the range kernel takes the shape
    (HipAttnBackend passes sp_decode_ranges()): the plan's range geometry, one workgroup per (piece of the step's keys,
    four kv heads).  ranges = 0: the plan's (request, split) items at split size `chunk` (what the backend runs on the
    other shapes).  plan=False: the plan-less static (request, split) grid.  kv_start: the encoder-decoder window
    offset (Mllama's self-attention launch).  ws: a workspace to use (its old contents are not cleared)."""
    bs, hq = q.shape[0], q.shape[1]
    max_len = int(seq.max())
    need = nat.decode_workspace_bytes(bs, hq, D, max_len, chunk, None, ranges)
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    assert ws.numel() >= need
    o = torch.full_like(q, float("nan"))
    pl = None
    if plan:
        pl = torch.empty(nat.decode_plan_bytes(bs, max_len, chunk, None, ranges) // 4, dtype=torch.int32, device=DEV)
        nat.decode_plan(pl, seq, max_len, chunk, None, ranges)
    nat.decode_attention(o, q, kb, vb, r2t, req, seq, SCALE, 0.0, max_len, chunk, ws, kv_start, pl, ranges=ranges)
    return o


def full_size_decode_checks(nat, dt, bs, hq, hkv, rows, what):
    """contexts U[128, 4096] seed 0 (bench.py's), random slot permutation, interleaved arena; (a) spot rows against
    the fp32 oracle, (b) split invariance, (c) slot relocation bit-exact, (d) request-order invariance bit-exact"""
    dtype = DTYPES[dt]
    gen = torch.Generator().manual_seed(0)
    lens = torch.randint(128, 4097, (bs,), generator=gen).tolist()
    lens[3], lens[bs - 56] = 4096, 128
    kb, vb, r2t = big_pool(2, lens, dtype, hkv=hkv)
    q = torch.randn(bs, hq, D, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)).to(dtype)
    req = torch.arange(bs, device=DEV)
    seq = torch.tensor(lens, device=DEV)
    o512 = run_decode(nat, q, kb, vb, r2t, req, seq, 512)
    assert torch.isfinite(o512.float()).all()
    # (a) spot rows against the fp32 oracle, error model without a max-scaled allowance
    ref = oracle_rows(q[rows], kb, vb, r2t, rows, [lens[i] for i in rows])
    aref = oracle_rows(q[rows], kb, vb, r2t, rows, [lens[i] for i in rows], abs_v=True)
    assert_attn_close(o512[rows], ref, aref, dtype, what=f"{what} {dt}: {len(rows)} rows vs oracle")
    # (b) split invariance at full size: the split size changes the partial sums, not the softmax; each
    # result is within the model of the oracle rows, and the two roundings differ by at most 2 units
    # (768: the split cap HipAttnBackend ships since round 4; 4096: every request in ONE split - what the backend
    # picks for near-uniform batches - so no partials and no merge at all; 256 also runs plan-less)
    u = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}[dtype]
    for chunk in (64, 256, 768, 4096):
        oc = run_decode(nat, q, kb, vb, r2t, req, seq, chunk)
        assert_attn_close(oc[rows], ref, aref, dtype, what=f"{what} {dt}: chunk {chunk} rows vs oracle")
        diff = (oc.float() - o512.float()).abs()
        assert float(diff.max()) <= 2.5 * u * float(vb.float().abs().max()), f"chunk {chunk} vs 512: {float(diff.max()):.3e}"
        if chunk == 256:
            assert torch.equal(run_decode(nat, q, kb, vb, r2t, req, seq, chunk, plan=False), oc), "plan-less grid"
    # (c) KV page indexing is bit-exact: relocate every row of the pool (and the table) - same bits
    kb2, vb2, r2t2 = relocate(kb, vb, r2t, gen)
    assert torch.equal(run_decode(nat, q, kb2, vb2, r2t2, req, seq, 512), o512)
    # (d) request-order invariance: a permuted batch gives the permuted rows, bit for bit
    order = torch.randperm(bs, generator=gen).to(DEV)
    o_perm = run_decode(nat, q[order].contiguous(), kb, vb, r2t, req[order].contiguous(), seq[order].contiguous(), 512)
    assert torch.equal(o_perm, o512[order])
    # (e) the layout is not part of the result: the same rows in two separate contiguous K / V buffers - same bits
    assert torch.equal(run_decode(nat, q, kb.contiguous(), vb.contiguous(), r2t, req, seq, 512), o512)
    # (f) the range geometry (what HipAttnBackend ships where sp_decode_ranges() > 0: both shapes), at the piece
    # count the library asks for and at two others: the oracle rows, at most 2 units from the split results, slot
    # relocation bit-exact; a permuted batch is cut at other places - another split of the same sums: 2 units
    auto = nat.decode_ranges(hq, hkv, D, dtype)
    assert auto > 0
    if auto:
        for ranges in (auto, 61, 1500):
            orr = run_decode(nat, q, kb, vb, r2t, req, seq, 512, ranges=ranges)
            assert torch.isfinite(orr.float()).all()
            assert_attn_close(orr[rows], ref, aref, dtype, what=f"{what} {dt}: {ranges} ranges, rows vs oracle")
            diff = (orr.float() - o512.float()).abs()
            assert float(diff.max()) <= 2.5 * u * float(vb.float().abs().max()), f"{ranges} ranges vs chunk 512: {float(diff.max()):.3e}"
            if ranges == auto:
                assert torch.equal(run_decode(nat, q, kb2, vb2, r2t2, req, seq, 512, ranges=ranges), orr)
                op = run_decode(nat, q[order].contiguous(), kb, vb, r2t, req[order].contiguous(), seq[order].contiguous(),
                                512, ranges=ranges)
                diff = (op.float() - orr[order].float()).abs()
                assert float(diff.max()) <= 2.5 * u * float(vb.float().abs().max()), f"permuted batch: {float(diff.max()):.3e}"


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_config2_decode_bs256_full_size(nat, dt):
    """config 2: Llama-3-8B heads, bs 256 - the HPW branch of decode_mfma_kernel (a wave per kv head)"""
    full_size_decode_checks(nat, dt, 256, HQ, HKV, [0, 3, 17, 64, 129, 200, 254, 255], "config 2 bs=256")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_config4_rank_shape_decode_bs128_full_size(nat, dt):
    """config 4's per-rank shape (Llama-3-70B at TP = 8: Hq 8 / Hkv 1, bs 128): the non-HPW branch of
    decode_mfma_kernel - the 4 waves share one head's keys and merge (m, l, O) through LDS behind two barriers"""
    full_size_decode_checks(nat, dt, 128, 8, 1, [0, 3, 17, 64, 72, 100, 126, 127], "config 4 rank shape bs=128")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_config3_extend_bs64_full_size(nat, dt):
    dtype = DTYPES[dt]
    gen = torch.Generator().manual_seed(0)
    bs = 64
    lens = torch.randint(128, 4097, (bs,), generator=gen).tolist()       # bench.py's prompt lengths (seed 0)
    lens[5], lens[40] = 4096, 128
    kb, vb, r2t = big_pool(4, lens, dtype)
    T = sum(lens)
    q = torch.randn(T, HQ, D, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5)).to(dtype)
    req = torch.arange(bs, device=DEV)
    seq = torch.tensor(lens, device=DEV)
    ext = seq.to(torch.int32)
    start = torch.zeros(bs, dtype=torch.int32, device=DEV)
    start[1:] = torch.cumsum(ext[:-1], 0)
    ws = torch.empty(nat.extend_workspace_bytes(T, bs, HQ, D, dtype), dtype=torch.uint8, device=DEV)

    def run(plan):
        o = torch.full_like(q, float("nan"))
        nat.extend_attention(o, q, kb, vb, r2t, req, seq, ext, start, SCALE, 0.0, True, max(lens), max(lens), ws,
                             plan=plan)
        return o
    plan = nat.extend_plan(ext, seq, T, HQ, HKV, True)
    o = run(plan)
    assert torch.isfinite(o.float()).all()
    assert torch.equal(run(None), o), "the work plan changes nothing"
    # the LDS-DMA ring's waits and barriers are counted by hand: a miscount is a race, and a race shows as
    # run-to-run differences at this size (17,976 workgroups x 8 kv heads, every CU busy) long before it shows
    # in a small case; the register-staged path must give the same bits
    for _ in range(12):
        assert torch.equal(run(plan), o), "LDS-DMA ring: run-to-run difference"
    try:
        nat.debug_set("extend_dma", 0)
        assert torch.equal(run(plan), o), "register-staged tiles vs LDS-DMA ring"
    finally:
        nat.debug_set("extend_dma", 1)
    starts = start.cpu().tolist()
    # (a) spot rows (first, interior, block edges, last) of several requests against the fp32 oracle
    spots = [(5, 0), (5, 63), (5, 64), (5, 2047), (5, 4095), (40, 127), (0, lens[0] - 1), (17, lens[17] // 2),
             (63, lens[63] - 1), (33, 1)]
    tok = [starts[b] + t for b, t in spots]
    ref = oracle_rows(q[tok], kb, vb, r2t, [b for b, _ in spots], [t + 1 for _, t in spots])
    aref = oracle_rows(q[tok], kb, vb, r2t, [b for b, _ in spots], [t + 1 for _, t in spots], abs_v=True)
    assert_attn_close(o[tok], ref, aref, dtype, what=f"config 3 bs=64 {dt}: {len(spots)} rows vs oracle")
    # (b) the last row of EVERY prompt is a decode step over the same keys: decode kernel vs extend kernel
    last = [starts[b] + lens[b] - 1 for b in range(bs)]
    od = torch.full_like(q[last], float("nan"))
    wsd = torch.empty(nat.decode_workspace_bytes(bs, HQ, D, max(lens), 512), dtype=torch.uint8, device=DEV)
    nat.decode_attention(od, q[last].contiguous(), kb, vb, r2t, req, seq, SCALE, 0.0, max(lens), 512, wsd)
    aall = oracle_rows(q[last], kb, vb, r2t, list(range(bs)), lens, abs_v=True)
    rall = oracle_rows(q[last], kb, vb, r2t, list(range(bs)), lens)
    assert_attn_close(o[last], rall, aall, dtype, what=f"config 3 {dt}: last rows (extend kernel) vs oracle")
    assert_attn_close(od, rall, aall, dtype, what=f"config 3 {dt}: last rows (decode kernel) vs oracle")
    # (c) chunked prefill (the server splits at 8192 new tokens, server/args.py:33-34): a prompt that is
    # cut in two - first part with no prefix, second part behind it as a cached prefix - gives the
    # unchunked rows again (another summation order: equal within the model, not bit for bit)
    for b, cut in ((5, 2048), (5, 1000), (0, 100), (17, lens[17] - 1)):
        L = lens[b]
        one = torch.tensor([b], device=DEV)
        o2 = torch.full_like(q[starts[b]:starts[b] + L], float("nan"))
        z = torch.zeros(1, dtype=torch.int32, device=DEV)
        nat.extend_attention(o2[:cut], q[starts[b]:starts[b] + cut], kb, vb, r2t, one, torch.tensor([cut], device=DEV),
                             torch.tensor([cut], dtype=torch.int32, device=DEV), z, SCALE, 0.0, True, cut, cut, ws)
        nat.extend_attention(o2[cut:], q[starts[b] + cut:starts[b] + L], kb, vb, r2t, one, torch.tensor([L], device=DEV),
                             torch.tensor([L - cut], dtype=torch.int32, device=DEV), z, SCALE, 0.0, True, L - cut, L, ws)
        whole = o[starts[b]:starts[b] + L]
        u = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}[dtype]
        diff = float((o2.float() - whole.float()).abs().max())
        assert diff <= 2.5 * u * float(vb.float().abs().max()), f"chunked at {cut}: {diff:.3e}"
        same = float((o2 == whole).float().mean())
        print(f"[parity] config 3 {dt}: request {b} cut at {cut}: {100 * same:.1f} % of the outputs bit-identical, "
              f"max |diff| {diff:.2e}")
        # rows of the first part see exactly the same keys in the same tiles: bit for bit
        assert torch.equal(o2[:cut // 64 * 64], whole[:cut // 64 * 64])


# ------------------------------------------------------------------------------------------------ config 5 (Mllama-11B)
ENC_LEN = 6404          # 4 tiles x 1601 vision positions = 100 x 64 + 4: every encoder window ends in a 4-key tail tile


def max_diff(a, b):
    return float((a.float() - b.float()).abs().max())


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_config5_cross_and_self_decode_bs32_full_size(nat, dt):
    """config 5 decode, bs 32, in the form HipAttnBackend.forward_decode ships for Mllama: one plan per kv window
    (range geometry at the library's piece count), the range kernel, the merge.  The table row of a request holds its
    6404 encoder slots and then its text slots; the CROSS launch reads [0, encoder_len) (seq_lens = encoder_lens, no
    kv_start), the SELF launch reads [encoder_len, encoder_len + text) (kv_start = encoder_lens, int64 as ScheduleBatch
    keeps them).  Per launch: (a) spot rows against the fp32 oracle, (b) the item geometry at chunk 512 and the range
    geometry at other piece counts within 2.5 u max|V|, (c) slot relocation bit-exact, (d) int32 seq_lens /
    req_pool_indices beside int64 encoder_lens bit-exact, (e) a workspace left full of another launch's partials
    bit-exact; (f) a mixed batch (encoder_len 0 / 1601 / 6404) in one launch."""
    dtype = DTYPES[dt]
    u = UNIT_ROUNDOFF[dtype]
    bs = 32
    gen = torch.Generator().manual_seed(0)
    text = torch.randint(64, 129, (bs,), generator=gen).tolist()
    text[5], text[20] = 64, 128
    enc = [ENC_LEN] * bs
    kb, vb, r2t = big_pool(6, [e + t for e, t in zip(enc, text)], dtype)
    kc, vc = kb.float().cpu(), vb.float().cpu()
    va = vc.abs()
    tol = 2.5 * u * float(va.max())
    kb2, vb2, r2t2 = relocate(kb, vb, r2t, gen)
    q = torch.randn(bs, HQ, D, device=DEV, generator=torch.Generator(device=DEV).manual_seed(7)).to(dtype)
    req = torch.arange(bs, device=DEV)
    enc_t, text_t = torch.tensor(enc, device=DEV), torch.tensor(text, device=DEV)
    auto = nat.decode_ranges(HQ, HKV, D, dtype)
    assert auto > 0
    rows = [0, 3, 5, 11, 17, 20, 26, bs - 1]           # first, last, the shortest (5) and the longest (20) text
    # one workspace big enough for every launch below (the item geometry of the cross launch at chunk 64 is the largest)
    ws = torch.empty(nat.decode_workspace_bytes(bs, HQ, D, ENC_LEN, 64, None, 1500), dtype=torch.uint8, device=DEV)

    def spot(o, lens, kv0, what, sel=rows):
        starts = None if kv0 is None else [kv0[i] for i in sel]
        ref = oracle_rows(q[sel], kc, vc, r2t, sel, [lens[i] for i in sel], kv_start=starts)
        aref = oracle_rows(q[sel], kc, va, r2t, sel, [lens[i] for i in sel], kv_start=starts)
        assert_attn_close(o[sel], ref, aref, dtype, what=f"config 5 {what} decode bs=32 {dt}")

    launches = {"cross": (enc_t, None, (text_t, enc_t)), "self": (text_t, enc_t, (enc_t, None))}
    for name, (seq, kv0, (other_seq, other_kv0)) in launches.items():
        lens, starts = seq.tolist(), None if kv0 is None else kv0.tolist()
        o = run_decode(nat, q, kb, vb, r2t, req, seq, 512, ranges=auto, kv_start=kv0)
        assert nat.debug_get("decode_last_kernel") == 3, "the range kernel ran"
        assert torch.isfinite(o.float()).all()
        # (a) spot rows against the fp32 oracle
        spot(o, lens, starts, f"{name}: {auto} ranges, {len(rows)} rows vs oracle")
        # (b) the (request, split) items at chunk 512, and the range geometry at two other piece counts
        o512 = run_decode(nat, q, kb, vb, r2t, req, seq, 512, kv_start=kv0)
        assert nat.debug_get("decode_last_kernel") != 3
        spot(o512, lens, starts, f"{name}: items at chunk 512, rows vs oracle")
        for ranges in (auto, 61, 1500):
            orr = run_decode(nat, q, kb, vb, r2t, req, seq, 512, ranges=ranges, kv_start=kv0)
            assert nat.debug_get("decode_last_kernel") == 3
            if ranges == auto:
                assert torch.equal(orr, o), "run-to-run difference"
            assert max_diff(orr, o512) <= tol, f"{name}: {ranges} ranges vs chunk 512: {max_diff(orr, o512):.3e}"
        # (c) slot relocation: the same bits
        assert torch.equal(run_decode(nat, q, kb2, vb2, r2t2, req, seq, 512, ranges=auto, kv_start=kv0), o), "relocated"
        # (d) index dtypes: int32 req_pool_indices / seq_lens (graph replay's) beside int64 encoder_lens
        i32 = torch.int32
        variants = ([(req.to(i32), seq), (req.to(i32), seq.to(i32))] if kv0 is None
                    else [(req.to(i32), seq.to(i32))])
        for r_, s_ in variants:
            got = run_decode(nat, q, kb, vb, r2t, r_, s_, 512, ranges=auto, kv_start=kv0)
            assert torch.equal(got, o), f"{name}: req {r_.dtype} / seq_lens {s_.dtype} / kv_start int64"
        # (e) a workspace full of the other launch's partials (item geometry at chunk 64, then its range launch)
        run_decode(nat, q, kb, vb, r2t, req, other_seq, 64, kv_start=other_kv0, ws=ws)
        run_decode(nat, q, kb, vb, r2t, req, other_seq, 512, ranges=auto, kv_start=other_kv0, ws=ws)
        assert torch.equal(run_decode(nat, q, kb, vb, r2t, req, seq, 512, ranges=auto, kv_start=kv0, ws=ws), o), "stale ws"

    # (f) a mixed batch: text-only requests (encoder_len 0), one-tile images (1601) and four-tile images in ONE launch.
    # The kernels leave a row without keys untouched (the backend hands cross-attention a zeroed output): it stays NaN.
    mixed = [(ENC_LEN, 0, 1601)[i % 3] for i in range(bs)]
    mixed_t = torch.tensor(mixed, device=DEV)
    full = [i for i in range(bs) if mixed[i]]
    empty = [i for i in range(bs) if not mixed[i]]
    om = run_decode(nat, q, kb, vb, r2t, req, mixed_t, 512, ranges=auto)
    assert nat.debug_get("decode_last_kernel") == 3
    assert torch.isnan(om[empty].float()).all(), "a row without encoder keys was written"
    assert torch.isfinite(om[full].float()).all(), "a neighbour of an empty row was disturbed"
    spot(om, mixed, None, f"cross, mixed encoder_len 0 / 1601 / 6404: all {len(full)} non-empty rows vs oracle", full)
    long_rows = [i for i in full if mixed[i] == ENC_LEN]
    om512 = run_decode(nat, q, kb, vb, r2t, req, enc_t, 512, ranges=auto)
    assert max_diff(om[long_rows], om512[long_rows]) <= tol, "mixed batch vs uniform batch, 6404-key rows"
    # ... and the self launch behind windows that start at 0, 1601 and 6404 (int64 kv_start, int32 lengths)
    os_ = run_decode(nat, q, kb, vb, r2t, req.to(torch.int32), text_t.to(torch.int32), 512, ranges=auto, kv_start=mixed_t)
    assert torch.isfinite(os_.float()).all()
    spot(os_, text, mixed, "self behind mixed windows 0 / 1601 / 6404", [0, 1, 2, 3, 4, 5, 20, bs - 1])


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_config5_image_prefill_full_size(nat, dt):
    """config 5's image-token prefill: four requests of 64 text rows over 6404 encoder keys each (non-causal) and one
    text-only request (encoder_len 0) in the middle of the batch, launched as HipAttnBackend.forward_extend launches the
    cross layer: seq_lens = encoder_lens, no kv_start, max_len = the longest encoder window, and the step's work plan,
    which init_forward_metadata builds from the TEXT seq_lens.  Then the self-attention prefill behind the encoder
    slots (causal, kv_start = encoder_lens) on the same data."""
    from scratchpad_amd import _native
    dtype = DTYPES[dt]
    enc = [ENC_LEN, ENC_LEN, 0, ENC_LEN, ENC_LEN]
    text = [64, 64, 40, 64, 64]
    bs, T = len(enc), sum(text)
    kb, vb, r2t = big_pool(8, [e + t for e, t in zip(enc, text)], dtype)
    kc, vc = kb.float().cpu(), vb.float().cpu()
    va = vc.abs()
    q = torch.randn(T, HQ, D, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9)).to(dtype)
    req = torch.arange(bs, device=DEV)
    enc_t, text_t = torch.tensor(enc, device=DEV), torch.tensor(text, device=DEV)
    ext = text_t.to(torch.int32)
    start = torch.zeros(bs, dtype=torch.int32, device=DEV)
    start[1:] = torch.cumsum(ext[:-1], 0)
    starts = start.cpu().tolist()
    ws = torch.empty(nat.extend_workspace_bytes(T, bs, HQ, D, dtype), dtype=torch.uint8, device=DEV)
    plan = nat.extend_plan(ext, text_t, T, HQ, HKV, True)          # the backend's: from the text lengths
    txt = slice(starts[2], starts[2] + text[2])
    rest = [t for t in range(T) if not starts[2] <= t < starts[2] + text[2]]

    def cross(plan, zero=True):
        # allocated as HipAttnBackend._alloc_out allocates a cross-attention output (zeroed, spare rows behind it)
        o = _native.empty_rows(T, HQ * D, dtype, DEV, zero=True).view(T, HQ, D)
        if not zero:
            o.fill_(float("nan"))
        nat.extend_attention(o, q, kb, vb, r2t, req, enc_t, ext, start, SCALE, 0.0, False, max(text), ENC_LEN, ws,
                             plan=plan)
        return o

    o = cross(plan)
    kernel = nat.debug_get("extend_last_kernel")
    assert kernel in (2, 3), f"a 6404-key window runs the 4-wave x 64-row kernel, not {_native.EXTEND_KERNELS[kernel]}"
    assert torch.isfinite(o.float()).all()
    assert torch.all(o[txt] == 0), "the text-only request's rows read as zeros"
    # unlike the decode kernels, the extend kernels WRITE zeros to rows without keys: a NaN-filled output gives the
    # same bits everywhere (and the rows around the text-only request are what they were)
    raw = cross(plan, zero=False)
    assert torch.equal(raw, o)
    # spot rows: first, last and an interior row of each image request against the fp32 oracle
    spots = [(b, t) for b in (0, 1, 3, 4) for t in (0, 17 + 9 * b, 63)]
    tok = [starts[b] + t for b, t in spots]
    ref = oracle_rows(q[tok], kc, vc, r2t, [b for b, _ in spots], [enc[b] for b, _ in spots])
    aref = oracle_rows(q[tok], kc, va, r2t, [b for b, _ in spots], [enc[b] for b, _ in spots])
    assert_attn_close(o[tok], ref, aref, dtype,
                      what=f"config 5 image prefill {dt} ({_native.EXTEND_KERNELS[kernel]}): {len(spots)} cross rows vs oracle")
    assert torch.equal(cross(None), o), "the work plan changes nothing"
    for _ in range(8):
        assert torch.equal(cross(plan), o), "run-to-run difference"
    try:
        for mode, kernels in ((2, (2, 3)), (0, (1,))):
            nat.debug_set("extend_w64", mode)
            got = cross(plan)
            assert nat.debug_get("extend_last_kernel") in kernels, (mode, nat.debug_get("extend_last_kernel"))
            assert torch.equal(got, o), f"extend_w64={mode}: max |diff| {max_diff(got, o):.3e}"
    finally:
        nat.debug_set("extend_w64", 1)

    # the self-attention prefill behind the encoder slots: causal over [encoder_len, encoder_len + text)
    def self_attn(plan):
        o = torch.full_like(q, float("nan"))
        nat.extend_attention(o, q, kb, vb, r2t, req, text_t, ext, start, SCALE, 0.0, True, max(text), ENC_LEN, ws,
                             enc_t, plan=plan)
        return o
    os_ = self_attn(plan)
    assert torch.isfinite(os_.float()).all()
    assert torch.equal(self_attn(None), os_)
    spots = [(b, t) for b in range(bs) for t in (0, 31, text[b] - 1)]
    tok = [starts[b] + t for b, t in spots]
    reqs, lens, kv0 = [b for b, _ in spots], [t + 1 for _, t in spots], [enc[b] for b, _ in spots]
    ref = oracle_rows(q[tok], kc, vc, r2t, reqs, lens, kv_start=kv0)
    aref = oracle_rows(q[tok], kc, va, r2t, reqs, lens, kv_start=kv0)
    assert_attn_close(os_[tok], ref, aref, dtype, what=f"config 5 self prefill behind the encoder {dt}: {len(spots)} rows vs oracle")
