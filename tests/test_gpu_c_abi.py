"""GPU parity of every compute entry point of include/scratchpad_hip.h, called the way an integrator calls it: through a
binding made from the header alone (tests/c_header.py), every parameter passed by its header name, never through the
wrappers of scratchpad_amd/_native.py.

Each call is set up so that arguments cannot stand in for one another: strides differ from their neighbours and from
the dense value, head counts and scales come in unequal pairs, padding between rows holds values that would change the
result if read (NaN in 16-bit activations, a value above any real logit or probability in the sampler's padding), and
every output lies inside a guard of a fixed bit pattern that must be unchanged, bit for bit, after the call.  Results
are held to the bar the suite already uses for each operation (oracle/ops.py, oracle/sampling.py, an fp32 matmul)."""
import math

import numpy as np
import pytest
import torch

from oracle import ops
from oracle import sampling as osamp
from tests import c_header
from tests.helpers import assert_attn_close, assert_close
from tests.test_gpu_elementwise import ulp_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = c_header.enum_values("sp_dtype")
ST = c_header.enum_values("sp_status")
OK = ST["SP_OK"]
CODE = {torch.float32: DT["SP_F32"], torch.float16: DT["SP_F16"], torch.bfloat16: DT["SP_BF16"]}
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
GUARD_BYTES = 256
PATTERN = 0xA5


@pytest.fixture(scope="module")
def lib():
    from scratchpad_amd import _native
    return c_header.bind(_native.lib_path())


def stream():
    return torch.cuda.current_stream().cuda_stream


def run(lib, name, **kw):
    rc = c_header.call(lib, name, **kw)
    assert rc == OK, f"{name} returned {rc}"
    torch.cuda.synchronize()


class Guarded:
    """`rows` x `cols` elements with `stride` elements from row to row, inside one byte buffer: GUARD_BYTES of PATTERN
    in front and behind, and `pad` (PATTERN when None) in the columns cols..stride of every row.  `t` is the strided
    view.  check() asserts that every byte outside the rows it is told were written is what it was when snapshot()
    was last called (after construction and `init`)."""

    def __init__(self, rows, cols, stride, dtype, init=None, pad=None):
        assert stride >= cols
        self.rows, self.cols, self.stride, self.dtype = rows, cols, stride, dtype
        self.es = torch.empty((), dtype=dtype).element_size()
        n = rows * stride * self.es
        self.raw = torch.full((n + 2 * GUARD_BYTES,), PATTERN, dtype=torch.uint8, device=DEV)
        self.body = self.raw[GUARD_BYTES:GUARD_BYTES + n].view(dtype).view(rows, stride)
        if pad is not None:
            self.body[:, cols:] = pad
        self.t = self.body[:, :cols]
        if init is not None:
            self.t.copy_(init.reshape(rows, cols))
        self.snapshot()

    def snapshot(self):
        self.ref = self.raw.clone()

    def view3(self, h, d):
        assert h * d == self.cols
        return self.t.view(self.rows, h, d) if self.rows else self.t.reshape(0, h, d)

    def check(self, what, written_rows="all"):
        """written_rows: "all", None (nothing may change) or a list of row indices whose first `cols` may change."""
        mask = torch.ones_like(self.raw, dtype=torch.bool)
        body = mask[GUARD_BYTES:GUARD_BYTES + self.rows * self.stride * self.es].view(self.rows, self.stride * self.es)
        if written_rows == "all":
            body[:, :self.cols * self.es] = False
        elif written_rows is not None:
            body[torch.as_tensor(written_rows, dtype=torch.long, device=DEV), :self.cols * self.es] = False
        diff = (self.raw != self.ref) & mask
        assert not bool(diff.any()), (f"{what}: {int(diff.sum())} bytes outside the output changed, first at byte "
                                      f"{int(diff.nonzero()[0])} of the guarded buffer")


def padded(x, stride, pad):
    """an input [rows, cols] copied into rows of `stride` elements whose padding holds `pad`"""
    rows, cols = x.shape
    return Guarded(rows, cols, stride, x.dtype, init=x, pad=pad)


# --------------------------------------------------------------------------- row kernels
@pytest.mark.parametrize("hidden", [136, 100])
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
def test_rmsnorm(lib, dt, hidden):
    dtype = DTYPES[dt]
    g = torch.Generator().manual_seed(hidden)
    T_ = 5
    x0 = torch.randn(T_, hidden, generator=g).to(dtype)
    w = (torch.randn(hidden, generator=g) * 0.3 + 1).to(dtype)
    x = padded(x0.to(DEV), hidden + 24, float("nan"))
    out = Guarded(T_, hidden, hidden + 40, dtype)
    wd = w.to(DEV)
    run(lib, "sp_rmsnorm", out=out.t, x=x.t, weight=wd, num_tokens=T_, hidden=hidden, x_stride=hidden + 24,
        out_stride=hidden + 40, eps=1e-5, dtype=CODE[dtype], stream=stream())
    ulp_close(out.t, ops.rmsnorm(x0, w, 1e-5), dtype, f"rmsnorm {dt} hidden {hidden}")
    out.check("rmsnorm out")
    x.check("rmsnorm x", None)


@pytest.mark.parametrize("hidden", [136, 100])
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
def test_fused_add_rmsnorm(lib, dt, hidden):
    dtype = DTYPES[dt]
    g = torch.Generator().manual_seed(hidden + 1)
    T_ = 6
    x0 = torch.randn(T_, hidden, generator=g).to(dtype)
    r0 = torch.randn(T_, hidden, generator=g).to(dtype)
    w = (torch.randn(hidden, generator=g) * 0.3 + 1).to(dtype)
    xs, rs = hidden + 24, hidden + 56
    x, r = padded(x0.to(DEV), xs, float("nan")), padded(r0.to(DEV), rs, float("nan"))
    run(lib, "sp_fused_add_rmsnorm", x=x.t, residual=r.t, weight=w.to(DEV), num_tokens=T_, hidden=hidden, x_stride=xs,
        res_stride=rs, eps=1e-6, dtype=CODE[dtype], stream=stream())
    yref, rref = ops.rmsnorm(x0, w, 1e-6, r0)
    ulp_close(x.t, yref, dtype, f"fused_add_rmsnorm x {dt} hidden {hidden}")
    assert torch.equal(r.t.cpu(), rref), "residual' = round(x + residual) must be bit-exact"
    x.check("fused_add_rmsnorm x")
    r.check("fused_add_rmsnorm residual")


@pytest.mark.parametrize("d", [72, 37])
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
def test_silu_and_mul(lib, dt, d):
    dtype = DTYPES[dt]
    g = torch.Generator().manual_seed(d)
    T_ = 4
    x0 = (torch.randn(T_, 2 * d, generator=g) * 3).to(dtype)
    x = padded(x0.to(DEV), 2 * d + 24, float("nan"))
    out = Guarded(T_, d, d + 40, dtype)
    run(lib, "sp_silu_and_mul", out=out.t, x=x.t, num_tokens=T_, d=d, x_stride=2 * d + 24, out_stride=d + 40,
        dtype=CODE[dtype], stream=stream())
    ulp_close(out.t, ops.silu_and_mul(x0), dtype, f"silu_and_mul {dt} d {d}")
    out.check("silu_and_mul out")
    x.check("silu_and_mul x", None)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("is_neox", [0, 1])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_rotary_embedding(lib, dt, is_neox, fused):
    dtype = DTYPES[dt]
    g = torch.Generator().manual_seed(7 + is_neox)
    T_, Hq, Hkv, D, rot, P = 6, 4, 2, 64, 32, 12
    qs, ks, vs, kvs = Hq * D + 24, Hkv * D + 40, Hkv * D + 56, Hkv * D + 8
    cache = ops.rope_cos_sin_cache(64, 10000.0, rot, None, dtype)
    pos = torch.randint(0, 64, (T_,), generator=g)
    q0 = torch.randn(T_, Hq * D, generator=g).to(dtype)
    k0 = torch.randn(T_, Hkv * D, generator=g).to(dtype)
    v0 = torch.randn(T_, Hkv * D, generator=g).to(dtype)
    q, k, v = padded(q0.to(DEV), qs, float("nan")), padded(k0.to(DEV), ks, float("nan")), padded(v0.to(DEV), vs, float("nan"))
    loc = torch.tensor([5, 0, 9, 2, 11, 7], dtype=torch.int64)      # non-monotone, with the dummy slot 0
    kb = Guarded(P + 1, Hkv * D, kvs, dtype, pad=float("nan"))
    vb = Guarded(P + 1, Hkv * D, kvs, dtype, pad=float("nan"))
    run(lib, "sp_rotary_embedding", positions=pos.to(DEV), q=q.t, k=k.t, cos_sin_cache=cache.to(DEV), num_tokens=T_,
        num_q_heads=Hq, num_kv_heads=Hkv, head_size=D, rotary_dim=rot, q_stride=qs, k_stride=ks, is_neox=is_neox,
        v=v.t if fused else None, v_stride=vs if fused else 0, k_buffer=kb.t if fused else None,
        v_buffer=vb.t if fused else None, out_cache_loc=loc.to(DEV) if fused else None,
        kv_buffer_stride=kvs if fused else 0, dtype=CODE[dtype], stream=stream())
    qr, kr = ops.rotary_embedding(pos, q0, k0, D, cache, bool(is_neox))
    ulp_close(q.t, qr, dtype, f"rotary q {dt} neox {is_neox}")
    ulp_close(k.t, kr, dtype, f"rotary k {dt} neox {is_neox}")
    assert torch.equal(q.t.cpu().view(T_, Hq, D)[:, :, rot:], q0.view(T_, Hq, D)[:, :, rot:]), "dims beyond rotary_dim"
    q.check("rotary q")
    k.check("rotary k")
    v.check("rotary v", None)
    if fused:
        assert torch.equal(kb.t.cpu()[loc], k.t.cpu()), "pool K rows == rotated k"
        assert torch.equal(vb.t.cpu()[loc], v0), "pool V rows == v"
        kb.check("rotary k_buffer", loc.tolist())
        vb.check("rotary v_buffer", loc.tolist())
    else:
        kb.check("rotary k_buffer", None)
        vb.check("rotary v_buffer", None)


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
def test_kv_store(lib, dt):
    dtype = DTYPES[dt]
    g = torch.Generator().manual_seed(11)
    T_, Hkv, D, Dv, P = 5, 2, 64, 32, 40          # P: room for a V row written at the K stride (a mixed-up stride stays inside the guard)
    kst, vst, kbs, vbs = Hkv * D + 24, Hkv * Dv + 40, Hkv * D + 8, Hkv * Dv + 24
    k0 = torch.randn(T_, Hkv * D, generator=g).to(dtype)
    v0 = torch.randn(T_, Hkv * Dv, generator=g).to(dtype)
    k, v = padded(k0.to(DEV), kst, float("nan")), padded(v0.to(DEV), vst, float("nan"))
    loc = torch.tensor([9, 0, 14, 3, 7], dtype=torch.int64)
    kb = Guarded(P + 1, Hkv * D, kbs, dtype, pad=float("nan"))
    vb = Guarded(P + 1, Hkv * Dv, vbs, dtype, pad=float("nan"))
    kb0, vb0 = kb.t.cpu(), vb.t.cpu()
    run(lib, "sp_kv_store", k_buffer=kb.t, v_buffer=vb.t, loc=loc.to(DEV), k=k.t, v=v.t, num_tokens=T_,
        num_kv_heads=Hkv, head_dim=D, v_head_dim=Dv, k_stride=kst, v_stride=vst, k_buffer_stride=kbs,
        v_buffer_stride=vbs, dtype=CODE[dtype], stream=stream())
    ops.kv_store(kb0.view(P + 1, Hkv, D), vb0.view(P + 1, Hkv, Dv), loc, k0.view(T_, Hkv, D), v0.view(T_, Hkv, Dv))
    assert torch.equal(kb.t.cpu()[loc], kb0[loc]), "K rows"
    assert torch.equal(vb.t.cpu()[loc], vb0[loc]), "V rows"
    kb.check("kv_store k_buffer", loc.tolist())
    vb.check("kv_store v_buffer", loc.tolist())
    k.check("kv_store k", None)
    v.check("kv_store v", None)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_kv_store_fp8(lib, dt):
    dtype = DTYPES[dt]
    g = torch.Generator().manual_seed(12)
    T_, Hkv, D, P = 5, 2, 64, 16
    kst, vst, kbs, vbs = Hkv * D + 24, Hkv * D + 40, Hkv * D + 8, Hkv * D + 16
    k_scale, v_scale = 1.7, 0.37
    k0 = (torch.randn(T_, Hkv * D, generator=g) * 3).to(dtype)
    v0 = (torch.randn(T_, Hkv * D, generator=g) * 0.3).to(dtype)
    k, v = padded(k0.to(DEV), kst, float("nan")), padded(v0.to(DEV), vst, float("nan"))
    loc = torch.tensor([9, 0, 14, 3, 7], dtype=torch.int64)
    kb = Guarded(P + 1, Hkv * D, kbs, torch.uint8, pad=0x7F)
    vb = Guarded(P + 1, Hkv * D, vbs, torch.uint8, pad=0x7F)
    run(lib, "sp_kv_store_fp8", k_buffer=kb.t, v_buffer=vb.t, loc=loc.to(DEV), k=k.t, v=v.t, num_tokens=T_,
        num_kv_heads=Hkv, head_dim=D, k_stride=kst, v_stride=vst, k_buffer_stride=kbs, v_buffer_stride=vbs,
        k_scale=k_scale, v_scale=v_scale, src_dtype=CODE[dtype], stream=stream())
    want_k = k0.clone().div_(k_scale).to(torch.float8_e5m2).view(torch.uint8)
    want_v = v0.clone().div_(v_scale).to(torch.float8_e5m2).view(torch.uint8)
    assert torch.equal(kb.t.cpu()[loc], want_k), "K rows"
    assert torch.equal(vb.t.cpu()[loc], want_v), "V rows"
    kb.check("kv_store_fp8 k_buffer", loc.tolist())
    vb.check("kv_store_fp8 v_buffer", loc.tolist())


def test_write_req_to_token(lib):
    g = torch.Generator().manual_seed(13)
    rows, width, row_stride = 7, 30, 37                 # 37: no length of the batch
    pre = torch.tensor([0, 5, 3, 12], dtype=torch.int64)
    ext = torch.tensor([4, 7, 0, 9], dtype=torch.int64)
    seq = pre + ext
    req = torch.tensor([5, 0, 2, 3], dtype=torch.int64)
    loc = torch.randperm(100, generator=g)[:int(ext.sum())] + 1
    init = torch.randint(1, 1000, (rows, width), generator=g, dtype=torch.int32)
    table = Guarded(rows, width, row_stride, torch.int32, init=init.to(DEV), pad=-7)
    ref = table.body.cpu()
    ops.write_req_to_token(ref, req, pre, seq, ext, loc)
    run(lib, "sp_write_req_to_token", req_to_token=table.t, row_stride=row_stride, req_pool_indices=req.to(DEV),
        pre_lens=pre.to(DEV), seq_lens=seq.to(DEV), extend_lens=ext.to(DEV), out_cache_loc=loc.to(DEV),
        batch_size=4, stream=stream())
    assert torch.equal(table.body.cpu(), ref)
    table.check("write_req_to_token")


def test_compute_and_clamp_position(lib):
    pre = torch.tensor([0, 7, 3, 0, 30], dtype=torch.int32)
    ext = torch.tensor([3, 1, 0, 5, 2], dtype=torch.int32)
    n = int(ext.sum())
    positions = Guarded(1, n, n, torch.int64)
    start = Guarded(1, 5, 5, torch.int32)
    run(lib, "sp_compute_position", positions=positions.t, extend_start_loc=start.t, extend_prefix_lens=pre.to(DEV),
        extend_seq_lens=ext.to(DEV), batch_size=5, stream=stream())
    rpos, rstart = ops.compute_position(pre, ext)
    assert torch.equal(positions.t.cpu()[0], rpos) and torch.equal(start.t.cpu()[0], rstart)
    positions.check("compute_position positions")
    start.check("compute_position extend_start_loc")
    seq = torch.tensor([0, 1, 17, 2 ** 31 - 1, 5])
    for idx64, idt in ((1, torch.int64), (0, torch.int32)):
        out = Guarded(1, 5, 5, torch.int64)
        run(lib, "sp_clamp_position", positions=out.t, seq_lens=seq.to(idt).to(DEV), idx64=idx64, batch_size=5,
            stream=stream())
        assert torch.equal(out.t.cpu()[0], ops.clamp_position(seq)), idx64
        out.check(f"clamp_position idx64 {idx64}")


# --------------------------------------------------------------------------- decode attention
HQ, HKV, D = 8, 2, 128                                   # Hq != Hkv: four query heads per kv head
KV_PAD = 16                                              # elements behind every pool row


def _pool(g, P, kv8, dtype):
    """K and V pools [P + 1, Hkv, D] with KV_PAD elements (bytes on a byte pool) of NaN behind every row"""
    out = []
    for _ in range(2):
        x = torch.randn(P + 1, HKV * D, generator=g)
        if kv8:
            buf = padded(x.to(torch.float8_e5m2).view(torch.uint8).to(DEV), HKV * D + KV_PAD, 0xFF)
        else:
            buf = padded(x.to(dtype).to(DEV), HKV * D + KV_PAD, float("nan"))
        out.append(buf)
    return out


def _widened(buf, kv8, scale):
    rows = buf.t.cpu()
    rows = rows.view(torch.float8_e5m2).float() if kv8 else rows.float()
    return (rows * scale).view(-1, HKV, D)


def _decode_problem(seed, lens, max_seq_len, kv_start, kv8, dtype):
    g = torch.Generator().manual_seed(seed)
    bs = len(lens)
    P = 4000
    kb, vb = _pool(g, P, kv8, dtype)
    r2t_stride = max_seq_len + 77                        # != max_seq_len; room for kv_start + every device length
    table = torch.randint(1, P + 1, (bs + 3, r2t_stride), generator=g, dtype=torch.int32)   # every entry a valid slot
    req = torch.randperm(bs + 3, generator=g)[:bs]
    qkv_stride = (HQ + 2 * HKV) * D + 8                  # q is a view of a fused qkv row
    qkv = torch.full((bs, qkv_stride), float("nan"))
    qkv[:, :HQ * D] = torch.randn(bs, HQ * D, generator=g)
    qkv = qkv.to(dtype).to(DEV)
    return dict(kb=kb, vb=vb, table=table, r2t_stride=r2t_stride, req=req, qkv=qkv, q_stride=qkv_stride,
                seq=torch.tensor(lens, dtype=torch.int64),
                kv_start=None if kv_start is None else torch.tensor(kv_start, dtype=torch.int64))


def _decode_reference(p, max_seq_len, k_scale, v_scale, kv8):
    bs = p["seq"].shape[0]
    q = p["qkv"][:, :HQ * D].float().cpu().view(bs, HQ, D)
    kw, vw = _widened(p["kb"], kv8, k_scale), _widened(p["vb"], kv8, v_scale)
    seq = p["seq"].clamp(max=max_seq_len)
    fn = lambda v: ops.decode_attention(q, kw, v, p["table"], p["req"], seq, D ** -0.5, 0.0, p["kv_start"])
    return fn, vw


def _decode_call(lib, p, out, out_stride, idx64, max_seq_len, chunk, max_slots, ranges, plan, plan_bytes, workspace,
                 workspace_bytes, k_scale, v_scale, kv8, dtype, batch_size=None):
    idt = torch.int64 if idx64 else torch.int32
    bs = p["seq"].shape[0] if batch_size is None else batch_size
    return c_header.call(
        lib, "sp_decode_attention", out=out, q=p["qkv"], k_buffer=p["kb"].t, v_buffer=p["vb"].t,
        req_to_token=p["table_dev"], req_to_token_stride=p["r2t_stride"], req_pool_indices=p["req"].to(idt).to(DEV),
        seq_lens=p["seq_dev"][idt], kv_start=None if p["kv_start"] is None else p["kv_start"].to(idt).to(DEV),
        idx64=idx64, batch_size=bs, num_q_heads=HQ, num_kv_heads=HKV, head_dim=D, q_stride=p["q_stride"],
        out_stride=out_stride, kv_buffer_stride=HKV * D + KV_PAD, sm_scale=D ** -0.5, logit_cap=0.0, k_scale=k_scale,
        v_scale=v_scale, max_seq_len=max_seq_len, chunk=chunk, max_slots=max_slots, ranges=ranges, workspace=workspace,
        workspace_bytes=workspace_bytes, plan=plan, plan_bytes=plan_bytes, dtype=CODE[dtype],
        kv_dtype=DT["SP_FP8_E5M2"] if kv8 else CODE[dtype], stream=stream())


def _prepare(p):
    p["table_dev"] = p["table"].to(DEV)
    p["seq_dev"] = {torch.int64: p["seq"].to(DEV), torch.int32: p["seq"].to(torch.int32).to(DEV)}


def _plan(lib, p, idx64, max_seq_len, chunk, max_slots, ranges):
    """a plan buffer of exactly sp_decode_plan_bytes() inside a guard, built from the step's lengths"""
    bs = p["seq"].shape[0]
    nbytes = c_header.call(lib, "sp_decode_plan_bytes", batch_size=bs, max_slots=max_slots, ranges=ranges)
    plan = Guarded(1, nbytes, nbytes, torch.uint8)
    run(lib, "sp_decode_plan", plan=plan.t, plan_bytes=nbytes, seq_lens=p["seq_dev"][torch.int64 if idx64 else torch.int32],
        idx64=idx64, batch_size=bs, max_seq_len=max_seq_len, chunk=chunk, max_slots=max_slots, ranges=ranges,
        stream=stream())
    plan.check("decode plan")
    return plan, nbytes


def _workspace(lib, slots):
    nbytes = c_header.call(lib, "sp_decode_attention_workspace_bytes", max_slots=slots, num_q_heads=HQ, v_head_dim=D)
    return Guarded(1, nbytes, nbytes, torch.uint8), nbytes


PLAN_KINDS = {"none": (False, False), "items+ranges": (True, True), "ranges": (False, True), "items": (True, False)}


@pytest.mark.parametrize("pool", ["bf16", "fp8"])
@pytest.mark.parametrize("kind", list(PLAN_KINDS))
def test_decode_attention(lib, kind, pool):
    """a ragged batch with an empty request and one whose device length exceeds max_seq_len, on every kind of plan,
    with and without kv_start, on int32 and int64 index tensors"""
    dtype = torch.bfloat16 if pool == "bf16" else torch.float16
    kv8 = pool == "fp8"
    k_scale, v_scale = (1.7, 0.37) if kv8 else (1.25, 0.75)
    max_seq_len, chunk, ranges_n = 300, 64, 7
    lens = [37, 0, max_seq_len + 50, 129, 1, 64]       # request 2: clamped to max_seq_len, its table row goes on
    bs = len(lens)
    items, with_ranges = PLAN_KINDS[kind]
    ranges = ranges_n if with_ranges else 0
    slots = c_header.call(lib, "sp_decode_plan_slots", batch_size=bs, kv_tokens=-1, max_seq_len=max_seq_len,
                          chunk=chunk) if items else 0
    out_stride = HQ * D + 24
    for kv_start in (None, [3, 11, 0, 40, 7, 2]):
        p = _decode_problem(17, lens, max_seq_len, kv_start, kv8, dtype)
        _prepare(p)
        fn, vw = _decode_reference(p, max_seq_len, k_scale, v_scale, kv8)
        ref = fn(vw)
        outs = {}
        for idx64 in (0, 1):
            plan, plan_bytes = (None, 0)
            if items or with_ranges:
                plan, plan_bytes = _plan(lib, p, idx64, max_seq_len, chunk, slots, ranges)
            ws_slots = max(slots, bs + ranges) if plan is not None else bs * math.ceil(max_seq_len / chunk)
            ws, ws_bytes = _workspace(lib, ws_slots)
            out = Guarded(bs, HQ * D, out_stride, dtype)
            rc = _decode_call(lib, p, out.t, out_stride, idx64, max_seq_len, chunk, slots, ranges,
                              None if plan is None else plan.t, plan_bytes, ws.t, ws_bytes, k_scale, v_scale, kv8, dtype)
            assert rc == OK, rc
            torch.cuda.synchronize()
            kernel = c_header.call(lib, "sp_debug_get", key=b"decode_last_kernel")
            assert kernel == (3 if with_ranges else 2), (kind, kernel)
            what = f"decode {pool} {kind} kv_start {kv_start is not None} idx64 {idx64}"
            rows = [b for b in range(bs) if lens[b] > 0]
            o = out.view3(HQ, D)
            if kv8:
                assert_close(o[rows], ref[rows], dtype, what=what, vmax=float(vw.abs().max()))
            else:
                assert_attn_close(o[rows], ref[rows], fn(vw.abs())[rows], dtype, what=what)
            out.check(what, rows)                       # the seq_len 0 row is left bit-unchanged
            ws.check(what + " workspace")
            if plan is not None:
                plan.check(what + " plan")
            outs[idx64] = out.t.cpu()
        assert torch.equal(outs[0], outs[1]), "int32 and int64 index tensors give the same bits"


def test_decode_out_rows_not_8_byte_aligned(lib):
    """out rows 4-byte but not 8-byte aligned: the items run the launch (correct output, not the range kernel); a plan
    without items cannot serve it and the call returns SP_ERR_INVALID_ARG, leaving `out` alone"""
    dtype = torch.bfloat16
    max_seq_len, chunk, ranges = 200, 64, 5
    lens = [150, 3, 200, 77]
    bs = len(lens)
    p = _decode_problem(23, lens, max_seq_len, None, False, dtype)
    _prepare(p)
    fn, vw = _decode_reference(p, max_seq_len, 1.0, 1.0, False)
    out_stride = HQ * D + 2                              # 2-byte elements: rows 4-byte aligned, every other one not 8
    slots = c_header.call(lib, "sp_decode_plan_slots", batch_size=bs, kv_tokens=int(sum(lens)),
                          max_seq_len=max_seq_len, chunk=chunk)
    for max_slots, want in ((slots, OK), (0, ST["SP_ERR_INVALID_ARG"])):
        plan, plan_bytes = _plan(lib, p, 1, max_seq_len, chunk, max_slots, ranges)
        ws, ws_bytes = _workspace(lib, max(max_slots, bs + ranges))
        out = Guarded(bs, HQ * D, out_stride, dtype)
        before = c_header.call(lib, "sp_debug_get", key=b"decode_last_kernel")
        rc = _decode_call(lib, p, out.t, out_stride, 1, max_seq_len, chunk, max_slots, ranges, plan.t, plan_bytes,
                          ws.t, ws_bytes, 1.0, 1.0, False, dtype)
        torch.cuda.synchronize()
        assert rc == want, (max_slots, rc)
        if want == OK:
            assert c_header.call(lib, "sp_debug_get", key=b"decode_last_kernel") != 3
            assert_attn_close(out.view3(HQ, D), fn(vw), fn(vw.abs()), dtype, what="decode, out rows 4-byte aligned")
            out.check("decode misaligned out")
        else:
            assert c_header.call(lib, "sp_debug_get", key=b"decode_last_kernel") == before
            out.check("decode refused", None)


# --------------------------------------------------------------------------- extend attention
@pytest.mark.parametrize("use_plan", [False, True])
@pytest.mark.parametrize("mode", ["causal", "window", "cross"])
@pytest.mark.parametrize("pool", ["bf16", "fp8"])
def test_extend_attention(lib, pool, mode, use_plan):
    dtype = torch.bfloat16 if pool == "bf16" else torch.float16
    kv8 = pool == "fp8"
    k_scale, v_scale = (1.7, 0.37) if kv8 else (1.25, 0.75)
    causal, window_left = {"causal": (1, -1), "window": (1, 17), "cross": (0, -1)}[mode]
    g = torch.Generator().manual_seed(31)
    ext = torch.tensor([5, 33, 70], dtype=torch.int32)
    prefix = torch.tensor([0, 20, 130], dtype=torch.int32)
    seq = (prefix + ext).to(torch.int64)
    kv_start = torch.tensor([4, 0, 9], dtype=torch.int64)
    bs, T_ = 3, int(ext.sum())
    max_seq_len = int(seq.max())
    P = 600
    kb, vb = _pool(g, P, kv8, dtype)
    r2t_stride = max_seq_len + 45
    table = torch.randint(1, P + 1, (bs + 2, r2t_stride), generator=g, dtype=torch.int32)
    req = torch.tensor([3, 0, 4], dtype=torch.int64)
    start_loc = torch.zeros(bs, dtype=torch.int32)
    start_loc[1:] = torch.cumsum(ext[:-1], 0)
    q_stride, out_stride = (HQ + 2 * HKV) * D + 8, HQ * D + 24
    qkv = torch.full((T_, q_stride), float("nan"))
    qkv[:, :HQ * D] = torch.randn(T_, HQ * D, generator=g)
    qkv = qkv.to(dtype).to(DEV)
    q = qkv[:, :HQ * D].float().cpu().view(T_, HQ, D)
    kw, vw = _widened(kb, kv8, k_scale), _widened(vb, kv8, v_scale)
    fn = lambda v: ops.extend_attention(q, kw, v, table, req, seq, ext, start_loc, D ** -0.5, causal=bool(causal),
                                        kv_start=kv_start, window_left=window_left)
    ref = fn(vw)
    ws_bytes = c_header.call(lib, "sp_extend_attention_workspace_bytes", num_tokens=T_, batch_size=bs, num_q_heads=HQ,
                             head_dim=D, dtype=CODE[dtype])
    plan_bytes = c_header.call(lib, "sp_extend_plan_bytes", num_tokens=T_, batch_size=bs, num_q_heads=HQ,
                               num_kv_heads=HKV)
    table_dev = table.to(DEV)
    outs = {}
    for idx64 in (0, 1):
        idt = torch.int64 if idx64 else torch.int32
        seq_d = seq.to(idt).to(DEV)
        plan = None
        if use_plan:
            plan = Guarded(1, plan_bytes, plan_bytes, torch.uint8)
            run(lib, "sp_extend_plan", plan=plan.t, plan_bytes=plan_bytes, extend_seq_lens=ext.to(DEV), seq_lens=seq_d,
                idx64=idx64, batch_size=bs, num_tokens=T_, num_q_heads=HQ, num_kv_heads=HKV, causal=causal,
                stream=stream())
        ws = Guarded(1, ws_bytes, ws_bytes, torch.uint8)
        out = Guarded(T_, HQ * D, out_stride, dtype)
        run(lib, "sp_extend_attention", out=out.t, q=qkv, k_buffer=kb.t, v_buffer=vb.t, req_to_token=table_dev,
            req_to_token_stride=r2t_stride, req_pool_indices=req.to(idt).to(DEV), seq_lens=seq_d,
            kv_start=kv_start.to(idt).to(DEV), idx64=idx64, extend_seq_lens=ext.to(DEV),
            extend_start_loc=start_loc.to(DEV), batch_size=bs, num_tokens=T_, num_q_heads=HQ, num_kv_heads=HKV,
            head_dim=D, q_stride=q_stride, out_stride=out_stride, kv_buffer_stride=HKV * D + KV_PAD,
            sm_scale=D ** -0.5, logit_cap=0.0, k_scale=k_scale, v_scale=v_scale, causal=causal,
            window_left=window_left, max_extend_len=int(ext.max()), max_seq_len=max_seq_len, workspace=ws.t,
            workspace_bytes=ws_bytes, plan=None if plan is None else plan.t, plan_bytes=plan_bytes if use_plan else 0,
            dtype=CODE[dtype], kv_dtype=DT["SP_FP8_E5M2"] if kv8 else CODE[dtype], stream=stream())
        what = f"extend {pool} {mode} plan {use_plan} idx64 {idx64}"
        o = out.view3(HQ, D)
        if kv8:
            assert_close(o, ref, dtype, what=what, vmax=float(vw.abs().max()))
        else:
            assert_attn_close(o, ref, fn(vw.abs()), dtype, what=what)
        out.check(what)
        ws.check(what + " workspace")
        if plan is not None:
            plan.check(what + " plan")
        kb.check(what + " k_buffer", None)
        outs[idx64] = out.t.cpu()
    assert torch.equal(outs[0], outs[1]), "int32 and int64 index tensors give the same bits"


# --------------------------------------------------------------------------- sampler
BIG_LOGIT = 1.0e4                                        # in the padding columns: above every real logit


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
def test_argmax(lib, dt):
    dtype = DTYPES[dt]
    g = torch.Generator().manual_seed(41)
    bs, vocab, row_stride = 4, 1000, 1037
    logits = torch.randn(bs, vocab, generator=g).to(dtype)
    logits[0, 17] = logits[0, 900] = 50.0               # a tie: the first index wins
    lg = padded(logits.to(DEV), row_stride, BIG_LOGIT)
    out = Guarded(1, bs, bs, torch.int64)
    run(lib, "sp_argmax", logits=lg.t, row_stride=row_stride, batch_size=bs, vocab=vocab, out_ids=out.t,
        dtype=CODE[dtype], stream=stream())
    assert torch.equal(out.t.cpu()[0], logits.float().argmax(-1)) and int(out.t[0, 0]) == 17
    out.check("argmax out_ids")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_argmax_shard_and_merge(lib, dt):
    """a [bs, 900] row cut into three shards of 300 real columns each, every shard with padding columns (row_stride >
    cols) holding the largest value; shard pairs carry global indices (index_offset > 0), the merge their argmax"""
    dtype = DTYPES[dt]
    g = torch.Generator().manual_seed(42)
    bs, cols, shards = 5, 300, 3
    full = torch.randn(bs, cols * shards, generator=g).to(dtype)
    full[1, 10] = full[1, 610] = 40.0                   # tie across shards: the lower global index wins
    full[2, 899] = 41.0                                 # the last real column of the last shard
    pairs = Guarded(shards * bs, 2, 2, torch.int32)
    for s in range(shards):
        row_stride = cols + 24 + 8 * s
        lg = padded(full[:, s * cols:(s + 1) * cols].contiguous().to(DEV), row_stride, BIG_LOGIT)
        dst = pairs.t[s * bs:(s + 1) * bs]
        run(lib, "sp_argmax_shard", logits=lg.t, row_stride=row_stride, batch_size=bs, cols=cols,
            index_offset=s * cols, out_pairs=dst, dtype=CODE[dtype], stream=stream())
        part = full[:, s * cols:(s + 1) * cols].float()
        got = dst.cpu()
        assert torch.equal(got[:, 0], part.max(-1).values.view(torch.int32)), s
        assert torch.equal(got[:, 1], (part.argmax(-1) + s * cols).to(torch.int32)), s
    pairs.check("argmax_shard out_pairs")
    out = Guarded(1, bs, bs, torch.int64)
    run(lib, "sp_argmax_merge", pairs=pairs.t, num_shards=shards, batch_size=bs, out_ids=out.t, stream=stream())
    assert torch.equal(out.t.cpu()[0], full.float().argmax(-1))
    assert int(out.t[0, 1]) == 10 and int(out.t[0, 2]) == 899
    out.check("argmax_merge out_ids")


@pytest.mark.parametrize("with_temperatures", [False, True])
def test_softmax_temperature(lib, with_temperatures):
    g = torch.Generator().manual_seed(43)
    bs, vocab, row_stride = 4, 1000, 1029
    logits = torch.randn(bs, vocab, generator=g) * 3
    temps = torch.tensor([0.7, 1.0, 1.9, 0.3])
    lg = padded(logits.to(DEV), row_stride, BIG_LOGIT)
    run(lib, "sp_softmax_temperature", logits_inout=lg.t, row_stride=row_stride,
        temperatures=temps.to(DEV) if with_temperatures else None, batch_size=bs, vocab=vocab, stream=stream())
    want = osamp.softmax_temperature(logits, temps if with_temperatures else torch.ones(bs))
    got = lg.t.cpu()
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-12)
    assert torch.allclose(got.sum(-1), torch.ones(bs), atol=1e-5)
    lg.check("softmax_temperature")


def _probs(seed, bs, vocab):
    g = torch.Generator().manual_seed(seed)
    scale = torch.tensor([0.5, 2.0, 5.0, 1.0, 8.0][:bs]).view(-1, 1)
    return torch.softmax(torch.randn(bs, vocab, generator=g) * scale, dim=-1)


FILTERS = ["all", "no_top_k", "no_top_p", "no_min_p"]
BIG_PROB = 2.0                                           # in the padding columns: above every probability


def _filters(which, bs, vocab):
    ks = torch.tensor([50, 3, 1 << 30, 700, 1][:bs], dtype=torch.int32)
    ps = torch.tensor([0.9, 1.0, 0.5, 0.95, 0.3][:bs])
    ms = torch.tensor([0.0, 0.05, 0.01, 0.001, 0.2][:bs])
    dev = dict(top_ks=ks.to(DEV), top_ps=ps.to(DEV), min_ps=ms.to(DEV))
    ref = [(int(min(ks[b], vocab)), float(ps[b]), float(ms[b])) for b in range(bs)]
    if which == "no_top_k":
        dev["top_ks"], ref = None, [(vocab, p, m) for _, p, m in ref]
    if which == "no_top_p":
        dev["top_ps"], ref = None, [(k, 2.0, m) for k, _, m in ref]        # no mass bound at all
    if which == "no_min_p":
        dev["min_ps"], ref = None, [(k, p, 0.0) for k, p, _ in ref]
    return dev, ref


@pytest.mark.parametrize("which", FILTERS)
def test_top_k_top_p_min_p_sample(lib, which):
    bs, vocab, row_stride = 5, 2000, 2000 + 44
    probs = _probs(44, bs, vocab)
    u = torch.tensor([0.1, 0.5, 0.93, 0.0, 0.77])
    dev, ref = _filters(which, bs, vocab)
    pr = padded(probs.to(DEV), row_stride, BIG_PROB)
    ids, cnt = Guarded(1, bs, bs, torch.int64), Guarded(1, bs, bs, torch.int32)
    run(lib, "sp_top_k_top_p_min_p_sample", probs=pr.t, row_stride=row_stride, **dev, uniform=u.to(DEV),
        batch_size=bs, vocab=vocab, out_ids=ids.t, keep_count=cnt.t, stream=stream())
    pn = probs.numpy()
    for b, (k, p, m) in enumerate(ref):
        keep, _ = osamp.select(pn[b], k, p, m)
        assert int(cnt.t[0, b]) == int(keep.sum()), (which, b)
        assert int(ids.t[0, b]) == osamp.sample(pn[b], k, p, m, float(u[b])), (which, b)
    ids.check("sample out_ids")
    cnt.check("sample keep_count")
    pr.check("sample probs", None)


@pytest.mark.parametrize("which", FILTERS)
def test_top_k_top_p_min_p_renorm(lib, which):
    bs, vocab, row_stride, out_stride = 5, 2000, 2000 + 44, 2000 + 12
    probs = _probs(45, bs, vocab)
    dev, ref = _filters(which, bs, vocab)
    pr = padded(probs.to(DEV), row_stride, BIG_PROB)
    out, cnt = Guarded(bs, vocab, out_stride, torch.float32), Guarded(1, bs, bs, torch.int32)
    run(lib, "sp_top_k_top_p_min_p_renorm", probs=pr.t, row_stride=row_stride, **dev, batch_size=bs, vocab=vocab,
        out=out.t, out_stride=out_stride, keep_count=cnt.t, stream=stream())
    got, pn = out.t.cpu().numpy(), probs.numpy()
    for b, (k, p, m) in enumerate(ref):
        want = osamp.renorm(pn[b], k, p, m)
        assert np.array_equal(got[b] > 0, want > 0), (which, b)
        assert np.allclose(got[b], want, rtol=2e-7, atol=0), (which, b)
        assert int(cnt.t[0, b]) == int((want > 0).sum()), (which, b)
    out.check("renorm out")
    cnt.check("renorm keep_count")
    pr.check("renorm probs", None)


# --------------------------------------------------------------------------- small-batch projection
@pytest.mark.parametrize("epilogue", [0, 1])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_gemm_skinny(lib, dt, epilogue):
    dtype = DTYPES[dt]
    g = torch.Generator().manual_seed(46 + epilogue)
    M, N, K = 5, 48, 256
    xs, ws_, os_ = K + 24, K + 40, N + 24
    x0 = torch.randn(M, K, generator=g).to(dtype)
    w0 = (torch.randn(N * (1 + epilogue), K, generator=g) * 0.05).to(dtype)
    x, w = padded(x0.to(DEV), xs, float("nan")), padded(w0.to(DEV), ws_, float("nan"))
    out = Guarded(M, N, os_, dtype)
    run(lib, "sp_gemm_skinny", out=out.t, x=x.t, w=w.t, M=M, N=N, K=K, x_stride=xs, w_stride=ws_, out_stride=os_,
        epilogue=epilogue, dtype=CODE[dtype], stream=stream())
    ref = x0.float() @ w0.float().T
    eps = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    got = out.t.float().cpu()
    if epilogue == 0:
        err = (got - ref).abs()
        assert bool((err <= eps * ref.abs() + 1e-4 * ref.abs().max()).all()), float(err.max())
    else:
        act = ops.silu_and_mul(ref.to(dtype)).float()       # the projection rounded once, then SiluAndMul
        err = (got - act).abs()
        assert bool((err <= 4 * eps * act.abs() + 4 * eps * act.abs().max()).all()), float(err.max())
    out.check(f"gemm_skinny epilogue {epilogue}")
    x.check("gemm_skinny x", None)
    w.check("gemm_skinny w", None)


# --------------------------------------------------------------------------- empty batches
def test_batch_size_zero_writes_nothing(lib):
    """every entry point that takes a batch size returns SP_OK for 0 and writes nothing, whatever the buffers hold"""
    buf = Guarded(1, 1 << 16, 1 << 16, torch.uint8)
    a = buf.t[0, 4096:]                                  # a device buffer far from both guard ends
    calls = {
        "sp_write_req_to_token": dict(req_to_token=a, row_stride=37, req_pool_indices=a, pre_lens=a, seq_lens=a,
                                      extend_lens=a, out_cache_loc=a),
        "sp_compute_position": dict(positions=a, extend_start_loc=a, extend_prefix_lens=a, extend_seq_lens=a),
        "sp_clamp_position": dict(positions=a, seq_lens=a, idx64=1),
        "sp_decode_plan": dict(plan=a, plan_bytes=16, seq_lens=a, idx64=0, max_seq_len=300, chunk=64, max_slots=6,
                               ranges=7),
        "sp_decode_attention": dict(out=a, q=a, k_buffer=a, v_buffer=a, req_to_token=a, req_to_token_stride=377,
                                    req_pool_indices=a, seq_lens=a, kv_start=None, idx64=0, num_q_heads=HQ,
                                    num_kv_heads=HKV, head_dim=D, q_stride=1544, out_stride=1048,
                                    kv_buffer_stride=272, sm_scale=0.1, logit_cap=0.0, k_scale=1.25, v_scale=0.75,
                                    max_seq_len=300, chunk=64, max_slots=6, ranges=7, workspace=a, workspace_bytes=16,
                                    plan=a, plan_bytes=16, dtype=DT["SP_BF16"], kv_dtype=DT["SP_BF16"]),
        "sp_extend_plan": dict(plan=a, plan_bytes=16, extend_seq_lens=a, seq_lens=a, idx64=0, num_tokens=0,
                               num_q_heads=HQ, num_kv_heads=HKV, causal=1),
        "sp_extend_attention": dict(out=a, q=a, k_buffer=a, v_buffer=a, req_to_token=a, req_to_token_stride=377,
                                    req_pool_indices=a, seq_lens=a, kv_start=None, idx64=0, extend_seq_lens=a,
                                    extend_start_loc=a, num_tokens=0, num_q_heads=HQ, num_kv_heads=HKV, head_dim=D,
                                    q_stride=1544, out_stride=1048, kv_buffer_stride=272, sm_scale=0.1,
                                    logit_cap=0.0, k_scale=1.25, v_scale=0.75, causal=1, window_left=-1,
                                    max_extend_len=0, max_seq_len=0, workspace=a, workspace_bytes=16, plan=a,
                                    plan_bytes=16, dtype=DT["SP_BF16"], kv_dtype=DT["SP_BF16"]),
        "sp_argmax": dict(logits=a, row_stride=1037, vocab=1000, out_ids=a, dtype=DT["SP_F32"]),
        "sp_argmax_shard": dict(logits=a, row_stride=324, cols=300, index_offset=300, out_pairs=a, dtype=DT["SP_F32"]),
        "sp_argmax_merge": dict(pairs=a, num_shards=3, out_ids=a),
        "sp_softmax_temperature": dict(logits_inout=a, row_stride=1029, temperatures=a, vocab=1000),
        "sp_top_k_top_p_min_p_sample": dict(probs=a, row_stride=2044, top_ks=a, top_ps=a, min_ps=a, uniform=a,
                                            vocab=2000, out_ids=a, keep_count=a),
        "sp_top_k_top_p_min_p_renorm": dict(probs=a, row_stride=2044, top_ks=a, top_ps=a, min_ps=a, vocab=2000,
                                            out=a, out_stride=2012, keep_count=a),
    }
    takes_bs = sorted(n for n, (_, args) in lib.sp_prototypes.items() if any(p == "batch_size" for p, _ in args)
                      and n != "sp_decode_plan_slots" and not n.endswith("_bytes"))
    assert sorted(calls) == takes_bs
    for name, kw in calls.items():
        rc = c_header.call(lib, name, batch_size=0, stream=stream(), **kw)
        torch.cuda.synchronize()
        assert rc == OK, (name, rc)
        buf.check(f"{name} with batch_size 0", None)
