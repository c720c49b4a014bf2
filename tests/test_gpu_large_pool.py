"""The KV-pool kernels with keys and stores beyond 2 GiB and 4 GiB of their pool's base.

Every kernel that reads or writes the paged pool turns a slot into a byte address; several narrow that arithmetic on
purpose (decode_mfma.hip: a 32-bit token stride times a 32-bit slot into one 64-bit multiply-add; extend_w64.hip: the
same, with the swizzle XORed into the finished address).  A default pool (MHATokenToKVPool, one arena
[layers, P+1, 2, Hkv, D] sized from free memory) is several GiB per layer, so a server under load keeps keys there.

A "far pool" is one allocation: a guard of 2 GiB + 1 MiB, then an arena [P+1, 2, Hkv, D] that ends past 4 GiB + 1 MiB,
with K and V its two strided views (either way round: V below K makes the range kernel's V - K distance negative).  Every
byte starts as 0xFF (NaN in every float type the pool holds, e5m2 included).  Real rows sit only at the slots a problem
uses, drawn from three bands - below 2 GiB, a run across the 2^31-byte line, above 4 GiB up to the last row - mixed
inside 64-key tiles, and one request lies above 4 GiB entirely.  For every used slot above 4 GiB, the slot at the same
offset modulo 2^32 (its "decoy") holds other finite rows:
  - an address truncated to 32 bits reads a plausible wrong row, which the oracle comparison catches;
  - a sign-extended 32-bit offset lands in the guard and reads NaN: a non-finite output, not a fault.

Each launch is checked (a) against the fp32 oracle over the used rows compacted to a small pool, (b) bit for bit against
the same launch on that compacted pool on the GPU - a result does not depend on where its rows live - and (c), where a
kernel is meant, by sp_debug_get.  Each store must write exact rows and nothing else: the count of non-NaN elements of
the whole allocation, guard included, grows by exactly what was written, and the decoys stay as they were.

End to end, a ModelRunner whose allocator has handed its first 4 GiB of slots to nobody serves prefills and decode steps
(eager and under graph replay) with the bits of a twin runner over a small pool."""
import gc
import random

import pytest
import torch

from oracle import ops
from tests.helpers import assert_attn_close, assert_close
from tests.test_gpu_attention import RANGE_KERNEL, nat, run_decode, run_extend, w64  # noqa: F401  (fixtures)
from tests.test_gpu_elementwise import ulp_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 2 ** 31 + 2 ** 20
FP8 = torch.uint8                                   # the byte pool of --kv-cache-dtype fp8_e5m2
VALU_KERNEL, ITEM_KERNEL = 1, 2                     # sp_debug_get("decode_last_kernel")
W8_KERNEL, W64_KERNEL, W64P_KERNEL = 1, 2, 3        # sp_debug_get("extend_last_kernel")


def _skip_small_device():
    total = torch.cuda.get_device_properties(0).total_memory
    if total < 16 * 2 ** 30:
        pytest.skip(f"a far pool needs ~6.1 GiB at once; this device has {total / 2 ** 30:.1f} GiB in all")


class FarPool:
    """One far pool (see the module docstring).  take() hands out unused slots of a band, fill() writes random rows at
    them (and their decoys), low() compacts the used rows into a small pool of the same layout."""

    def __init__(self, dtype, Hkv, D, swap=False, seed=0):
        self.dtype, self.Hkv, self.D, self.swap = dtype, Hkv, D, swap
        self.tok = 2 * Hkv * D * torch.empty(0, dtype=dtype).element_size()      # token stride in bytes
        self.P = (2 ** 32 + 2 ** 26) // self.tok
        self.n2, self.n4 = 2 ** 31 // self.tok, 2 ** 32 // self.tok               # slots at 2 GiB, 4 GiB
        self.buf = torch.full((GUARD + (self.P + 1) * self.tok,), 0xFF, dtype=torch.uint8, device=DEV)
        self.arena = self.buf[GUARD:].view(dtype).view(self.P + 1, 2, Hkv, D)
        k, v = (1, 0) if swap else (0, 1)
        self.kb, self.vb = self.arena[:, k], self.arena[:, v]
        assert self.kb.stride(0) * self.kb.element_size() == self.tok
        self.gen = torch.Generator().manual_seed(seed)
        self.rng = random.Random(seed)
        self.used, self.decoys = set(), {}
        self.arena[0] = self.rows(1)[0].to(DEV)        # the dummy row padded lanes read: finite, as in a served pool
        self.bands = {"low": range(self.P - self.n4 + 1, self.n2 - 1024),   # (above the decoys' range)
                      "mid": range(self.n2 - 512, self.n2 + 512),
                      "high": range(self.n4 + 1, self.P + 1)}

    def rows(self, n):
        x = torch.randn(n, 2, self.Hkv, self.D, generator=self.gen)
        return x.to(torch.float8_e5m2).view(torch.uint8) if self.dtype == FP8 else x.to(self.dtype)

    def take(self, n, band):
        out = []
        while len(out) < n:
            s = self.rng.choice(self.bands[band])
            if s not in self.used:
                self.used.add(s)
                out.append(s)
        return out

    def mixed(self, n):
        """n slots, a third of each band, shuffled (so that one 64-key tile holds all three); the last slot of the pool
        is among the first that are asked for"""
        if n == 0:
            return []
        last = [] if self.P in self.used else [self.P]
        self.used.update(last)
        rest = n - len(last)
        s = last + self.take(rest // 3, "low") + self.take(rest // 3, "mid") + self.take(rest - 2 * (rest // 3), "high")
        self.rng.shuffle(s)
        return s

    def fill(self):
        """random rows at every used slot; at the decoy of each one above 4 GiB, other random rows"""
        used = sorted(self.used)
        self.arena[torch.tensor(used, device=DEV)] = self.rows(len(used)).to(DEV)
        dec = sorted(s - self.n4 for s in used if s >= self.n4)
        assert dec and not set(dec) & self.used and dec[0] >= 1
        rows = self.rows(len(dec))
        self.arena[torch.tensor(dec, device=DEV)] = rows.to(DEV)
        self.decoys = dict(idx=torch.tensor(dec, device=DEV), rows=rows)

    def decoys_intact(self):
        return torch.equal(self.arena[self.decoys["idx"]].cpu(), self.decoys["rows"])

    def low(self, r2t):
        """the used rows (and the dummy row) compacted into a small arena of the same layout: (k, v, r2t remapped)"""
        keep = torch.tensor([0] + sorted(self.used), device=DEV)
        arena = self.arena[keep].contiguous()
        k, v = (1, 0) if self.swap else (0, 1)
        r2t_low = torch.searchsorted(keep, r2t.long()).to(torch.int32)
        assert torch.equal(keep[r2t_low.long()], r2t.long())
        return arena[:, k], arena[:, v], r2t_low

    def non_nan(self):
        """non-NaN elements of the whole allocation, guard included (counted on the device, 16 M at a time)"""
        flat = self.buf.view(self.dtype)
        n = 0
        for c in flat.split(2 ** 24):
            n += int((c != 0xFF).sum()) if self.dtype == FP8 else int((~torch.isnan(c)).sum())
        return n

    def free(self):
        # (the storage itself, not this object's references: views of it may outlive the test in a traceback)
        self.buf.untyped_storage().resize_(0)
        del self.buf, self.arena, self.kb, self.vb


@pytest.fixture
def far_pool():
    """make(dtype, Hkv, D, swap, seed) -> FarPool; one per test, freed afterwards"""
    _skip_small_device()
    made = []

    def make(*a, **kw):
        assert not made, "one far pool at a time"
        made.append(FarPool(*a, **kw))
        return made[0]
    torch.cuda.reset_peak_memory_stats()
    yield make
    print(f"[far pool] peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")
    for fp in made:
        fp.free()
    made.clear()
    gc.collect()
    torch.cuda.empty_cache()


def paged(fp, lens, high_req, seed, split=None, high_first=False):
    """the table of a problem over far pool fp: request high_req's keys all above 4 GiB, every other request's keys
    from the three bands - except, where `split` is given, the positions at or past split[b] (high_first: before it),
    which lie above 4 GiB too"""
    g = torch.Generator().manual_seed(seed)
    bs = len(lens)
    r2t = torch.zeros(bs + 2, max(lens) + 4, dtype=torch.int32)
    req = torch.randperm(bs + 2, generator=g)[:bs]
    for b, n in enumerate(lens):
        if b == high_req:
            s = fp.take(n, "high")
        else:
            cut = n if split is None else min(n, split[b])
            s = fp.take(cut, "high") + fp.mixed(n - cut) if high_first else fp.mixed(cut) + fp.take(n - cut, "high")
        r2t[req[b], :n] = torch.tensor(s, dtype=torch.int32)
    fp.fill()
    return r2t.to(DEV), req.to(DEV), g


def act_dtype(fp, dt):
    return dt if fp.dtype == FP8 else fp.dtype


def oracle_pool(kb, vb, fp, k_scale, v_scale):
    """fp32 CPU copies of a (compacted) pool; a byte pool widened from e5m2 and multiplied by the layer scales"""
    if fp.dtype == FP8:
        return (kb.cpu().view(torch.float8_e5m2).float() * k_scale, vb.cpu().view(torch.float8_e5m2).float() * v_scale)
    return kb.float().cpu(), vb.float().cpu()


def against_oracle(o, fn, kc, vc, fp, dtype, what):
    """o against fn(k, v) in fp32: the attention error model for 16-bit pools (<= 1 unit), vmax for a byte pool,
    the plain fp32 bar for fp32"""
    ref = fn(kc, vc)
    if fp.dtype == FP8:
        assert_close(o, ref, dtype, what=what, vmax=float(vc.abs().max()))
    elif dtype == torch.float32:
        assert_close(o, ref, dtype, what=what)
    else:
        assert_attn_close(o, ref, fn(kc, vc.abs()), dtype, what=what)


# ----------------------------------------------------------------------------------- decode
def decode_checks(nat, fp, p, low, scale, what, kernel=None, kv_start=None, k_scale=None, v_scale=None, **kw):
    """one launch on the far pool and on its compacted twin: oracle, bits, kernel"""
    dtype = p["q"].dtype
    o = run_decode(nat, p, scale, kv_start=kv_start, k_scale=k_scale, v_scale=v_scale, **kw)
    ran = nat.debug_get("decode_last_kernel")
    c = {k: p[k].cpu() for k in ("q", "req_pool_indices", "seq_lens")}
    kc, vc = oracle_pool(low["k_buffer"], low["v_buffer"], fp, k_scale or 1.0, v_scale or 1.0)
    fn = lambda k, v: ops.decode_attention(c["q"].float(), k, v, low["req_to_token"].cpu(), c["req_pool_indices"],
                                           c["seq_lens"], scale, kw.get("cap", 0.0),
                                           None if kv_start is None else kv_start.cpu())
    against_oracle(o, fn, kc, vc, fp, dtype, what)
    o_low = run_decode(nat, {**p, **low}, scale, kv_start=kv_start, k_scale=k_scale, v_scale=v_scale, **kw)
    assert torch.equal(o, o_low), f"{what}: the far pool's result differs from the compacted pool's"
    if kernel is not None:
        assert ran == kernel, f"{what}: decode kernel {ran} ran, {kernel} was meant"
    return o


def decode_problem(fp, Hq, seed, lens=(300, 129, 64, 1, 700, 65), high_req=4, dt=torch.bfloat16):
    r2t, req, g = paged(fp, list(lens), high_req, seed)
    q = torch.randn(len(lens), Hq, fp.D, generator=g).to(act_dtype(fp, dt)).to(DEV)
    p = dict(q=q, k_buffer=fp.kb, v_buffer=fp.vb, req_to_token=r2t, req_pool_indices=req,
             seq_lens=torch.tensor(lens, device=DEV))
    kl, vl, rl = fp.low(r2t)
    return p, dict(k_buffer=kl, v_buffer=vl, req_to_token=rl)


def forced(nat, key, value, reset):
    class _Ctx:
        def __enter__(self):
            nat.debug_set(key, value)

        def __exit__(self, *exc):
            nat.debug_set(key, reset)
    return _Ctx()


DECODE_SHAPES = pytest.mark.parametrize("Hq,Hkv,D", [(32, 8, 128), (16, 8, 64), (8, 1, 128)])
SWAP = pytest.mark.parametrize("swap", [False, True], ids=["k-below-v", "v-below-k"])
DT16 = pytest.mark.parametrize("dt", ["bf16", "f16"])


def decode_case(far_pool, dt, Hq, Hkv, D, swap):
    dtype = {"bf16": torch.bfloat16, "f16": torch.float16}[dt]
    fp = far_pool(dtype, Hkv, D, swap, seed=Hq + D)
    p, low = decode_problem(fp, Hq, seed=Hq + D + 1)
    return fp, p, low, f"{dt} {Hq}/{Hkv}/{D} {'V below K' if swap else 'K below V'}"


@SWAP
@DECODE_SHAPES
@DT16
def test_decode_range_kernel_beyond_4gib(nat, far_pool, dt, Hq, Hkv, D, swap):
    """The range kernel in the form that ships (a plan without items, its range section, the separate merge); it streams
    its gathers always (the library's default and decode_nt_min_mb 0; "never" sends a launch to the items)"""
    fp, p, low, name = decode_case(far_pool, dt, Hq, Hkv, D, swap)
    ranges = nat.decode_ranges(Hq, Hkv, D, p["q"].dtype)
    assert ranges > 0
    outs = {}
    for nt in (-2, 0):
        with forced(nat, "decode_nt_min_mb", nt, -2):
            outs[nt] = decode_checks(nat, fp, p, low, D ** -0.5, f"range kernel, nt {nt}, {name}", RANGE_KERNEL,
                                     ranges=ranges, items=False)
    assert torch.equal(outs[0], outs[-2])
    assert fp.decoys_intact()


@SWAP
@DECODE_SHAPES
@DT16
def test_decode_item_kernels_beyond_4gib(nat, far_pool, dt, Hq, Hkv, D, swap):
    """The matrix-core item kernel with its gathers streaming and plain (decode_nt_min_mb 0 and -1) and with a logit
    soft-cap (its CAP instantiation), the VALU kernel, and the plan-less static grid"""
    fp, p, low, name = decode_case(far_pool, dt, Hq, Hkv, D, swap)
    scale = D ** -0.5
    with forced(nat, "decode_kernel", 2, 0):
        outs = []
        for nt in (0, -1):
            with forced(nat, "decode_nt_min_mb", nt, -2):
                outs.append(decode_checks(nat, fp, p, low, scale, f"item kernel, nt {nt}, {name}", ITEM_KERNEL))
        assert torch.equal(outs[0], outs[1]), "the cache policy changes no bit"
        decode_checks(nat, fp, p, low, scale, f"item kernel, soft cap, {name}", ITEM_KERNEL, cap=30.0)
    with forced(nat, "decode_kernel", 1, 0):
        decode_checks(nat, fp, p, low, scale, f"VALU kernel, {name}", VALU_KERNEL)
    decode_checks(nat, fp, p, low, scale, f"plan-less static grid, {name}", ITEM_KERNEL, use_plan=False)
    assert fp.decoys_intact()


def test_decode_fp32_pool_beyond_4gib(nat, far_pool):
    """fp32 takes the VALU kernel, with a plan and without (an 8 KiB token stride: 2^19 slots to 4 GiB)"""
    fp = far_pool(torch.float32, 8, 128, True, seed=32)
    p, low = decode_problem(fp, 32, seed=33)
    decode_checks(nat, fp, p, low, 128 ** -0.5, "fp32 pool, plan", VALU_KERNEL)
    decode_checks(nat, fp, p, low, 128 ** -0.5, "fp32 pool, plan-less", VALU_KERNEL, use_plan=False)


@pytest.mark.parametrize("swap", [False, True], ids=["k-below-v", "v-below-k"])
def test_decode_fp8_pool_beyond_4gib(nat, far_pool, swap):
    """an e5m2 byte pool (2 KiB token stride) with layer scales != 1, through the range kernel and the item kernel"""
    fp = far_pool(FP8, 8, 128, swap, seed=8)
    p, low = decode_problem(fp, 32, seed=9)
    kw = dict(k_scale=1.7, v_scale=0.37)
    ranges = nat.decode_ranges(32, 8, 128, torch.bfloat16, torch.uint8)
    decode_checks(nat, fp, p, low, 128 ** -0.5, "fp8 pool, range kernel", RANGE_KERNEL, ranges=ranges, items=False,
                  **kw)
    with forced(nat, "decode_kernel", 2, 0):
        decode_checks(nat, fp, p, low, 128 ** -0.5, "fp8 pool, item kernel", ITEM_KERNEL, **kw)


def test_decode_encoder_decoder_beyond_4gib(nat, far_pool):
    """Mllama's two launches per layer: cross attention over the encoder slots (seq_lens = encoder lengths) and
    self-attention behind them (kv_start = encoder lengths, pointing at keys above 4 GiB), on the range kernel and
    the item kernel"""
    fp = far_pool(torch.bfloat16, 8, 128, False, seed=40)
    enc, dec = [90, 400, 7, 130], [5, 70, 200, 1]
    r2t, req, g = paged(fp, [e + d for e, d in zip(enc, dec)], 1, seed=41, split=enc)
    q = torch.randn(len(enc), 32, 128, generator=g).to(torch.bfloat16).to(DEV)
    kl, vl, rl = fp.low(r2t)
    low = dict(k_buffer=kl, v_buffer=vl, req_to_token=rl)
    enc_t, dec_t = torch.tensor(enc, device=DEV), torch.tensor(dec, device=DEV)
    ranges = nat.decode_ranges(32, 8, 128, torch.bfloat16)
    base = dict(q=q, k_buffer=fp.kb, v_buffer=fp.vb, req_to_token=r2t, req_pool_indices=req)
    for what, seq, k0 in (("cross", enc_t, None), ("self behind the encoder", dec_t, enc_t)):
        p = {**base, "seq_lens": seq}
        decode_checks(nat, fp, p, low, 0.09, f"{what}, range kernel", RANGE_KERNEL, kv_start=k0, ranges=ranges,
                      items=False)
        with forced(nat, "decode_kernel", 2, 0):
            decode_checks(nat, fp, p, low, 0.09, f"{what}, item kernel", ITEM_KERNEL, kv_start=k0)


# ----------------------------------------------------------------------------------- extend
def extend_problem(fp, Hq, pre, ext, high_req, seed, dt=torch.bfloat16):
    """prefix keys above 4 GiB, new keys from the three bands, request high_req above 4 GiB entirely"""
    lens = [a + b for a, b in zip(pre, ext)]
    r2t, req, g = paged(fp, lens, high_req, seed, split=pre, high_first=True)
    q = torch.randn(sum(ext), Hq, fp.D, generator=g).to(act_dtype(fp, dt)).to(DEV)
    ext_t = torch.tensor(ext, dtype=torch.int32, device=DEV)
    start = torch.zeros(len(ext), dtype=torch.int32, device=DEV)
    start[1:] = torch.cumsum(ext_t[:-1], 0)
    kl, vl, rl = fp.low(r2t)
    return dict(q=q, r2t=r2t, req=req, seq=torch.tensor(lens, device=DEV), ext=ext_t, start=start), \
        dict(k_buffer=kl, v_buffer=vl, req_to_token=rl)


def extend_checks(nat, fp, e, low, what, kernel=None, seq=None, k_scale=None, v_scale=None, **kw):
    seq = e["seq"] if seq is None else seq
    q = e["q"]
    scale = q.shape[2] ** -0.5
    args = (e["req"], seq, e["ext"], e["start"], scale)
    o = run_extend(nat, q, fp.kb, fp.vb, e["r2t"], *args, k_scale=k_scale, v_scale=v_scale, **kw)
    ran = nat.debug_get("extend_last_kernel")
    kc, vc = oracle_pool(low["k_buffer"], low["v_buffer"], fp, k_scale or 1.0, v_scale or 1.0)
    k0 = kw.get("kv_start")
    fn = lambda k, v: ops.extend_attention(q.cpu().float(), k, v, low["req_to_token"].cpu(), e["req"].cpu(), seq.cpu(),
                                           e["ext"].cpu(), e["start"].cpu(), scale, kw.get("cap", 0.0),
                                           causal=kw.get("causal", True), kv_start=None if k0 is None else k0.cpu(),
                                           window_left=kw.get("window_left", -1))
    against_oracle(o, fn, kc, vc, fp, q.dtype, what)
    o_low = run_extend(nat, q, low["k_buffer"], low["v_buffer"], low["req_to_token"], *args, k_scale=k_scale,
                       v_scale=v_scale, **kw)
    assert torch.equal(o, o_low), f"{what}: the far pool's result differs from the compacted pool's"
    if kernel is not None:
        assert ran == kernel, f"{what}: extend kernel {ran} ran, {kernel} was meant"
    return o


EXT_PRE, EXT_LEN = [300, 0, 65, 700, 0], [130, 200, 1, 64, 257]


@pytest.mark.parametrize("dt,D,swap", [("bf16", 128, False), ("f16", 128, True), ("bf16", 64, True),
                                       ("f16", 64, False)])
def test_extend_eight_wave_kernel_beyond_4gib(nat, far_pool, w64, dt, D, swap):
    """extend_w64 = 0: the eight-wave kernel, plain attention, a sliding window and a soft-cap, each with its K/V
    tiles by LDS-DMA into the swizzled ring (the default for 16-bit pools) and staged through registers (extend_dma 0)"""
    dtype = {"bf16": torch.bfloat16, "f16": torch.float16}[dt]
    Hq = 32 if D == 128 else 16
    fp = far_pool(dtype, 8, D, swap, seed=D + 3)
    e, low = extend_problem(fp, Hq, EXT_PRE, EXT_LEN, 1, seed=D + 4, dt=dtype)
    w64(0)
    name = f"{dt} D {D} {'V below K' if swap else 'K below V'}"
    for dma, staging in ((1, "LDS-DMA ring"), (0, "register staging")):
        with forced(nat, "extend_dma", dma, 1):
            extend_checks(nat, fp, e, low, f"eight-wave, {staging}, {name}", W8_KERNEL)
            extend_checks(nat, fp, e, low, f"eight-wave, {staging}, window 100, {name}", W8_KERNEL, window_left=100)
            extend_checks(nat, fp, e, low, f"eight-wave, {staging}, soft cap, {name}", W8_KERNEL, cap=30.0)
    assert fp.decoys_intact()


@pytest.mark.parametrize("persist", [0, 2], ids=["per-item", "persistent"])
@pytest.mark.parametrize("dt,swap", [("bf16", False), ("f16", True)])
def test_extend_w64_kernel_beyond_4gib(nat, far_pool, w64, dt, swap, persist):
    """extend_w64 = 2 with a plan, in the form with one workgroup per item and in the persistent form; prefixes above
    4 GiB, prompts of several tiles; then the cross-attention form (non-causal over a kv_start window), on the eight-wave
    kernel and on this one"""
    dtype = {"bf16": torch.bfloat16, "f16": torch.float16}[dt]
    fp = far_pool(dtype, 8, 128, swap, seed=64 + persist)
    e, low = extend_problem(fp, 32, EXT_PRE, EXT_LEN, 1, seed=65, dt=dtype)
    name = f"{dt} {'V below K' if swap else 'K below V'} persist {persist}"
    kernel = W64P_KERNEL if persist else W64_KERNEL
    plan = nat.extend_plan(e["ext"], e["seq"], int(e["ext"].sum()), 32, 8, True)
    w64(2, persist)
    extend_checks(nat, fp, e, low, f"w64, {name}", kernel, plan=plan)
    # cross attention: every new row sees keys [kv_start, kv_start + enc) of its row - above 4 GiB for most
    enc = torch.tensor([200, 150, 60, 500, 257], device=DEV)
    k0 = torch.tensor([100, 50, 5, 200, 0], device=DEV)
    xplan = nat.extend_plan(e["ext"], enc, int(e["ext"].sum()), 32, 8, False)
    w64(0)
    o8 = extend_checks(nat, fp, e, low, f"cross, eight-wave, {name}", W8_KERNEL, seq=enc, causal=False, kv_start=k0)
    w64(2, persist)
    o = extend_checks(nat, fp, e, low, f"cross, w64, {name}", kernel, seq=enc, causal=False, kv_start=k0, plan=xplan)
    assert torch.equal(o, o8), "cross rows: the two extend kernels agree bit for bit"
    assert fp.decoys_intact()


def test_extend_fp8_pool_beyond_4gib(nat, far_pool):
    fp = far_pool(FP8, 8, 128, True, seed=88)
    e, low = extend_problem(fp, 32, EXT_PRE, EXT_LEN, 1, seed=89)
    extend_checks(nat, fp, e, low, "fp8 pool, scaled", W8_KERNEL, k_scale=1.7, v_scale=0.37)


# ----------------------------------------------------------------------------------- stores
def store_slots(fp, n):
    """n unused slots: most above 4 GiB (the last row among them), a few across the 2^31-byte line"""
    s = ([fp.P] if fp.P not in fp.used else []) + fp.take(n - 8, "high")
    fp.used.update(s[:1])
    s += fp.take(n - len(s), "mid")
    fp.rng.shuffle(s)
    return s


def prepare_store(fp, n_used=64, n_store=77):
    """decoys for the slots a store will write (so that a truncated address hits finite rows); the rows at the used
    slots; the count of non-NaN elements before the store"""
    loc = store_slots(fp, n_store)
    fp.mixed(n_used)
    for s in loc:
        fp.used.discard(s)
    fp.fill()                      # rows at the used slots and decoys of the high ones
    dec = sorted(s - fp.n4 for s in loc if s >= fp.n4)
    rows = fp.rows(len(dec))
    fp.arena[torch.tensor(dec, device=DEV)] = rows.to(DEV)
    idx = torch.cat([fp.decoys["idx"], torch.tensor(dec, device=DEV)])
    fp.decoys = dict(idx=idx, rows=torch.cat([fp.decoys["rows"], rows]))
    fp.used.update(loc)
    return torch.tensor(loc, dtype=torch.int64, device=DEV), fp.non_nan()


def after_store(fp, before, written, what):
    got = fp.non_nan()
    assert got == before + written, f"{what}: {got - before} elements turned non-NaN, {written} were written"
    assert fp.decoys_intact(), f"{what}: a decoy row changed"


@pytest.mark.parametrize("case", ["16-byte", "element", "fp32 16-byte", "fp32 element"])
def test_kv_store_beyond_4gib(nat, far_pool, case):
    """sp_kv_store on a bf16 and an fp32 pool: the 16-byte path, and the element path of that element size (source rows
    that are not 16-byte aligned)"""
    dtype = torch.float32 if case.startswith("fp32") else torch.bfloat16
    fp = far_pool(dtype, 8, 128, case.endswith("element"), seed=7)
    loc, before = prepare_store(fp)
    T_ = loc.numel()
    g = torch.Generator().manual_seed(3)
    off = 1 if case.endswith("element") else 0     # (rows one element past 16-byte alignment: the element path)
    src = torch.randn(T_, 2048 + 8 * off, generator=g).to(dtype).to(DEV)
    k, v = src[:, off:off + 1024].view(T_, 8, 128), src[:, off + 1024:off + 2048].view(T_, 8, 128)
    nat.kv_store(fp.kb, fp.vb, loc, k, v)
    same = torch.equal(fp.kb[loc], k) and torch.equal(fp.vb[loc], v)
    assert same, f"kv_store {case}: the rows at the slots are not the rows stored"
    after_store(fp, before, 2 * k.numel(), f"kv_store {case}")


def test_kv_store_fp8_beyond_4gib(nat, far_pool):
    fp = far_pool(FP8, 8, 128, True, seed=17)
    loc, before = prepare_store(fp)
    T_ = loc.numel()
    g = torch.Generator().manual_seed(4)
    k = torch.randn(T_, 8, 128, generator=g).to(torch.bfloat16).to(DEV)
    v = torch.randn(T_, 8, 128, generator=g).to(torch.bfloat16).to(DEV)
    nat.kv_store_fp8(fp.kb, fp.vb, loc, k, v, 1.7, 0.37)
    want = lambda x, s: (x / s).to(torch.float8_e5m2).view(torch.uint8)      # pool.py: div_ in the dtype, then cast
    same = torch.equal(fp.kb[loc], want(k, 1.7)) and torch.equal(fp.vb[loc], want(v, 0.37))
    assert same, "kv_store_fp8: the rows at the slots are not the rows stored"
    after_store(fp, before, 2 * k.numel(), "kv_store_fp8")


@pytest.mark.parametrize("neox,rot", [(True, 128), (False, 128), (True, 64), (False, 64)])
def test_rotary_fused_store_beyond_4gib(nat, far_pool, neox, rot):
    """sp_rotary_embedding with the fused K/V store, neox and GPT-J, full and partial rotary_dim (the pass-through tail
    of each row lands at the slot too)"""
    dtype, Hq, Hkv, D = torch.bfloat16, 32, 8, 128
    fp = far_pool(dtype, Hkv, D, not neox, seed=rot + neox)
    loc, before = prepare_store(fp)
    T_ = loc.numel()
    torch.manual_seed(5)
    cache = ops.rope_cos_sin_cache(4096, 500000.0, rot, None, dtype).to(DEV)
    qkv = torch.randn(T_, (Hq + 2 * Hkv) * D, device=DEV).to(dtype)
    q, k, v = qkv.split([Hq * D, Hkv * D, Hkv * D], dim=-1)
    pos = torch.randint(0, 4096, (T_,), device=DEV)
    q0, k0 = q.clone(), k.clone()
    nat.rotary_embedding(pos, q, k, D, cache, neox, value=v, k_buffer=fp.kb, v_buffer=fp.vb, out_cache_loc=loc)
    qr, kr = ops.rotary_embedding(pos.cpu(), q0.cpu(), k0.cpu(), D, cache.cpu(), neox)
    ulp_close(q, qr, dtype, "q")
    ulp_close(k, kr, dtype, "k")
    same_k, same_v = torch.equal(fp.kb[loc].reshape(T_, -1), k), torch.equal(fp.vb[loc].reshape(T_, -1), v)
    assert same_k, "pool K rows != rotated k"
    assert same_v, "pool V rows != v"
    after_store(fp, before, 2 * k.numel(), f"rotary store neox={neox} rotary_dim={rot}")


# ----------------------------------------------------------------------------------- end to end
def serve(kv_cache_dtype, pool_tokens, hold):
    """A 1-layer Llama with Llama-3-8B's kv heads (8 x 128: a 4 KiB token stride in the bf16 arena, 2 KiB in the fp8 one)
    driven as the scheduler drives it: a ragged prefill of three prompts, a second prefill whose cached prefix is the
    first prompt's slots, then three decode steps, each under graph replay and eagerly.  `hold` slots are taken from the
    allocator before anything is scheduled and kept, so that every slot the batches get lies past them.  Returns every
    step's logits and sampled ids (CPU) and the slots the batches were given."""
    from scratchpad_amd.model_runner import ModelConfig, ModelRunner, ServerArgs, TpModelWorker
    from scratchpad_amd.schedule_batch import Req, ScheduleBatch
    cfg = ModelConfig(2048, 1024, 1, 16, 8, 1000, context_len=2048, max_position_embeddings=2048)
    args = ServerArgs(max_total_tokens=pool_tokens, max_running_requests=8, cuda_graph_bs=[4],
                      kv_cache_dtype=kv_cache_dtype)
    mr = ModelRunner(cfg, args, dtype=torch.bfloat16, seed=5)
    mr.init_cuda_graphs()
    assert mr.graph_runner is not None
    alloc = mr.token_to_kv_pool_allocator
    held = alloc.alloc(hold) if hold else None
    worker = TpModelWorker(mr)
    dev = mr.device
    gen = torch.Generator().manual_seed(9)
    prompts = [torch.randint(0, 1000, (n,), generator=gen).tolist() for n in (300, 77, 130)]
    steps, slots = [], []

    def run(name, batch):
        b = batch.get_model_worker_batch()
        out, nxt = worker.forward_batch_generation(b)
        steps.append((name, out.next_token_logits.float().cpu(), nxt.cpu()))
        slots.append(batch.out_cache_loc.cpu())
        return b, nxt

    sb = ScheduleBatch([Req(f"r{i}", "", p, None) for i, p in enumerate(prompts)], mr.req_to_token_pool, alloc,
                       device=dev)
    sb.prepare_for_extend()
    _, nxt = run("ragged prefill", sb)
    prefix = mr.req_to_token_pool.req_to_token[sb.reqs[0].req_pool_idx, :300].to(torch.int64)
    more = torch.randint(0, 1000, (150,), generator=gen).tolist()
    chunk = ScheduleBatch([Req("r3", "", prompts[0] + more, None, prefix_indices=prefix)], mr.req_to_token_pool, alloc,
                          device=dev)
    chunk.prepare_for_extend()
    assert chunk.prefix_lens == [300] and chunk.extend_lens == [150]
    run("prefill behind a cached prefix", chunk)
    sb.output_ids = nxt
    for step in range(3):
        sb.prepare_for_decode()
        b, _ = run(f"decode step {step}, graph replay", sb)
        graphs, mr.graph_runner = mr.graph_runner, None
        out, nxt = worker.forward_batch_generation(b)
        mr.graph_runner = graphs
        steps.append((f"decode step {step}, eager", out.next_token_logits.float().cpu(), nxt.cpu()))
        for r, tok in zip(sb.reqs, sb.input_ids.tolist()):
            r.output_ids.append(tok)
        sb.output_ids = nxt
    tok_bytes = mr.token_to_kv_pool.k_buffer[0].stride(0) * mr.token_to_kv_pool.k_buffer[0].element_size()
    del held
    return steps, slots, tok_bytes


@pytest.mark.parametrize("kv", ["auto", "fp8_e5m2"])
def test_model_runner_serves_beyond_4gib_as_from_a_small_pool(kv):
    """The serving stack at its shipped kernel choices over a pool whose first 4 GiB of slots are held: the same steps
    as a runner of the same seed over a small pool, bit for bit - logits and sampled ids - with every slot of every batch
    lying past 4 GiB of the layer's base.  (The small twin runs first and is freed before the large pool exists.)"""
    _skip_small_device()
    held = 2 ** 20 if kv == "auto" else 2 ** 21          # 4 GiB of 4 KiB (bf16) / 2 KiB (e5m2) token rows
    twin, twin_slots, _ = serve(kv, 4096, 0)
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    far, far_slots, tok_bytes = serve(kv, held + held // 16, held)
    print(f"[far pool] model runner {kv}: peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")
    gc.collect()
    torch.cuda.empty_cache()
    assert tok_bytes * held == 2 ** 32
    for s_twin, s_far in zip(twin_slots, far_slots):
        assert int(s_twin.max()) < 4096 and int(s_far.min()) > held, "the twin's slots are low, the far run's past 4 GiB"
    assert len(far) == len(twin) == 2 + 2 * 3
    for (name, lt, it), (_, lf, i_f) in zip(twin, far):
        assert torch.isfinite(lf).all(), f"{kv} {name}: non-finite logits"
        same_logits, same_ids = torch.equal(lf, lt), torch.equal(i_f, it)
        assert same_logits, f"{kv} {name}: logits differ from the small pool's, max |diff| {float((lf - lt).abs().max()):.3e}"
        assert same_ids, f"{kv} {name}: sampled ids differ"
