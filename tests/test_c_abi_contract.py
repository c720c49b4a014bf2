"""CPU checks of the C ABI as an integrator binds it (tests/c_header.py: the header alone).

* scratchpad_amd/_native.py's SIGNATURES carry the header's types, argument for argument;
* INTEGRATION.md's binding stub (section 1) and its decode call (section 3) agree with the header;
* every compute entry point refuses, on the host, the calls the header says it refuses - a NULL required
  pointer or a negative size (SP_ERR_INVALID_ARG), a workspace or plan one byte short (SP_ERR_WORKSPACE),
  a shape that is not built (SP_ERR_UNSUPPORTED).  Only calls that return before any launch are made here."""
import ast
import ctypes
import os
import re

import pytest

from tests import c_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATUS = c_header.enum_values("sp_status")
OK, INVALID, UNSUPPORTED, WORKSPACE = (STATUS[k] for k in ("SP_OK", "SP_ERR_INVALID_ARG", "SP_ERR_UNSUPPORTED",
                                                            "SP_ERR_WORKSPACE"))
DT = c_header.enum_values("sp_dtype")


def test_header_parses_into_known_types():
    protos = c_header.prototypes()
    assert len(protos) >= 40
    assert c_header.abi_version() == 10
    assert DT == {"SP_F32": 0, "SP_F16": 1, "SP_BF16": 2, "SP_FP8_E5M2": 3}
    assert STATUS == {"SP_OK": 0, "SP_ERR_INVALID_ARG": -1, "SP_ERR_UNSUPPORTED": -2, "SP_ERR_WORKSPACE": -3,
                      "SP_ERR_LAUNCH": -4}
    res, args = protos["sp_decode_attention"]
    assert res is ctypes.c_int and len(args) == 32
    assert [n for n, _ in args[27:30]] == ["plan", "plan_bytes", "dtype"]
    assert args[28][1] is ctypes.c_size_t
    with pytest.raises(ValueError):
        c_header.ctype_of("double")
    with pytest.raises(ValueError):
        c_header.ctype_of("const short*")


def test_native_signatures_match_the_header():
    from scratchpad_amd import _native
    protos = c_header.prototypes()
    assert sorted(_native.SIGNATURES) == sorted(protos)
    bad = []
    for name, (res, args) in protos.items():
        nres, nargs = _native.SIGNATURES[name]
        want = [t for _, t in args]
        if nres is not res or list(nargs) != want:
            bad.append(f"{name}: _native ({nres.__name__}, {[t.__name__ for t in nargs]}) != header "
                       f"({res.__name__}, {[t.__name__ for t in want]})")
    assert not bad, "\n".join(bad)


def _section(text: str, number: str) -> str:
    m = re.search(r"^## " + re.escape(number) + r"\. .*?(?=^## )", text, flags=re.M | re.S)
    assert m, f"INTEGRATION.md has no section {number}"
    return m.group(0)


def _call_text(section: str, fn: str) -> str:
    """The source of the call `fn(...)` in `section` (balanced parentheses, '#' comments dropped)."""
    start = section.index(fn + "(")
    depth, i = 0, start + len(fn)
    while True:
        c = section[i]
        depth += c == "("
        depth -= c == ")"
        i += 1
        if depth == 0:
            break
    return "\n".join(line.split("#")[0] for line in section[start:i].splitlines())


def test_integration_md_binds_the_header():
    """INTEGRATION.md 1 is the binding an integrator copies: every argtypes line it shows, the ABI version it asserts,
    and the positional decode call of section 3 must agree with include/scratchpad_hip.h."""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    protos = c_header.prototypes()
    s1 = _section(text, "1")
    ns = {"_vp": ctypes.c_void_p, "_i64": ctypes.c_int64, "_i32": ctypes.c_int, "_f32": ctypes.c_float,
          "_sz": ctypes.c_size_t}
    alias = re.search(r"^_vp, _i64, _i32, _f32, _sz = (.*)$", s1, flags=re.M)
    assert alias, "section 1 no longer defines the _vp/_i64/_i32/_f32/_sz aliases"
    assert eval(alias.group(1), {"ctypes": ctypes}) == tuple(ns.values())
    errors = []
    lines = re.findall(r"^_lib\.(sp_\w+)\.argtypes = ([^#\n]*)", s1, flags=re.M)
    assert lines, "section 1 shows no argtypes line"
    for name, expr in lines:
        got = eval(expr, dict(ns))
        want = [t for _, t in protos[name][1]]
        if got != want:
            errors.append(f"{name}.argtypes: {len(got)} types {[t.__name__ for t in got]} != the header's {len(want)} "
                          f"{[t.__name__ for t in want]}")
    v = re.search(r"^assert _lib\.sp_abi_version\(\) == (\d+)", s1, flags=re.M)
    assert v, "section 1 asserts no ABI version"
    if int(v.group(1)) != c_header.abi_version():
        errors.append(f"sp_abi_version: section 1 asserts {v.group(1)}, the header is at {c_header.abi_version()}")
    call = ast.parse(_call_text(_section(text, "3"), "_lib.sp_decode_attention"), mode="eval").body
    assert not call.keywords
    if len(call.args) != len(protos["sp_decode_attention"][1]):
        errors.append(f"sp_decode_attention call in section 3: {len(call.args)} arguments, the header has "
                      f"{len(protos['sp_decode_attention'][1])}")
    assert not errors, "\n".join(errors)


# --------------------------------------------------------------------------- host-side return codes
@pytest.fixture(scope="module")
def lib():
    from scratchpad_amd import _native, build
    build.build_native(verbose=False)
    return c_header.bind(_native.lib_path())


@pytest.fixture(scope="module")
def addr():
    """a 16-byte-aligned host address standing for every non-NULL buffer: no call below reaches a launch"""
    buf = (ctypes.c_char * 4096)()
    a = ctypes.addressof(buf)
    yield a + (-a) % 16
    del buf


def _refusals(a):
    """entry point -> (good keyword arguments of a call that would launch, [(override, expected status)]).
    Every override makes the call return on the host: a NULL required pointer, a negative size, ..."""
    return {
        "sp_rmsnorm": (dict(out=a, x=a, weight=a, num_tokens=4, hidden=64, x_stride=72, out_stride=80, eps=1e-5,
                            dtype=DT["SP_BF16"], stream=None),
                       [(dict(out=None), INVALID), (dict(x=None), INVALID), (dict(weight=None), INVALID),
                        (dict(num_tokens=-1), INVALID), (dict(hidden=-64), INVALID)]),
        "sp_fused_add_rmsnorm": (dict(x=a, residual=a, weight=a, num_tokens=4, hidden=64, x_stride=72, res_stride=88,
                                      eps=1e-5, dtype=DT["SP_BF16"], stream=None),
                                 [(dict(x=None), INVALID), (dict(residual=None), INVALID), (dict(weight=None), INVALID),
                                  (dict(num_tokens=-1), INVALID), (dict(hidden=-1), INVALID)]),
        "sp_silu_and_mul": (dict(out=a, x=a, num_tokens=3, d=64, x_stride=136, out_stride=72, dtype=DT["SP_F16"],
                                 stream=None),
                            [(dict(out=None), INVALID), (dict(x=None), INVALID), (dict(num_tokens=-3), INVALID),
                             (dict(d=-64), INVALID)]),
        "sp_rotary_embedding": (dict(positions=a, q=a, k=a, cos_sin_cache=a, num_tokens=5, num_q_heads=4, num_kv_heads=2,
                                     head_size=64, rotary_dim=32, q_stride=280, k_stride=152, is_neox=1, v=a,
                                     v_stride=168, k_buffer=a, v_buffer=a, out_cache_loc=a, kv_buffer_stride=136,
                                     dtype=DT["SP_BF16"], stream=None),
                                [(dict(positions=None), INVALID), (dict(q=None), INVALID), (dict(k=None), INVALID),
                                 (dict(cos_sin_cache=None), INVALID), (dict(v=None), INVALID),
                                 (dict(v_buffer=None), INVALID), (dict(out_cache_loc=None), INVALID),
                                 (dict(num_tokens=-5), INVALID), (dict(num_q_heads=-4), INVALID),
                                 (dict(head_size=-64), INVALID), (dict(rotary_dim=-32), INVALID),
                                 (dict(rotary_dim=66), INVALID), (dict(kv_buffer_stride=-136), INVALID)]),
        "sp_kv_store": (dict(k_buffer=a, v_buffer=a, loc=a, k=a, v=a, num_tokens=3, num_kv_heads=2, head_dim=64,
                             v_head_dim=32, k_stride=152, v_stride=80, k_buffer_stride=136, v_buffer_stride=72,
                             dtype=DT["SP_F16"], stream=None),
                        [(dict(k_buffer=None), INVALID), (dict(v_buffer=None), INVALID), (dict(loc=None), INVALID),
                         (dict(k=None), INVALID), (dict(v=None), INVALID), (dict(num_tokens=-3), INVALID),
                         (dict(num_kv_heads=-2), INVALID), (dict(head_dim=-64), INVALID),
                         (dict(v_head_dim=-32), INVALID), (dict(dtype=DT["SP_FP8_E5M2"]), UNSUPPORTED)]),
        "sp_kv_store_fp8": (dict(k_buffer=a, v_buffer=a, loc=a, k=a, v=a, num_tokens=3, num_kv_heads=2, head_dim=64,
                                 k_stride=152, v_stride=168, k_buffer_stride=136, v_buffer_stride=144, k_scale=1.5,
                                 v_scale=0.5, src_dtype=DT["SP_BF16"], stream=None),
                            [(dict(k_buffer=None), INVALID), (dict(v_buffer=None), INVALID), (dict(loc=None), INVALID),
                             (dict(k=None), INVALID), (dict(v=None), INVALID), (dict(num_tokens=-3), INVALID),
                             (dict(num_kv_heads=-2), INVALID), (dict(head_dim=-64), INVALID),
                             (dict(k_scale=0.0), INVALID), (dict(v_scale=-1.0), INVALID),
                             (dict(k_buffer_stride=140), UNSUPPORTED)]),
        "sp_write_req_to_token": (dict(req_to_token=a, row_stride=37, req_pool_indices=a, pre_lens=a, seq_lens=a,
                                       extend_lens=a, out_cache_loc=a, batch_size=3, stream=None),
                                  [(dict(req_to_token=None), INVALID), (dict(req_pool_indices=None), INVALID),
                                   (dict(pre_lens=None), INVALID), (dict(seq_lens=None), INVALID),
                                   (dict(extend_lens=None), INVALID), (dict(out_cache_loc=None), INVALID),
                                   (dict(batch_size=-3), INVALID), (dict(row_stride=-37), INVALID)]),
        "sp_compute_position": (dict(positions=a, extend_start_loc=a, extend_prefix_lens=a, extend_seq_lens=a,
                                     batch_size=3, stream=None),
                                [(dict(positions=None), INVALID), (dict(extend_start_loc=None), INVALID),
                                 (dict(extend_prefix_lens=None), INVALID), (dict(extend_seq_lens=None), INVALID),
                                 (dict(batch_size=-3), INVALID)]),
        "sp_clamp_position": (dict(positions=a, seq_lens=a, idx64=1, batch_size=3, stream=None),
                              [(dict(positions=None), INVALID), (dict(seq_lens=None), INVALID),
                               (dict(batch_size=-3), INVALID)]),
        "sp_argmax": (dict(logits=a, row_stride=1030, batch_size=3, vocab=1000, out_ids=a, dtype=DT["SP_F32"],
                           stream=None),
                      [(dict(logits=None), INVALID), (dict(out_ids=None), INVALID), (dict(batch_size=-3), INVALID),
                       (dict(vocab=-1000), INVALID), (dict(row_stride=999), INVALID)]),
        "sp_argmax_shard": (dict(logits=a, row_stride=530, batch_size=3, cols=500, index_offset=500, out_pairs=a,
                                 dtype=DT["SP_BF16"], stream=None),
                            [(dict(logits=None), INVALID), (dict(out_pairs=None), INVALID),
                             (dict(batch_size=-3), INVALID), (dict(cols=-500), INVALID),
                             (dict(index_offset=-1), INVALID), (dict(row_stride=499), INVALID)]),
        "sp_argmax_merge": (dict(pairs=a, num_shards=2, batch_size=3, out_ids=a, stream=None),
                            [(dict(pairs=None), INVALID), (dict(out_ids=None), INVALID),
                             (dict(batch_size=-3), INVALID), (dict(num_shards=-2), INVALID)]),
        "sp_softmax_temperature": (dict(logits_inout=a, row_stride=1030, temperatures=a, batch_size=3, vocab=1000,
                                        stream=None),
                                   [(dict(logits_inout=None), INVALID), (dict(batch_size=-3), INVALID),
                                    (dict(vocab=-1000), INVALID), (dict(row_stride=999), INVALID)]),
        "sp_top_k_top_p_min_p_sample": (dict(probs=a, row_stride=1030, top_ks=a, top_ps=a, min_ps=a, uniform=a,
                                             batch_size=3, vocab=1000, out_ids=a, keep_count=a, stream=None),
                                        [(dict(probs=None), INVALID), (dict(uniform=None), INVALID),
                                         (dict(out_ids=None), INVALID), (dict(batch_size=-3), INVALID),
                                         (dict(vocab=-1000), INVALID), (dict(row_stride=999), INVALID)]),
        "sp_top_k_top_p_min_p_renorm": (dict(probs=a, row_stride=1030, top_ks=a, top_ps=a, min_ps=a, batch_size=3,
                                             vocab=1000, out=a, out_stride=1010, keep_count=a, stream=None),
                                        [(dict(probs=None), INVALID), (dict(out=None), INVALID),
                                         (dict(batch_size=-3), INVALID), (dict(vocab=-1000), INVALID),
                                         (dict(row_stride=999), INVALID), (dict(out_stride=999), INVALID)]),
        "sp_gemm_skinny": (dict(out=a, x=a, w=a, M=4, N=64, K=128, x_stride=136, w_stride=144, out_stride=72,
                                epilogue=0, dtype=DT["SP_BF16"], stream=None),
                           [(dict(out=None), INVALID), (dict(x=None), INVALID), (dict(w=None), INVALID),
                            (dict(M=-4), INVALID), (dict(N=-64), INVALID), (dict(K=-128), INVALID),
                            (dict(epilogue=2), INVALID), (dict(M=17), UNSUPPORTED), (dict(K=100), UNSUPPORTED),
                            (dict(dtype=DT["SP_F32"]), UNSUPPORTED), (dict(x_stride=132), INVALID)]),
    }


@pytest.mark.parametrize("name", sorted(_refusals(0)))
def test_host_side_refusals(lib, addr, name):
    good, cases = _refusals(addr)[name]
    assert set(good) == {p for p, _ in lib.sp_prototypes[name][1]}
    for override, want in cases:
        got = c_header.call(lib, name, **{**good, **override})
        assert got == want, f"{name}({override}) returned {got}, expected {want}"


def _decode_args(a, lib, **kw):
    """a plan-less decode launch of 3 requests over 2 splits (max_seq_len 100, chunk 64), workspace sized exactly"""
    args = dict(out=a, q=a, k_buffer=a, v_buffer=a, req_to_token=a, req_to_token_stride=131, req_pool_indices=a,
                seq_lens=a, kv_start=None, idx64=0, batch_size=3, num_q_heads=8, num_kv_heads=2, head_dim=64,
                q_stride=1536, out_stride=520, kv_buffer_stride=136, sm_scale=0.125, logit_cap=0.0, k_scale=1.25,
                v_scale=0.75, max_seq_len=100, chunk=64, max_slots=0, ranges=0, workspace=a,
                workspace_bytes=c_header.call(lib, "sp_decode_attention_workspace_bytes", max_slots=6, num_q_heads=8,
                                              v_head_dim=64),
                plan=None, plan_bytes=0, dtype=DT["SP_BF16"], kv_dtype=DT["SP_BF16"], stream=None)
    args.update(kw)
    return args


def test_decode_refusals(lib, addr):
    a = addr
    call = lambda **kw: c_header.call(lib, "sp_decode_attention", **_decode_args(a, lib, **kw))
    ws = _decode_args(a, lib)["workspace_bytes"]
    assert ws == 6 * 8 * 65 * 4 + 16
    for p in ("out", "q", "k_buffer", "v_buffer", "req_to_token", "req_pool_indices", "seq_lens"):
        assert call(**{p: None}) == INVALID, p
    for k in ("batch_size", "num_q_heads", "num_kv_heads", "head_dim", "max_seq_len"):
        assert call(**{k: -1}) == INVALID, k
    assert call(k_scale=0.0) == INVALID and call(v_scale=-1.0) == INVALID
    assert call(workspace_bytes=ws - 1) == WORKSPACE
    assert call(workspace=None) == WORKSPACE
    assert call(head_dim=96) == UNSUPPORTED
    assert call(dtype=DT["SP_F32"], kv_dtype=DT["SP_FP8_E5M2"]) == UNSUPPORTED
    # the kernels form a key's address as base + slot * token stride with the stride held in 32 bits: a token stride
    # of 2^32 bytes or more is refused (bf16: the stride is in elements, the byte pool's in bytes)
    assert call(kv_buffer_stride=2 ** 31) == INVALID
    assert call(kv_buffer_stride=2 ** 32, kv_dtype=DT["SP_FP8_E5M2"]) == INVALID
    # a plan one byte short of sp_decode_plan_bytes(batch_size, max_slots, ranges), for each kind of plan
    for slots, ranges in ((6, 0), (6, 32), (0, 32)):
        need = c_header.call(lib, "sp_decode_plan_bytes", batch_size=3, max_slots=slots, ranges=ranges)
        assert call(plan=a, plan_bytes=need - 1, max_slots=slots, ranges=ranges) == WORKSPACE, (slots, ranges)
    assert call(plan=a, plan_bytes=1 << 20, max_slots=0, ranges=0) == INVALID     # a plan with neither section


def test_decode_plan_refusals(lib, addr):
    a = addr
    need = c_header.call(lib, "sp_decode_plan_bytes", batch_size=3, max_slots=6, ranges=32)
    assert need == (4 + 3 + 2 * 6 + 4 + 4 + 32) * 4
    good = dict(plan=a, plan_bytes=need, seq_lens=a, idx64=1, batch_size=3, max_seq_len=100, chunk=64, max_slots=6,
                ranges=32, stream=None)
    call = lambda **kw: c_header.call(lib, "sp_decode_plan", **{**good, **kw})
    assert call(plan=None) == INVALID and call(seq_lens=None) == INVALID
    for k in ("batch_size", "max_seq_len", "max_slots", "ranges", "chunk"):
        assert call(**{k: -1}) == INVALID, k
    assert call(plan_bytes=need - 1) == WORKSPACE
    assert call(max_slots=0, ranges=0) == INVALID
    # ABI 10: an item plan has room for one item per request (the plan kernel's split size can always reach that)
    assert call(max_slots=2) == INVALID and call(max_slots=2, ranges=0) == INVALID
    assert call(max_seq_len=(1 << 30) + 1, ranges=0) == INVALID


def test_extend_refusals(lib, addr):
    a = addr
    T_, bs, Hq, Hkv = 40, 3, 8, 2
    wsb = c_header.call(lib, "sp_extend_attention_workspace_bytes", num_tokens=T_, batch_size=bs, num_q_heads=Hq,
                        head_dim=64, dtype=DT["SP_F16"])
    pb = c_header.call(lib, "sp_extend_plan_bytes", num_tokens=T_, batch_size=bs, num_q_heads=Hq, num_kv_heads=Hkv)
    good = dict(out=a, q=a, k_buffer=a, v_buffer=a, req_to_token=a, req_to_token_stride=131, req_pool_indices=a,
                seq_lens=a, kv_start=a, idx64=0, extend_seq_lens=a, extend_start_loc=a, batch_size=bs, num_tokens=T_,
                num_q_heads=Hq, num_kv_heads=Hkv, head_dim=64, q_stride=536, out_stride=528, kv_buffer_stride=136,
                sm_scale=0.125, logit_cap=0.0, k_scale=1.25, v_scale=0.75, causal=1, window_left=-1,
                max_extend_len=20, max_seq_len=100, workspace=a, workspace_bytes=wsb, plan=a, plan_bytes=pb,
                dtype=DT["SP_F16"], kv_dtype=DT["SP_F16"], stream=None)
    call = lambda **kw: c_header.call(lib, "sp_extend_attention", **{**good, **kw})
    for p in ("out", "q", "k_buffer", "v_buffer", "req_to_token", "req_pool_indices", "seq_lens", "extend_seq_lens",
              "extend_start_loc"):
        assert call(**{p: None}) == INVALID, p
    for k in ("batch_size", "num_tokens", "num_q_heads", "num_kv_heads", "max_extend_len", "max_seq_len"):
        assert call(**{k: -1}) == INVALID, k
    assert call(k_scale=0.0) == INVALID
    assert call(workspace_bytes=wsb - 1) == WORKSPACE and call(workspace=None) == WORKSPACE
    assert call(plan_bytes=pb - 1) == WORKSPACE
    assert call(head_dim=80) == UNSUPPORTED
    assert call(dtype=DT["SP_F32"], kv_dtype=DT["SP_FP8_E5M2"]) == UNSUPPORTED
    plan_good = dict(plan=a, plan_bytes=pb, extend_seq_lens=a, seq_lens=a, idx64=0, batch_size=bs, num_tokens=T_,
                     num_q_heads=Hq, num_kv_heads=Hkv, causal=1, stream=None)
    pcall = lambda **kw: c_header.call(lib, "sp_extend_plan", **{**plan_good, **kw})
    for p in ("plan", "extend_seq_lens", "seq_lens"):
        assert pcall(**{p: None}) == INVALID, p
    for k in ("batch_size", "num_tokens", "num_q_heads", "num_kv_heads"):
        assert pcall(**{k: -1}) == INVALID, k
    assert pcall(plan_bytes=pb - 1) == WORKSPACE


def test_call_spells_out_every_parameter(lib):
    with pytest.raises(TypeError, match="missing"):
        c_header.call(lib, "sp_argmax_merge", pairs=None, num_shards=1, batch_size=0, stream=None)
    with pytest.raises(TypeError, match="unknown"):
        c_header.call(lib, "sp_argmax_merge", pairs=None, num_shards=1, batch_size=0, out_ids=None, stream=None,
                      row_stride=4)
    assert c_header.call(lib, "sp_argmax_merge", pairs=None, num_shards=1, batch_size=0, out_ids=None,
                         stream=None) == OK
