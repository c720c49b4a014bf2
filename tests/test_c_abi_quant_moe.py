"""sp_qmoe_gate_up, sp_qmoe_down and sp_qmoe_combine as an integrator binds them (tests/c_header.py: the header alone):
the prototypes parse into known types, match scratchpad_amd/_native.py's SIGNATURES, are exported, and refuse on the
host - before any launch - what the header says they refuse.  The additions are additive: the ABI version stays 10.
Only calls that return before a launch are made."""
import ctypes

import pytest

from tests import c_header

STATUS = c_header.enum_values("sp_status")
OK, INVALID, UNSUPPORTED = STATUS["SP_OK"], STATUS["SP_ERR_INVALID_ARG"], STATUS["SP_ERR_UNSUPPORTED"]
DT = c_header.enum_values("sp_dtype")
ENTRIES = ("sp_qmoe_gate_up", "sp_qmoe_down", "sp_qmoe_combine")
H, I, E, K, T = 128, 64, 4, 2, 5


def test_prototypes_parse_and_match_native_signatures():
    from scratchpad_amd import _native
    protos = c_header.prototypes()
    assert c_header.abi_version() == 10
    for name in ENTRIES + ("sp_qmoe_weight_tiles",):
        assert name in protos, f"{name} is not declared in include/scratchpad_hip.h"
        res, args = protos[name]
        assert res is ctypes.c_int
        assert _native.SIGNATURES[name] == (res, [t for _, t in args])
        assert "batch_size" not in [n for n, _ in args]
    assert [n for n, _ in protos["sp_qmoe_gate_up"][1]] == [
        "h", "x", "codes", "meta", "scales", "expert_offsets", "sorted_pos", "num_tokens", "top_k", "num_experts",
        "hidden", "inter", "x_stride", "h_stride", "codes_expert_stride", "meta_expert_stride", "scales_expert_stride",
        "dtype", "stream"]
    assert [n for n, _ in protos["sp_qmoe_down"][1]] == [
        "tmp", "h", "codes", "meta", "scales", "topk_weights", "expert_offsets", "sorted_pos", "num_tokens", "top_k",
        "num_experts", "hidden", "inter", "h_stride", "tmp_stride", "codes_expert_stride", "meta_expert_stride",
        "scales_expert_stride", "dtype", "stream"]
    assert [n for n, _ in protos["sp_qmoe_combine"][1]] == [
        "out", "tmp", "base", "topk_ids", "num_tokens", "top_k", "num_experts", "hidden", "tmp_stride", "base_stride",
        "out_stride", "order", "dtype", "stream"]
    assert set(_native.QMOE_CALLS) == {"gate_up", "down", "combine"}


@pytest.fixture(scope="module")
def lib():
    from scratchpad_amd import _native, build
    build.build_native(verbose=False)
    return c_header.bind(_native.lib_path())


@pytest.fixture(scope="module")
def addr():
    """a 16-byte-aligned HOST address standing for every non-NULL buffer: no call below reaches a launch"""
    buf = (ctypes.c_char * 4096)()
    a = ctypes.addressof(buf)
    yield a + (-a) % 16
    del buf


def test_library_exports_them_and_abi_stays_10(lib):
    assert all(hasattr(lib, name) for name in ENTRIES)
    assert lib.sp_abi_version() == 10
    assert lib.sp_qmoe_weight_tiles() in (1, 2, 4)


def shared_refusals(call, good, pointers, sizes):
    """what the three entries refuse alike"""
    for p in pointers:
        assert call(**{p: None}) == INVALID, p
    for p in sizes:
        assert call(**{p: -good[p]}) == INVALID, p
    assert call(num_tokens=0) == OK, "num_tokens == 0 is SP_OK without a launch"
    assert call(num_tokens=0, dtype=DT["SP_F32"]) == OK
    for dt in ("SP_F32", "SP_FP8_E5M2"):
        assert call(dtype=DT[dt]) == UNSUPPORTED, dt
    assert call(dtype=7) == UNSUPPORTED
    assert call(num_experts=0) == UNSUPPORTED and call(num_experts=65) == UNSUPPORTED
    assert call(top_k=0) == UNSUPPORTED and call(top_k=9, num_experts=16) == UNSUPPORTED
    assert call(top_k=E + 1) == UNSUPPORTED, "top_k > num_experts"
    assert call(num_tokens=16385) == UNSUPPORTED


def test_gate_up_refuses_on_the_host(lib, addr):
    a = addr
    N = 2 * I
    good = dict(h=a, x=a, codes=a, meta=a, scales=a, expert_offsets=a, sorted_pos=a, num_tokens=T, top_k=K,
                num_experts=E, hidden=H, inter=I, x_stride=H + 8, h_stride=I + 8,
                codes_expert_stride=N * H // 4 + 16, meta_expert_stride=N * H // 8 + 8, scales_expert_stride=N + 1,
                dtype=DT["SP_BF16"], stream=None)
    assert set(good) == {p for p, _ in lib.sp_prototypes["sp_qmoe_gate_up"][1]}
    call = lambda **kw: c_header.call(lib, "sp_qmoe_gate_up", **{**good, **kw})
    shared_refusals(call, good, ("h", "x", "codes", "meta", "scales", "expert_offsets", "sorted_pos"),
                    ("num_tokens", "top_k", "num_experts", "hidden", "inter"))
    for v in (0, 32, 96, 136):
        assert call(hidden=v, x_stride=4096, codes_expert_stride=1 << 20, meta_expert_stride=1 << 20) == UNSUPPORTED, v
        assert call(inter=v, h_stride=4096, codes_expert_stride=1 << 20, meta_expert_stride=1 << 20,
                    scales_expert_stride=4096) == UNSUPPORTED, v
    # strides below the width they span
    assert call(x_stride=H - 8) == INVALID and call(x_stride=-(H + 8)) == INVALID
    assert call(h_stride=I - 8) == INVALID
    assert call(codes_expert_stride=N * H // 4 - 16) == INVALID
    assert call(meta_expert_stride=N * H // 8 - 8) == INVALID
    assert call(scales_expert_stride=N - 1) == INVALID
    # bases and strides that break the vector widths read
    assert call(x=a + 8) == INVALID and call(x_stride=H + 4) == INVALID
    assert call(h=a + 8) == INVALID and call(h_stride=I + 4) == INVALID
    assert call(codes=a + 8) == INVALID and call(codes_expert_stride=N * H // 4 + 8) == INVALID
    assert call(meta=a + 4) == INVALID and call(meta_expert_stride=N * H // 8 + 4) == INVALID
    assert call(scales=a + 1) == INVALID
    # more than 65535 grid.y blocks
    big = 8 * lib.sp_qmoe_weight_tiles() * 65536
    assert call(inter=big, h_stride=big, codes_expert_stride=1 << 40, meta_expert_stride=1 << 40,
                scales_expert_stride=2 * big) == INVALID


def test_down_refuses_on_the_host(lib, addr):
    a = addr
    good = dict(tmp=a, h=a, codes=a, meta=a, scales=a, topk_weights=a, expert_offsets=a, sorted_pos=a, num_tokens=T,
                top_k=K, num_experts=E, hidden=H, inter=I, h_stride=I + 8, tmp_stride=H + 8,
                codes_expert_stride=H * I // 4 + 16, meta_expert_stride=H * I // 8 + 8, scales_expert_stride=H + 1,
                dtype=DT["SP_F16"], stream=None)
    assert set(good) == {p for p, _ in lib.sp_prototypes["sp_qmoe_down"][1]}
    call = lambda **kw: c_header.call(lib, "sp_qmoe_down", **{**good, **kw})
    shared_refusals(call, good, ("tmp", "h", "codes", "meta", "scales", "topk_weights", "expert_offsets", "sorted_pos"),
                    ("num_tokens", "top_k", "num_experts", "hidden", "inter"))
    for v in (0, 32, 96, 136):
        assert call(hidden=v, tmp_stride=4096, codes_expert_stride=1 << 20, meta_expert_stride=1 << 20,
                    scales_expert_stride=4096) == UNSUPPORTED, v
        assert call(inter=v, h_stride=4096, codes_expert_stride=1 << 20, meta_expert_stride=1 << 20) == UNSUPPORTED, v
    assert call(h_stride=I - 8) == INVALID and call(tmp_stride=H - 8) == INVALID and call(tmp_stride=-(H + 8)) == INVALID
    assert call(codes_expert_stride=H * I // 4 - 16) == INVALID
    assert call(meta_expert_stride=H * I // 8 - 8) == INVALID
    assert call(scales_expert_stride=H - 1) == INVALID
    assert call(h=a + 8) == INVALID and call(h_stride=I + 4) == INVALID
    assert call(tmp=a + 8) == INVALID and call(tmp_stride=H + 4) == INVALID
    assert call(codes=a + 8) == INVALID and call(codes_expert_stride=H * I // 4 + 8) == INVALID
    assert call(meta=a + 4) == INVALID and call(meta_expert_stride=H * I // 8 + 4) == INVALID
    assert call(scales=a + 1) == INVALID
    big = 16 * lib.sp_qmoe_weight_tiles() * 65536
    assert call(hidden=big, tmp_stride=big, codes_expert_stride=1 << 40, meta_expert_stride=1 << 40,
                scales_expert_stride=big) == INVALID


def test_combine_refuses_on_the_host(lib, addr):
    a = addr
    good = dict(out=a, tmp=a, base=a, topk_ids=a, num_tokens=T, top_k=K, num_experts=E, hidden=H, tmp_stride=H + 8,
                base_stride=H + 16, out_stride=H, order=1, dtype=DT["SP_BF16"], stream=None)
    assert set(good) == {p for p, _ in lib.sp_prototypes["sp_qmoe_combine"][1]}
    call = lambda **kw: c_header.call(lib, "sp_qmoe_combine", **{**good, **kw})
    shared_refusals(call, good, ("out", "tmp", "base", "topk_ids"), ("num_tokens", "top_k", "num_experts", "hidden"))
    for v in (0, 32, 96, 136):
        assert call(hidden=v, tmp_stride=4096, base_stride=4096, out_stride=4096) == UNSUPPORTED, v
    for order in (-1, 2, 7):
        assert call(order=order) == UNSUPPORTED, order
    for p in ("tmp_stride", "base_stride", "out_stride"):
        assert call(**{p: H - 8}) == INVALID and call(**{p: H + 4}) == INVALID, p
    for p in ("out", "tmp", "base"):
        assert call(**{p: a + 8}) == INVALID, p
