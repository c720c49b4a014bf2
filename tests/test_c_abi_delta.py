"""sp_delta_group and sp_delta_mm as an integrator binds them (tests/c_header.py: the header alone): the prototypes parse
into known types, match scratchpad_amd/_native.py's SIGNATURES, are exported, and refuse on the host - before any launch
- what the header says they refuse.  The additions are additive: the ABI version stays 10.  Only calls that return
before a launch are made."""
import ctypes

import pytest

from tests import c_header

STATUS = c_header.enum_values("sp_status")
OK, INVALID, UNSUPPORTED = STATUS["SP_OK"], STATUS["SP_ERR_INVALID_ARG"], STATUS["SP_ERR_UNSUPPORTED"]
DT = c_header.enum_values("sp_dtype")


def test_prototypes_parse_and_match_native_signatures():
    from scratchpad_amd import _native
    protos = c_header.prototypes()
    assert c_header.abi_version() == 10
    assert "sp_delta_group" in protos and "sp_delta_mm" in protos, "not declared in include/scratchpad_hip.h"
    assert [n for n, _ in protos["sp_delta_group"][1]] == [
        "slot_offsets", "sorted_rows", "indices", "num_tokens", "num_slots", "stream"]
    assert [n for n, _ in protos["sp_delta_mm"][1]] == [
        "y", "x", "codes", "meta", "scales", "slot_offsets", "sorted_rows", "num_tokens", "num_slots", "N", "K",
        "x_stride", "y_stride", "codes_slot_stride", "meta_slot_stride", "scales_slot_stride", "dtype", "stream"]
    for name in ("sp_delta_group", "sp_delta_mm"):
        res, args = protos[name]
        assert res is ctypes.c_int
        assert _native.SIGNATURES[name] == (res, [t for _, t in args])
        assert "batch_size" not in [n for n, _ in args]
    assert set(_native.DELTA_CALLS) == {"group", "mm"}


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
    assert hasattr(lib, "sp_delta_group") and hasattr(lib, "sp_delta_mm")
    assert lib.sp_abi_version() == 10


def test_group_refuses_on_the_host(lib, addr):
    a = addr
    good = dict(slot_offsets=a, sorted_rows=a, indices=a, num_tokens=70, num_slots=3, stream=None)
    assert set(good) == {p for p, _ in lib.sp_prototypes["sp_delta_group"][1]}
    call = lambda **kw: c_header.call(lib, "sp_delta_group", **{**good, **kw})
    for p in ("slot_offsets", "sorted_rows", "indices"):
        assert call(**{p: None}) == INVALID, p
    assert call(num_tokens=-70) == INVALID and call(num_slots=-3) == INVALID
    assert call(num_slots=0) == UNSUPPORTED and call(num_slots=65) == UNSUPPORTED
    assert call(num_tokens=16385) == UNSUPPORTED


def test_mm_refuses_on_the_host(lib, addr):
    a = addr
    N, K = 48, 320
    good = dict(y=a, x=a, codes=a, meta=a, scales=a, slot_offsets=a, sorted_rows=a, num_tokens=70, num_slots=3, N=N,
                K=K, x_stride=K + 8, y_stride=N + 4, codes_slot_stride=N * K // 4 + 16, meta_slot_stride=N * K // 8 + 8,
                scales_slot_stride=N + 1, dtype=DT["SP_BF16"], stream=None)
    assert set(good) == {p for p, _ in lib.sp_prototypes["sp_delta_mm"][1]}
    call = lambda **kw: c_header.call(lib, "sp_delta_mm", **{**good, **kw})
    for p in ("y", "x", "codes", "meta", "scales", "slot_offsets", "sorted_rows"):
        assert call(**{p: None}) == INVALID, p
    for p in ("num_tokens", "num_slots", "N", "K"):
        assert call(**{p: -good[p]}) == INVALID, p
    assert call(num_tokens=0) == OK, "num_tokens == 0 is SP_OK without a launch"
    assert call(num_tokens=0, dtype=DT["SP_F32"]) == OK
    for dt in ("SP_F32", "SP_FP8_E5M2"):
        assert call(dtype=DT[dt]) == UNSUPPORTED, dt
    assert call(dtype=7) == UNSUPPORTED
    assert call(num_slots=0) == UNSUPPORTED and call(num_slots=65) == UNSUPPORTED
    assert call(num_tokens=16385) == UNSUPPORTED
    for k in (0, 32, 96, 328):
        assert call(K=k, x_stride=4096) == UNSUPPORTED, k
    for n in (0, 8, 40):
        assert call(N=n) == UNSUPPORTED, n
    # strides below the width they span
    assert call(x_stride=K - 8) == INVALID and call(x_stride=-(K + 8)) == INVALID
    assert call(y_stride=N - 1) == INVALID
    assert call(codes_slot_stride=N * K // 4 - 16) == INVALID
    assert call(meta_slot_stride=N * K // 8 - 8) == INVALID
    assert call(scales_slot_stride=N - 1) == INVALID
    # bases and strides that break the vector widths read: 16 B of x and codes, 8 B of meta, 2 B of y and scales
    assert call(x=a + 8) == INVALID and call(x_stride=K + 4) == INVALID
    assert call(codes=a + 8) == INVALID and call(codes_slot_stride=N * K // 4 + 8) == INVALID
    assert call(meta=a + 4) == INVALID and call(meta_slot_stride=N * K // 8 + 4) == INVALID
    assert call(y=a + 1) == INVALID and call(scales=a + 1) == INVALID
