"""The penalty / vocab-mask entry points as an integrator binds them (tests/c_header.py: the header alone): the four
prototypes parse into known types, match scratchpad_amd/_native.py's SIGNATURES, are exported, and refuse on the host
- before any launch - what the header says they refuse.  The addition is additive: the ABI version stays 10."""
import ctypes

import pytest

from tests import c_header

NAMES = ("sp_penalty_reset", "sp_penalty_cumulate", "sp_penalty_apply", "sp_vocab_mask_apply")
STATUS = c_header.enum_values("sp_status")
OK, INVALID = STATUS["SP_OK"], STATUS["SP_ERR_INVALID_ARG"]


def test_prototypes_parse_and_match_native_signatures():
    from scratchpad_amd import _native
    protos = c_header.prototypes()
    for name in NAMES:
        assert name in protos, f"{name} is not declared in include/scratchpad_hip.h"
        res, args = protos[name]
        nres, nargs = _native.SIGNATURES[name]
        assert res is ctypes.c_int and nres is res
        assert list(nargs) == [t for _, t in args], name
        assert args[-1][0] == "stream"
    assert [n for n, _ in protos["sp_penalty_apply"][1]][:2] == ["logits", "row_stride"]
    assert c_header.abi_version() == 10


@pytest.fixture(scope="module")
def lib():
    from scratchpad_amd import _native, build
    build.build_native(verbose=False)
    return c_header.bind(_native.lib_path())


@pytest.fixture(scope="module")
def addr():
    buf = (ctypes.c_char * 4096)()
    a = ctypes.addressof(buf)
    yield a + (-a) % 16
    del buf


def test_library_exports_them_and_abi_stays_10(lib):
    for name in NAMES:
        assert hasattr(lib, name)
    assert lib.sp_abi_version() == 10


def _refusals(a):
    return {
        "sp_penalty_reset": (dict(n_distinct=a, out_len=a, pool_row_indices=a, idx64=1, num_rows=3, pool_rows=8,
                                  stream=None),
                             [(dict(n_distinct=None), INVALID), (dict(out_len=None), INVALID),
                              (dict(pool_row_indices=None), INVALID), (dict(num_rows=-3), INVALID),
                              (dict(pool_rows=-8), INVALID), (dict(num_rows=0, n_distinct=None), OK)]),
        "sp_penalty_cumulate": (dict(entries=a, n_distinct=a, out_len=a, error=a, req_pool_indices=a, idx64=1,
                                     token_ids=a, num_rows=3, pool_rows=8, capacity=64, vocab=1000, stream=None),
                                [(dict(entries=None), INVALID), (dict(n_distinct=None), INVALID),
                                 (dict(out_len=None), INVALID), (dict(error=None), INVALID),
                                 (dict(req_pool_indices=None), INVALID), (dict(token_ids=None), INVALID),
                                 (dict(num_rows=-3), INVALID), (dict(pool_rows=-8), INVALID),
                                 (dict(capacity=-64), INVALID), (dict(vocab=-1000), INVALID),
                                 (dict(num_rows=0, entries=None, token_ids=None), OK)]),
        "sp_penalty_apply": (dict(logits=a, row_stride=1030, entries=a, n_distinct=a, out_len=a, req_pool_indices=a,
                                  idx64=0, frequency_penalties=a, presence_penalties=a, repetition_penalties=a,
                                  min_new_tokens=a, stop_token_ids=a, max_stops=3, num_rows=3, pool_rows=8,
                                  capacity=64, vocab=1000, stream=None),
                             [(dict(logits=None), INVALID), (dict(entries=None), INVALID),
                              (dict(n_distinct=None), INVALID), (dict(out_len=None), INVALID),
                              (dict(req_pool_indices=None), INVALID), (dict(frequency_penalties=None), INVALID),
                              (dict(presence_penalties=None), INVALID), (dict(repetition_penalties=None), INVALID),
                              (dict(stop_token_ids=None), INVALID), (dict(min_new_tokens=None), INVALID),
                              (dict(num_rows=-3), INVALID), (dict(vocab=-1000), INVALID),
                              (dict(capacity=-64), INVALID), (dict(pool_rows=-8), INVALID),
                              (dict(max_stops=-3), INVALID), (dict(row_stride=999), INVALID),
                              (dict(num_rows=0, logits=None), OK)]),
        "sp_vocab_mask_apply": (dict(logits=a, row_stride=1030, mask=a, mask_stride=32, mask_width=32, mask_kind=0,
                                     num_rows=3, vocab=1000, stream=None),
                                [(dict(logits=None), INVALID), (dict(mask=None), INVALID),
                                 (dict(num_rows=-3), INVALID), (dict(vocab=-1000), INVALID),
                                 (dict(row_stride=999), INVALID),
                                 (dict(mask_width=33, mask_stride=33), INVALID),       # wider than ceil(1000 / 32)
                                 (dict(mask_width=32, mask_stride=31), INVALID),
                                 (dict(mask_kind=2), INVALID),
                                 (dict(mask_kind=1, mask_width=999, mask_stride=1000), INVALID),   # bool: one per column
                                 (dict(num_rows=0, logits=None, mask=None), OK),
                                 (dict(num_rows=0, mask_width=33, mask_stride=33), INVALID)]),
    }


@pytest.mark.parametrize("name", NAMES)
def test_host_side_refusals(lib, addr, name):
    good, cases = _refusals(addr)[name]
    assert set(good) == {p for p, _ in lib.sp_prototypes[name][1]}
    for override, want in cases:
        got = c_header.call(lib, name, **{**good, **override})
        assert got == want, f"{name}({override}) returned {got}, expected {want}"
