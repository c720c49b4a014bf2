"""sp_embedding_pool as an integrator binds it (tests/c_header.py: the header alone): the prototype parses into known
types, matches scratchpad_amd/_native.py's SIGNATURES, is exported, and refuses on the host - before any launch - what
the header says it refuses.  The addition is additive: the ABI version stays 10.  Only calls that return before a
launch are made."""
import ctypes

import pytest

from tests import c_header

NAME = "sp_embedding_pool"
STATUS = c_header.enum_values("sp_status")
OK, INVALID, UNSUPPORTED = STATUS["SP_OK"], STATUS["SP_ERR_INVALID_ARG"], STATUS["SP_ERR_UNSUPPORTED"]
DT = c_header.enum_values("sp_dtype")


def test_prototype_parses_and_matches_native_signatures():
    from scratchpad_amd import _native
    protos = c_header.prototypes()
    assert NAME in protos, f"{NAME} is not declared in include/scratchpad_hip.h"
    res, args = protos[NAME]
    nres, nargs = _native.SIGNATURES[NAME]
    assert res is ctypes.c_int and nres is res
    assert list(nargs) == [t for _, t in args]
    names = [n for n, _ in args]
    assert names == ["out", "out_stride", "x", "x_stride", "residual", "res_stride", "weight", "eps", "extend_seq_lens",
                     "idx64", "num_seqs", "num_tokens", "hidden", "normalize", "dtype", "stream"]
    assert "batch_size" not in names
    assert c_header.abi_version() == 10


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


def test_library_exports_it_and_abi_stays_10(lib):
    assert hasattr(lib, NAME)
    assert lib.sp_abi_version() == 10


def test_host_side_refusals(lib, addr):
    a = addr
    good = dict(out=a, out_stride=4096, x=a, x_stride=4096, residual=a, res_stride=4096, weight=a, eps=1e-5,
                extend_seq_lens=a, idx64=0, num_seqs=0, num_tokens=15, hidden=4096, normalize=1, dtype=DT["SP_BF16"],
                stream=None)
    assert set(good) == {p for p, _ in lib.sp_prototypes[NAME][1]}
    call = lambda **kw: c_header.call(lib, NAME, **{**good, **kw})
    assert call() == OK, "num_seqs == 0 is SP_OK without a launch"
    assert call(residual=None, weight=None, eps=0.0) == OK, "the gather-and-normalise form"
    assert call(residual=None) == OK, "sp_rmsnorm's form"
    for p in ("out", "x", "extend_seq_lens"):
        assert call(num_seqs=3, **{p: None}) == INVALID, p
        assert call(**{p: None}) == INVALID, p + " (no sequences)"
    for p, v in (("num_seqs", -3), ("num_tokens", -15), ("hidden", -4096), ("hidden", 0)):
        assert call(**{p: v}) == INVALID, p
    for p in ("out_stride", "x_stride", "res_stride"):
        assert call(num_seqs=3, **{p: 4095}) == INVALID, p
        assert call(num_seqs=3, **{p: -4096}) == INVALID, p
    assert call(num_seqs=3, weight=None) == INVALID, "a residual without a weight"
    assert call(num_seqs=3, eps=0.0) == INVALID and call(num_seqs=3, eps=-1e-5) == INVALID, "eps <= 0 with a weight"
    assert call(num_seqs=3, residual=None, weight=None, eps=0.0, dtype=7) == UNSUPPORTED
    assert call(dtype=DT["SP_FP8_E5M2"]) == UNSUPPORTED
    # a residual stride is not read when there is no residual
    assert call(residual=None, res_stride=0) == OK
