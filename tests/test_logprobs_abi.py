"""sp_logprobs as an integrator binds it (tests/c_header.py: the header alone): declared, typed as
scratchpad_amd/_native.py's SIGNATURES say, exported, and refusing on the host - before any launch - what the header
says it refuses.  Additive: the ABI version stays 10.  Plus the CPU self-test of tests/logprob_oracle.py, the float64
statement the GPU tests (tests/test_gpu_logprobs.py) hold the kernel to."""
import ctypes
import re

import numpy as np
import pytest
import torch

from oracle import sampling as osamp
from tests import c_header, logprob_oracle as lpo

NAMES = ("sp_logprobs", "sp_logprobs_workspace_bytes")
STATUS = c_header.enum_values("sp_status")
OK, INVALID, WORKSPACE = STATUS["SP_OK"], STATUS["SP_ERR_INVALID_ARG"], STATUS["SP_ERR_WORKSPACE"]


def _cap() -> int:
    return int(re.search(r"#define\s+SP_LOGPROBS_MAX_TOP_K\s+(\d+)", open(c_header.HEADER).read()).group(1))


def test_header_declares_it_with_the_native_signature():
    from scratchpad_amd import _native
    protos = c_header.prototypes()
    for name in NAMES:
        assert name in protos, f"{name} is not declared in include/scratchpad_hip.h"
        res, args = protos[name]
        nres, nargs = _native.SIGNATURES[name]
        assert nres is res and list(nargs) == [t for _, t in args], name
    res, args = protos["sp_logprobs"]
    names = [n for n, _ in args]
    assert res is ctypes.c_int and names[-1] == "stream" and names[:3] == ["rows", "row_stride", "kind"]
    assert "num_rows" in names and "batch_size" not in names
    assert protos["sp_logprobs_workspace_bytes"][0] is ctypes.c_size_t
    assert c_header.abi_version() == 10
    assert _cap() >= 20 and _native.LOGPROBS_MAX_TOP_K == _cap()


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


def test_library_exports_it_and_abi_stays_10(lib):
    for name in NAMES:
        assert hasattr(lib, name)
    assert lib.sp_abi_version() == 10


def test_workspace_bytes(lib):
    ws = lambda n, v, k: c_header.call(lib, "sp_logprobs_workspace_bytes", num_rows=n, vocab=v, max_top_k=k)
    assert ws(0, 1000, 5) == 0 and ws(-1, 1000, 5) == 0 and ws(4, 0, 5) == 0 and ws(4, 1000, _cap() + 1) == 0
    assert ws(256, 128256, 20) == 256 * (16 + 8 * 20)                 # one workgroup per row
    assert ws(1, 128256, 20) > ws(256, 128256, 20) // 256             # few rows: a row is cut into slices
    assert ws(1, 128256, 20) % (16 + 8 * 20) == 0 and ws(1, 128256, 20) // (16 + 8 * 20) <= 32
    assert ws(1, 1000, 0) == 16                                       # a row too short to cut


def test_host_side_refusals(lib, addr):
    a = addr
    good = dict(rows=a, row_stride=1030, kind=0, top_ps=None, chosen_ids=a, top_ks=a, max_top_k=5, ids_offsets=a,
                ids_flat=a, num_rows=3, vocab=1000, out_chosen=a, out_top_vals=a, out_top_ids=a, out_ids_vals=a,
                workspace=a, workspace_bytes=1 << 20, stream=None)
    assert set(good) == {p for p, _ in lib.sp_prototypes["sp_logprobs"][1]}
    cases = [(dict(rows=None), INVALID), (dict(workspace=None), INVALID),
             (dict(out_chosen=None), INVALID),                              # chosen_ids without its output
             (dict(out_top_vals=None), INVALID), (dict(out_top_ids=None), INVALID),
             (dict(out_ids_vals=None), INVALID),
             (dict(ids_offsets=None), INVALID), (dict(ids_flat=None), INVALID),  # the CSR pair is nullable together
             (dict(num_rows=-3), INVALID), (dict(vocab=-1000), INVALID), (dict(vocab=0), INVALID),
             (dict(max_top_k=-1), INVALID), (dict(max_top_k=_cap() + 1), INVALID),
             (dict(kind=2), INVALID), (dict(kind=-1), INVALID),
             (dict(row_stride=999), INVALID),
             (dict(workspace_bytes=8), WORKSPACE),
             (dict(num_rows=0), OK), (dict(num_rows=0, rows=None, workspace=None, workspace_bytes=0), OK),
             (dict(num_rows=0, max_top_k=_cap() + 1), INVALID)]
    for override, want in cases:
        got = c_header.call(lib, "sp_logprobs", **{**good, **override})
        assert got == want, f"sp_logprobs({override}) returned {got}, expected {want}"


# --------------------------------------------------------------------------- the oracle, against torch and oracle/
def test_oracle_kind0_is_log_softmax():
    x = lpo.logit_rows(777, 6)
    got = lpo.all_values(x, 0)
    want = torch.log_softmax(torch.from_numpy(x).double(), dim=-1).numpy()
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(got)) and np.all(got[~fin] == -np.inf)
    assert np.allclose(got[fin], want[fin], atol=1e-12)


def test_oracle_kind1_is_log_of_renorm_rows():
    p, top_ps = lpo.prob_rows(777, 9)
    got = lpo.all_values(p, 1, top_ps)
    ren = osamp.renorm_rows(p, None, top_ps, None).astype(np.float64)
    dropped = ren == 0
    assert dropped.any() and not dropped.all()
    assert np.all(got[dropped] == lpo.FLOOR)
    # renorm_rows rounds to fp32 twice (the denominator, the quotient): 3 ulp of a value near 1 in the logarithm
    assert np.allclose(got[~dropped], np.log(ren[~dropped]), atol=4e-7)
    # no top_p: everything with mass is kept
    assert np.all((lpo.all_values(p, 1, None) > lpo.FLOOR) == (p > 0))


def test_oracle_top_order_is_value_descending_id_ascending():
    row = np.array([1.0, 3.0, 3.0, -np.inf, 2.0, 3.0, -0.0, 0.0], dtype=np.float32)
    assert lpo.top_order(row, 8).tolist() == [1, 2, 5, 4, 0, 6, 7, 3]
    x = lpo.logit_rows(5000, 5)
    for b in range(5):
        ids = lpo.top_order(x[b], 20)
        assert ids.tolist() == np.lexsort((np.arange(5000), -x[b].astype(np.float64)))[:20].tolist()
        v = x[b][ids]
        assert np.all(np.diff(v) <= 0) and all(ids[i] < ids[i + 1] for i in range(19) if v[i] == v[i + 1])
    assert lpo.distinct_top(np.array([3, 2, 1, 0], np.float32), 2) and not lpo.distinct_top(np.array([3, 2, 2, 0], np.float32), 2)


def test_tie_heavy_rows_have_ties_inside_the_top_20():
    """what the GPU tests rely on when they call their rows tie-heavy"""
    for vocab in (32000, 128256):
        x = lpo.logit_rows(vocab, 8)
        tied = [not lpo.distinct_top(x[b], 20) for b in range(8)]
        assert sum(tied) >= 6, (vocab, tied)
        p, _ = lpo.prob_rows(vocab, 8)
        assert sum(not lpo.distinct_top(p[b], 20) for b in range(8)) >= 6


def test_expected_reports_floor_outside_the_vocabulary():
    x = lpo.logit_rows(100, 2)
    c, tv, ti, iv = lpo.expected(x, 0, None, [100, -1], [0, 3], [[5, 200], None])
    assert c.tolist() == [lpo.FLOOR, lpo.FLOOR] and iv[0][1] == lpo.FLOOR and iv[0][0] > lpo.FLOOR
    assert ti[0] == [] and len(ti[1]) == 3 and len(iv[1]) == 0
