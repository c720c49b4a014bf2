"""sp_gemm_skinny_xielu - up_proj and xIELU of SwissAIMLP (nn/models/swissai/apertus.py:63-68) in one launch - against
its contract: bit for bit sp_gemm_skinny(epilogue 0) followed by sp_xielu, the contract epilogue 1 holds against
sp_silu_and_mul.  Shapes it refuses fall to the two calls inside SwissAIMLP."""
import pytest
import torch

from tests.apertus_oracle import XIELU_BETA, XIELU_EPS

pytestmark = pytest.mark.gpu

UNSUPPORTED = -2
SENTINEL = -7.0


def _inputs(M, N, K, dtype, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(M, K, device="cuda", generator=g).to(dtype)
    w = (torch.randn(N, K, device="cuda", generator=g) * 0.05).to(dtype)
    ap = torch.tensor([-0.75], device="cuda").to(dtype)
    an = torch.tensor([0.5], device="cuda").to(dtype)
    return x, w, ap, an


def _fused(lib, out, x, w, ap, an, M, N, K):
    from scratchpad_amd import _native
    return lib.sp_gemm_skinny_xielu(out.data_ptr(), x.data_ptr(), w.data_ptr(), M, N, K, x.stride(0), w.stride(0),
                                    out.stride(0), ap.data_ptr(), an.data_ptr(), XIELU_BETA, XIELU_EPS,
                                    _native._dt(x), _native._stream())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
# K = 2336 is 73 k-steps: every wave runs one unrolled group of 8 and then a tail step (csrc/stream_gemm.h)
@pytest.mark.parametrize("M,N,K", [(1, 64, 32), (5, 96, 256), (16, 160, 256), (16, 21504, 4096), (7, 96, 2336)])
def test_fused_equals_projection_then_xielu(M, N, K, dtype):
    from scratchpad_amd import _native
    lib = _native.load()
    x, w, ap, an = _inputs(M, N, K, dtype)
    spare = 8
    one = torch.full((M, N + spare), SENTINEL, device="cuda", dtype=dtype)
    two = torch.full((M, N + spare), SENTINEL, device="cuda", dtype=dtype)
    _native._check(_fused(lib, one, x, w, ap, an, M, N, K), "sp_gemm_skinny_xielu")
    _native._check(lib.sp_gemm_skinny(two.data_ptr(), x.data_ptr(), w.data_ptr(), M, N, K, x.stride(0), w.stride(0),
                                      two.stride(0), 0, _native._dt(x), _native._stream()), "sp_gemm_skinny")
    proj = two[:, :N].clone()
    _native._check(lib.sp_xielu(two.data_ptr(), two.data_ptr(), ap.data_ptr(), an.data_ptr(), XIELU_BETA, XIELU_EPS,
                                M, N, two.stride(0), two.stride(0), _native._dt(x), _native._stream()), "sp_xielu")
    assert torch.equal(one.view(torch.int16), two.view(torch.int16)), \
        f"{int((one != two).sum())} of {one.numel()} elements differ from the two-call result"
    assert (one[:, N:] == SENTINEL).all(), "spare output columns were written"
    assert not torch.equal(one[:, :N], proj), "the activation was not applied"
    # and the wrapper takes this path and says so
    before = dict(_native.XIELU_CALLS)
    got = _native.linear_xielu(x, w, ap, an, XIELU_BETA, XIELU_EPS)
    assert _native.XIELU_CALLS["gemm_skinny_xielu"] == before["gemm_skinny_xielu"] + 1
    assert _native.XIELU_CALLS["two_call"] == before["two_call"] and _native.XIELU_CALLS["xielu"] == before["xielu"]
    assert torch.equal(got, one[:, :N])


@pytest.fixture()
def tp1():
    from scratchpad_amd import distributed as dist_
    if not dist_.model_parallel_is_initialized():
        dist_.initialize_model_parallel(1)
    return dist_


@pytest.mark.parametrize("M,K", [(17, 64), (4, 48)], ids=["M17", "K48"])
def test_refused_shapes_take_the_two_calls_in_the_mlp(tp1, M, K):
    from scratchpad_amd import _native
    from scratchpad_amd.apertus import SwissAIMLP
    dtype, N = torch.bfloat16, 96
    lib = _native.load()
    x, w, ap, an = _inputs(M, N, K, dtype, seed=1)
    out = torch.full((M, N), SENTINEL, device="cuda", dtype=dtype)
    assert _fused(lib, out, x, w, ap, an, M, N, K) == UNSUPPORTED
    torch.cuda.synchronize()
    assert (out == SENTINEL).all(), "a refused call launched"
    with torch.device("cuda"):
        mlp = SwissAIMLP(K, N, "xielu", dtype=dtype).to(dtype)
    g = torch.Generator(device="cuda").manual_seed(2)
    mlp.up_proj.weight.data.copy_(w)
    mlp.down_proj.weight.data.copy_((torch.randn(K, N, device="cuda", generator=g) * 0.05).to(dtype))
    mlp.act_fn.alpha_p.data.copy_(ap)
    mlp.act_fn.alpha_n.data.copy_(an)
    before = dict(_native.XIELU_CALLS)
    got = mlp(x)
    assert _native.XIELU_CALLS["gemm_skinny_xielu"] == before["gemm_skinny_xielu"]
    assert _native.XIELU_CALLS["xielu"] == before["xielu"] + 1
    assert _native.XIELU_CALLS["two_call"] == before["two_call"] + (1 if M <= 16 else 0)
    up = _native.linear(x, w)
    act = _native.xielu(up, ap, an, XIELU_BETA, XIELU_EPS)
    want = _native.linear(act, mlp.down_proj.weight)
    assert torch.equal(got, want)
    assert torch.isfinite(got).all() and float(got.abs().max()) > 0
