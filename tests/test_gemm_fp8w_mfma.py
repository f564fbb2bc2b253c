"""W8A16 decode GEMM on MFMA (ops/csrc/gemm_fp8w_mfma.hip), M = 1..32,
against an fp64 reference, per element, with the inputs and the bound of
test_gemv_fp8.py:

  |y - y64| <= u |y64| + g scale[n] sum_k |x[m,k]| |w8[n,k]|

u = 2^-8 (the bf16 output rounding), g = 2 (K + 2) 2^-24: K fp32 roundings
in any order plus the scale multiply, doubled for unspecified internal
rounding, which covers the MFMA's accumulation and the three adds of the
epilogue. SwiGLU: dh = (u + e32) |h| + 1.1 |u| gb + |silu(g)| ub with gb, ub
the dot-product bounds of g and u. Derived, not measured.
"""

import pytest
import torch

from torchx_amd import ops
from torchx_amd.ops.bounds import E32, U, bound_ratio


def _inputs(M, N, K, seed):
    """bf16 x [M, K]; randn w [N, K] with row n times 2^((n % 5) - 2), so
    that the row scales differ, quantised."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).bfloat16()
    w = torch.randn(N, K, generator=g)
    w *= (2.0 ** ((torch.arange(N) % 5) - 2))[:, None]
    return x, ops.quantize_fp8_rows(w)


def _ref_bound(x, w):
    """fp64 y64 [M, N] and the dot-product part of the bound."""
    xd, wd, sd = x.double(), w.w8.double(), w.scale.double()
    g = 2 * (x.shape[1] + 2) * 2.0 ** -24
    return (xd @ wd.t()) * sd, g * (xd.abs() @ wd.abs().t()) * sd


def _swiglu_ref_bound(x, w):
    y64, dot_bound = _ref_bound(x, w)
    (g64, u64), (gb, ub) = y64.chunk(2, dim=1), dot_bound.chunk(2, dim=1)
    silu = g64 * torch.sigmoid(g64)
    h64 = silu * u64
    return h64, (U + E32) * h64.abs() + 1.1 * u64.abs() * gb + silu.abs() * ub


def _dev(x, w):
    dev = torch.device("cuda:0")
    return x.to(dev), w.w8.to(dev), w.scale.to(dev)


# The launcher takes RT = 2 row tiles per block for N > 8192, and for
# N > 4096 at M > 16, else 1; MT = 1 token tile up to M = 16 and 2 above;
# (RT, MT) after each shape. The last two are added to the issue's six so
# that both RT = 2 instances run.
@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", [
    (1, 16, 1024),    # (1, 1) one token, one exact tile, one loop iteration
    (5, 21, 2048),    # (1, 1) partial second block
    (9, 40, 3072),    # (1, 1) three blocks, the last partial
    (16, 16, 5120),   # (1, 1) full token tile
    (17, 9, 1024),    # (1, 2) one live column in the second tile; N < 16
    (32, 33, 9216),   # (1, 2) full token tiles
    (9, 8200, 1024),  # (2, 1) last block: 8 live rows, second tile past N
    (32, 4129, 1024),  # (2, 2) last block: one live row, N % 4 != 0
])
def test_gemm_fp8w_mfma_within_bound(M, N, K):
    x, w = _inputs(M, N, K, seed=N)
    y64, dot_bound = _ref_bound(x, w)
    y = ops.hip_ops().gemm_fp8w_mfma(*_dev(x, w))
    ratio, ok = bound_ratio(y.cpu(), y64, U * y64.abs() + dot_bound)
    print(f"gemm_fp8w_mfma M={M} N={N} K={K}: max err/bound {ratio:.3f}")
    assert ok, ratio


@pytest.mark.gpu
@pytest.mark.parametrize("M,I,K", [
    (1, 4, 1024), (12, 24, 3072),  # MT = 1; one and two blocks
    (32, 16, 2048)])               # MT = 2
def test_gemm_swiglu_fp8w_mfma_within_bound(M, I, K):
    x, w = _inputs(M, 2 * I, K, seed=I)
    h64, bound = _swiglu_ref_bound(x, w)
    h = ops.hip_ops().gemm_swiglu_fp8w_mfma(*_dev(x, w))
    ratio, ok = bound_ratio(h.cpu(), h64, bound)
    print(f"gemm_swiglu_fp8w_mfma M={M} I={I} K={K}: max err/bound "
          f"{ratio:.3f}")
    assert ok, ratio


@pytest.mark.gpu
@pytest.mark.parametrize("op,M,Mp,N", [
    ("gemm_fp8w_mfma", 16, 9, 21), ("gemm_fp8w_mfma", 32, 17, 21),
    ("gemm_swiglu_fp8w_mfma", 32, 17, 42)])
def test_columns_independent(op, M, Mp, N):
    """Rows 0 .. M' - 1 of the M-row output are those of the call on
    x[:M'], bit for bit: no padding column leaks, no clamped row is
    stored."""
    x, w8, scale = _dev(*_inputs(M, N, 2048, seed=M))
    fn = getattr(ops.hip_ops(), op)
    assert torch.equal(fn(x, w8, scale)[:Mp], fn(x[:Mp].contiguous(), w8,
                                                scale))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1024, 1536], ids=["kernel", "K1536-fallback"])
def test_decode_linear_routes_m12(K):
    dev = torch.device("cuda:0")
    x, w = _inputs(12, 18, K, seed=K)
    y64, dot_bound = _ref_bound(x, w)
    h64, h_bound = _swiglu_ref_bound(x, w)
    xd, wd = x.to(dev).reshape(1, 12, K), w.to(dev)
    y = ops.decode_linear(xd, wd)
    h = ops.decode_linear_swiglu(xd, wd)
    assert y.shape == (1, 12, 18) and h.shape == (1, 12, 9)
    assert bound_ratio(y[0].cpu(), y64, U * y64.abs() + dot_bound)[1]
    assert bound_ratio(h[0].cpu(), h64, h_bound)[1]
    if K == 1024:
        assert torch.equal(y[0], ops.hip_ops().gemm_fp8w_mfma(*_dev(x, w)))
        assert torch.equal(
            h[0], ops.hip_ops().gemm_swiglu_fp8w_mfma(*_dev(x, w)))
