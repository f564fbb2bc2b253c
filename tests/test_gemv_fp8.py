"""W8A16 decode GEMVs (ops/csrc/gemv_fp8.hip): fp8 e4m3 weights with a
per-row fp32 scale against an fp64 reference, per element:

  |y - y64| <= u |y64| + g scale[n] sum_k |x[m,k]| |w8[n,k]|

u = 2^-8 (the bf16 output rounding), g = 2 (K + 2) 2^-24: K fp32
accumulation roundings in any order plus the scale multiply, doubled for
the unspecified internal rounding of v_dot2c. Derived, not measured.
SwiGLU: dh = u |h| + g (1.1 |u| gabs + |silu(g)| uabs) + e32 |h|, the dh_i
of the moe_gemv.hip tests with g on the dot-product terms; the e32 = 2^-16
term covers the v_exp_f32, the reciprocal and the two multiplies, all
relative to h.
"""

import pytest
import torch

from torchx_amd import ops
from torchx_amd.ops import reference
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
    K = x.shape[1]
    g = 2 * (K + 2) * 2.0 ** -24
    return (xd @ wd.t()) * sd, g * (xd.abs() @ wd.abs().t()) * sd


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", [
    (1, 8, 1024), (3, 21, 4096), (4, 40, 3072), (8, 16, 5120),
    (2, 9, 9216),  # K > 8192: the launcher's 4-rows-per-wave instance
])
def test_gemv_fp8w_within_bound(M, N, K):
    dev = torch.device("cuda:0")
    x, w = _inputs(M, N, K, seed=N)
    y64, dot_bound = _ref_bound(x, w)
    y = ops.hip_ops().gemv_fp8w(x.to(dev), w.w8.to(dev), w.scale.to(dev))
    ratio, ok = bound_ratio(y.cpu(), y64, U * y64.abs() + dot_bound)
    print(f"gemv_fp8w M={M} N={N} K={K}: max err/bound {ratio:.3f}")
    assert ok, ratio


@pytest.mark.gpu
@pytest.mark.parametrize("M,I,K", [(1, 4, 1024), (3, 6, 5120), (8, 8, 4096)])
def test_gemv_swiglu_fp8w_within_bound(M, I, K):
    dev = torch.device("cuda:0")
    x, w = _inputs(M, 2 * I, K, seed=I)
    y64, dot_bound = _ref_bound(x, w)
    (g64, u64), (gb, ub) = y64.chunk(2, dim=1), dot_bound.chunk(2, dim=1)
    silu = g64 * torch.sigmoid(g64)
    h64 = silu * u64
    bound = (U + E32) * h64.abs() + 1.1 * u64.abs() * gb + silu.abs() * ub
    h = ops.hip_ops().gemv_swiglu_fp8w(x.to(dev), w.w8.to(dev),
                                       w.scale.to(dev))
    ratio, ok = bound_ratio(h.cpu(), h64, bound)
    print(f"gemv_swiglu_fp8w M={M} I={I} K={K}: max err/bound {ratio:.3f}")
    assert ok, ratio


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1024, 1536], ids=["kernel", "K1536-fallback"])
def test_decode_linear_fp8_weight_gpu_routes(K):
    dev = torch.device("cuda:0")
    x, w = _inputs(2, 9, K, seed=K)
    y64, dot_bound = _ref_bound(x, w)
    y = ops.decode_linear(x.to(dev).reshape(1, 2, K), w.to(dev))
    assert y.shape == (1, 2, 9) and y.dtype == torch.bfloat16
    assert bound_ratio(y[0].cpu(), y64, U * y64.abs() + dot_bound)[1]
    if K == 1024:
        assert torch.equal(y[0], ops.hip_ops().gemv_fp8w(
            x.to(dev), w.w8.to(dev), w.scale.to(dev)))


@pytest.mark.gpu
def test_decode_step_fp8_weights_end_to_end(monkeypatch):
    """One decode step after a short prefill, fp8 path and bf16 path on the
    snapped weights, both against the same step on the CPU in fp32 with the
    fp32 dequantised weights: max|fp8 - ref| <= 2 max|bf16 - ref|. Both
    round activations to bf16 between the same ops and fp8 has the more
    exact weights; 2 is the margin for the summation orders. 2 layers,
    8/2 heads of 128, intermediate 2048, B = 3; hidden is 2048, not 1024:
    the rmsnorm kernels of the step take multiples of 2048 only."""
    from torchx_amd.models.generate import (
        KVCache, decode_step, prefill, quantize_decode_weights,
    )
    from torchx_amd.models.llama import LlamaConfig, LlamaModel

    dev = torch.device("cuda:0")
    torch.manual_seed(11)
    cfg = LlamaConfig(vocab_size=512, hidden_size=2048, intermediate_size=2048,
                      num_layers=2, num_heads=8, num_kv_heads=2, head_dim=128,
                      max_seq_len=64)
    B, S, T = 3, 16, 32
    model = quantize_decode_weights(LlamaModel(cfg, device=dev))
    ref_model = LlamaModel(cfg)
    ref_model.load_state_dict(model.state_dict())
    ref_model.float()
    lins = [getattr(blk, n) for blk in model.blocks
            for n in ("wqkv", "wo", "wgu", "wdown")]
    ref_lins = [getattr(blk, n) for blk in ref_model.blocks
                for n in ("wqkv", "wo", "wgu", "wdown")]
    for lin, ref_lin in zip(lins, ref_lins):
        ref_lin.weight.data = lin.decode_weight.dequant().cpu()

    tokens = torch.randint(0, cfg.vocab_size, (B, S), device=dev)
    caches = [KVCache.empty(cfg, B, T, dev) for _ in range(cfg.num_layers)]
    nxt = prefill(model, tokens, caches).argmax(-1, keepdim=True)

    def step(m, device, dtype):
        cs = [KVCache(c.k.to(device, dtype), c.v.to(device, dtype), S)
              for c in caches]
        return decode_step(m, nxt.to(device), cs).double().cpu()

    seen = []
    for name in ("decode_linear", "decode_linear_swiglu"):
        def spy(x, w, fn=getattr(ops, name)):
            seen.append(type(w))
            return fn(x, w)
        monkeypatch.setattr(ops, name, spy)
    fp8 = step(model, dev, torch.bfloat16)
    assert seen.count(ops.Fp8Weight) == 4 * cfg.num_layers
    assert len(seen) == 4 * cfg.num_layers + 1  # + the bf16 lm_head
    for lin in lins:
        del lin.decode_weight
    bf16 = step(model, dev, torch.bfloat16)
    ref = step(ref_model, "cpu", torch.float32)
    d8, d16 = (fp8 - ref).abs().max().item(), (bf16 - ref).abs().max().item()
    print(f"decode step max|logits - ref|: fp8 {d8:.4g}, bf16 {d16:.4g}")
    assert d8 <= 2 * d16, (d8, d16)


def test_quantize_fp8_rows():
    torch.manual_seed(0)
    w = torch.randn(6, 1024)
    w[4] = 0.0
    w[5, 0] = torch.finfo(torch.bfloat16).max
    q = ops.quantize_fp8_rows(w.bfloat16())
    w = w.bfloat16().float()
    assert q.shape == (6, 1024) and q.scale.dtype == torch.float32
    deq = q.dequant()
    assert torch.isfinite(deq).all() and q.scale[4] == 1.0
    assert ((deq - w).abs()
            <= 2.0 ** -4 * w.abs() + q.scale[:, None] * 2.0 ** -10).all()
    amax8 = q.w8.float().abs().amax(1)
    assert (amax8[[0, 1, 2, 3, 5]] == 448).all() and amax8[4] == 0


@pytest.mark.parametrize("K", [1024, 1536], ids=["K1024", "K1536-fallback"])
def test_decode_linear_fp8_weight_cpu(K):
    x, w = _inputs(3, 10, K, seed=K)
    x = x.reshape(1, 3, K)
    deq = w.dequant()
    want = (x.float() @ deq.t()).bfloat16()
    assert torch.equal(ops.decode_linear(x, w), want)
    assert torch.equal(reference.decode_linear_fp8w(x, deq), want)
    g, u = (x.float() @ deq.t()).chunk(2, dim=-1)
    want = (torch.nn.functional.silu(g) * u).bfloat16()
    got = ops.decode_linear_swiglu(x, w)
    assert got.shape == (1, 3, 5) and torch.equal(got, want)
