#!/usr/bin/env python3
"""Per-shape decode-GEMV probe: gemv_bf16 vs torch.matmul (hipBLASLt) at
the Llama-3-8B decode shapes, CUDA-event timed, with achieved weight-
stream GB/s (the op's roof is the ~8 TB/s HBM3E read of W); then the
bf16 kernels against the W8A16 ones (gemv_fp8.hip) on the four block
shapes at M = 1, 4, 8. ``--mfma`` runs only the MFMA fp8 kernels
(gemm_fp8w_mfma.hip) against the dot2 kernels and bf16 matmul."""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from torchx_amd.ops import hip_ops, quantize_fp8_rows

SHAPES = [  # (M, N, K) = (batch, out-features, in-features)
    ("wqkv", 4, 6144, 4096),
    ("wo", 4, 4096, 4096),
    ("wgu", 4, 28672, 4096),
    ("wdown", 4, 4096, 14336),
    ("lm_head", 4, 128256, 4096),
]


def time_fn(fn, iters=100):
    s, e = torch.cuda.Event(True), torch.cuda.Event(True)
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3  # us


def main():
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    ops = hip_ops()
    tot_g = tot_m = 0.0
    for name, M, N, K in SHAPES:
        x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
        w = torch.randn(N, K, device=dev, dtype=torch.bfloat16)
        t_g = time_fn(lambda: ops.gemv_bf16(x, w))
        t_m = time_fn(lambda: torch.matmul(x, w.t()))
        gb = N * K * 2 / 1e9
        print(f"{name:8s} M={M} N={N:6d} K={K:5d}  W={gb*1e3:7.1f} MB  "
              f"gemv {t_g:7.1f} us ({gb/(t_g*1e-6):6.0f} GB/s)  "
              f"matmul {t_m:7.1f} us ({gb/(t_m*1e-6):6.0f} GB/s)")
        tot_g += t_g
        tot_m += t_m
    layer_g = tot_g - t_g  # last shape is lm_head
    layer_m = tot_m - t_m
    print(f"one decode step GEMV total: gemv {(layer_g*32 + t_g)/1e3:.3f} ms"
          f"  matmul {(layer_m*32 + t_m)/1e3:.3f} ms")

    # fused wgu+swiglu vs separate gemv + swiglu kernel
    M, I, K = 4, 14336, 4096
    x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
    w = torch.randn(2 * I, K, device=dev, dtype=torch.bfloat16)
    t_f = time_fn(lambda: ops.gemv_swiglu_bf16(x, w))
    gb = 2 * I * K * 2 / 1e9
    print(f"wgu+swiglu fused: {t_f:7.1f} us ({gb/(t_f*1e-6):6.0f} GB/s) "
          f"vs separate gemv {time_fn(lambda: ops.gemv_bf16(x, w)):7.1f} us"
          f" + swiglu kernel")
    fp8_vs_bf16(dev, ops)
    return 0


def fp8_vs_bf16(dev, ops, rounds=3):
    """bf16 against fp8 weights on the four block GEMVs (wgu through the
    fused SwiGLU kernels), alternated within each round; median time and
    weight bytes/s of each, and fp8 time / bf16 time."""
    print("bf16 vs fp8 weights (us, weight GB/s; ratio = fp8 / bf16 time)")
    for name, _, N, K in SHAPES[:4]:
        w = torch.randn(N, K, device=dev, dtype=torch.bfloat16)
        q = quantize_fp8_rows(w)
        if name == "wgu":
            f16, f8 = ops.gemv_swiglu_bf16, ops.gemv_swiglu_fp8w
        else:
            f16, f8 = ops.gemv_bf16, ops.gemv_fp8w
        for M in (1, 4, 8):
            x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
            t16, t8 = [], []
            for _ in range(rounds):
                t16.append(time_fn(lambda: f16(x, w)))
                t8.append(time_fn(lambda: f8(x, q.w8, q.scale)))
            t16, t8 = sorted(t16)[rounds // 2], sorted(t8)[rounds // 2]
            print(f"{name:6s} M={M} N={N:6d} K={K:5d}  "
                  f"bf16 {t16:7.1f} us ({N*K*2/t16/1e3:6.0f} GB/s)  "
                  f"fp8 {t8:7.1f} us ({N*K/t8/1e3:6.0f} GB/s)  "
                  f"ratio {t8/t16:.3f}")


def _median_rounds(fns, rounds, iters=100):
    """Median us of each fn over ``rounds`` rounds, the fns alternated
    within a round."""
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for t, fn in zip(ts, fns):
            t.append(time_fn(fn, iters))
    return [sorted(t)[rounds // 2] for t in ts]


def mfma_vs_dot2_bf16(dev, ops, rounds=5):
    """The MFMA fp8-weight kernels (gemm_fp8w_mfma.hip) on the four block
    shapes (wgu through the fused SwiGLU kernels): against the dot2 kernels
    at M = 4 .. 8 and against what the bf16 path runs at M = 9, 16, 32
    (``x @ w.t()``, plus the torch SwiGLU for wgu), alternated within each
    round, medians. The plain kernel is timed with 1 and with 2 row tiles
    per block. One timing of the dequantising fallback per shape."""
    from torchx_amd.ops import reference

    def bf16_swiglu(x, w):
        g, u = (x @ w.t()).chunk(2, dim=-1)
        return torch.nn.functional.silu(g.float()).to(u.dtype) * u

    print("mfma fp8 kernels (us, fp8 weight GB/s); rt = row tiles per block")
    for name, _, N, K in SHAPES[:4]:
        w = torch.randn(N, K, device=dev, dtype=torch.bfloat16)
        q = quantize_fp8_rows(w)
        glu = name == "wgu"
        if glu:
            new = [lambda x: ops.gemm_swiglu_fp8w_mfma(x, q.w8, q.scale)]
            tags = ["mfma"]
        else:
            new = [lambda x, rt=rt: ops.gemm_fp8w_mfma(x, q.w8, q.scale, rt)
                   for rt in (1, 2)]
            tags = ["mfma rt=1", "mfma rt=2"]
        for M in (4, 5, 6, 7, 8, 9, 16, 32):
            x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
            if M <= 8:
                old = ops.gemv_swiglu_fp8w if glu else ops.gemv_fp8w
                other, otag = (lambda x: old(x, q.w8, q.scale)), "dot2"
            elif glu:
                other, otag = (lambda x: bf16_swiglu(x, w)), "bf16 matmul"
            else:
                other, otag = (lambda x: x @ w.t()), "bf16 matmul"
            ts = _median_rounds([lambda f=f: f(x) for f in new + [other]],
                                rounds)
            line = "  ".join(f"{tag} {t:7.1f} us ({N*K/t/1e3:6.0f} GB/s)"
                             for tag, t in zip(tags, ts))
            print(f"{name:6s} M={M:2d} N={N:6d} K={K:5d}  {line}  "
                  f"{otag} {ts[-1]:7.1f} us  "
                  f"ratio {min(ts[:-1])/ts[-1]:.3f}")
        fb = reference.decode_linear_swiglu_fp8w if glu \
            else reference.decode_linear_fp8w
        t = time_fn(lambda: fb(x, q.dequant()), iters=5)
        print(f"{name:6s} M={M:2d} dequantising fallback {t:9.1f} us")


if __name__ == "__main__":
    if "--mfma" in sys.argv:
        sys.exit(mfma_vs_dot2_bf16(torch.device("cuda:0"), hip_ops()))
    sys.exit(main())
