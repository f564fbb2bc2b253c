#!/usr/bin/env python3
"""Attention kernel microbenchmark: TF/s for fwd and bwd at the bench shape
(B=4, S=4096, Hq=32, Hkv=8, D=128, causal bf16)."""

import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from torchx_amd import ops


def flops_fwd(B, S, Hq, D, causal):
    f = 2 * 2 * B * Hq * S * S * D  # QK^T + PV
    return f // 2 if causal else f


def time_fn(fn, iters=20, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def time_events(fn, iters):
    """Mean ms per call by device events."""
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def bench_paged_prefill(iters, rounds=5):
    """paged_prefill_attn at ctx=0 against attn_fwd on the same logical
    data: the K/V of a dense run scattered into pages through a seeded
    permutation. The two kernels alternate within each round; per shape
    the median round and the spread over rounds are printed."""
    hip = ops.hip_ops(required=True)
    dev = torch.device("cuda", 0)
    Hq, Hkv, D = 32, 8, 128
    scale = D ** -0.5
    for B, S in ((4, 4096), (1, 512)):
        torch.manual_seed(0)
        q = torch.randn(B, S, Hq, D, device=dev, dtype=torch.bfloat16)
        k = torch.randn(B, S, Hkv, D, device=dev, dtype=torch.bfloat16)
        v = torch.randn(B, S, Hkv, D, device=dev, dtype=torch.bfloat16)
        ctx = torch.zeros(B, dtype=torch.int32, device=dev)
        for P in (16, 64):
            M = S // P
            g = torch.Generator().manual_seed(0)
            table = (torch.randperm(B * M, generator=g) + 1).to(torch.int32)
            table = table.reshape(B, M).to(dev)
            kpool = torch.zeros(B * M + 1, P, Hkv, D, device=dev,
                                dtype=torch.bfloat16)
            vpool = torch.zeros_like(kpool)
            kpool[table.long().reshape(-1)] = k.reshape(B * M, P, Hkv, D)
            vpool[table.long().reshape(-1)] = v.reshape(B * M, P, Hkv, D)

            def dense():
                return hip.attn_fwd(q, k, v, scale, True)

            def paged():
                return hip.paged_prefill_attn(q, kpool, vpool, table, ctx,
                                              scale)

            same = torch.equal(dense()[0], paged())
            for _ in range(5):
                dense()
                paged()
            # the small shape runs tens of microseconds: time more calls
            n = iters if S >= 4096 else iters * 50
            td, tp = [], []
            for _ in range(rounds):
                td.append(time_events(dense, n))
                tp.append(time_events(paged, n))
            td.sort()
            tp.sort()
            fl = flops_fwd(B, S, Hq, D, True)
            md, mp = td[rounds // 2], tp[rounds // 2]
            print(f"B{B} S{S} H{Hq}/{Hkv} P{P}: dense {md:.4f} ms "
                  f"[{td[0]:.4f}..{td[-1]:.4f}] {fl / md / 1e9:.0f} TF/s | "
                  f"paged {mp:.4f} ms [{tp[0]:.4f}..{tp[-1]:.4f}] "
                  f"{fl / mp / 1e9:.0f} TF/s | paged/dense {mp / md:.3f} | "
                  f"bit-identical {same}")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--B", type=int, default=4)
    p.add_argument("--S", type=int, default=4096)
    p.add_argument("--Hq", type=int, default=32)
    p.add_argument("--Hkv", type=int, default=8)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--mode", type=str, default="both",
                   choices=["fwd", "bwd", "both", "paged-prefill"],
                   help="paged-prefill: time paged_prefill_attn at ctx=0 "
                        "against attn_fwd (fixed shapes B4 S4096 and "
                        "B1 S512, H32/8, page sizes 16 and 64)")
    p.add_argument("--dq-mode", type=str, default=None,
                   choices=["stream", "recompute"],
                   help="dQ path of the backward (default: the extension's "
                        "own default, see ops.set_attn_bwd_dq_mode)")
    p.add_argument("--dkv-impl", type=str, default=None,
                   choices=["merged", "split"],
                   help="dK/dV kernel of the backward (default: the "
                        "extension's own default, see "
                        "ops.set_attn_bwd_dkv_impl)")
    args = p.parse_args()
    if args.mode == "paged-prefill":
        bench_paged_prefill(args.iters)
        return
    B, S, Hq, Hkv, D = args.B, args.S, args.Hq, args.Hkv, 128
    if args.dkv_impl is not None:
        ops.set_attn_bwd_dkv_impl(args.dkv_impl)
    if args.dq_mode is not None:
        ops.set_attn_bwd_dq_mode(args.dq_mode)

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    q = torch.randn(B, S, Hq, D, device=dev, dtype=torch.bfloat16, requires_grad=True)
    k = torch.randn(B, S, Hkv, D, device=dev, dtype=torch.bfloat16, requires_grad=True)
    v = torch.randn(B, S, Hkv, D, device=dev, dtype=torch.bfloat16, requires_grad=True)
    do = torch.randn(B, S, Hq, D, device=dev, dtype=torch.bfloat16)

    hip = ops.hip_ops(required=True)
    scale = D ** -0.5

    def fwd():
        return hip.attn_fwd(q, k, v, scale, True)

    o, lse = fwd()
    if args.mode in ("fwd", "both"):
        t_fwd = time_fn(fwd, args.iters)
        tf_fwd = flops_fwd(B, S, Hq, D, True) / t_fwd / 1e12
        print(f"fwd: {t_fwd*1e3:.3f} ms  {tf_fwd:.0f} TF/s")

    if args.mode in ("bwd", "both"):
        def bwd():
            return hip.attn_bwd(q, k, v, o, do, lse, scale, True)

        t_bwd = time_fn(bwd, args.iters)
        tf_bwd = flops_fwd(B, S, Hq, D, True) * 2.5 / t_bwd / 1e12
        print(f"bwd: {t_bwd*1e3:.3f} ms  {tf_bwd:.0f} TF/s")


if __name__ == "__main__":
    main()
