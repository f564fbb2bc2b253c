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


def _alternate(fns, n, rounds):
    """Time the callables in turn within each round; per callable the
    (median, min, max) ms over the rounds."""
    for _ in range(5):
        for fn in fns.values():
            fn()
    ts = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            ts[name].append(time_events(fn, n))
    out = {}
    for name, t in ts.items():
        t.sort()
        out[name] = (t[rounds // 2], t[0], t[-1])
    return out


def _show(label, res, base):
    parts = [f"{name} {m:.4f} ms [{lo:.4f}..{hi:.4f}]"
             for name, (m, lo, hi) in res.items()]
    ratios = [f"{name}/{base} {res[name][0] / res[base][0]:.3f}"
              for name in res if name != base]
    print(f"{label}: " + " | ".join(parts + ratios))


def bench_paged_prefill_ragged(iters, rounds=5):
    """paged_prefill_attn_ragged (tiles heaviest first, and sequence by
    sequence) against paged_prefill_attn on the same pools, ctx = 0,
    H32/8, P16: at equal lengths (B4 S4096, B4 S512) on the same data; at
    q_lens [4096, 512, 512, 64] against a loop of the existing op per
    sequence and against the existing op padded to the longest. Then the
    fused rope + page append against the dispatches it replaces at
    T = 2048. The candidates alternate within each round."""
    hip = ops.hip_ops(required=True)
    dev = torch.device("cuda", 0)
    Hq, Hkv, D, P = 32, 8, 128, 16
    scale = D ** -0.5
    for q_lens in ([4096] * 4, [512] * 4, [4096, 512, 512, 64]):
        torch.manual_seed(0)
        B, S = len(q_lens), max(q_lens)
        M = S // P                       # every row mapped: padding is legal
        g = torch.Generator().manual_seed(0)
        table = (torch.randperm(B * M, generator=g) + 1).to(torch.int32)
        table = table.reshape(B, M).to(dev)
        kpool = torch.randn(B * M + 1, P, Hkv, D, device=dev,
                            dtype=torch.bfloat16)
        vpool = torch.randn_like(kpool)
        qpad = torch.randn(B, S, Hq, D, device=dev, dtype=torch.bfloat16)
        q = torch.cat([qpad[b, :n] for b, n in enumerate(q_lens)])
        ctx = torch.zeros(B, dtype=torch.int32, device=dev)
        plans = {h: ops.RaggedPlan(q_lens, dev, heavy_first=h)
                 for h in (True, False)}
        per_seq = [(qpad[b:b + 1, :n].contiguous(), table[b:b + 1],
                    ctx[b:b + 1]) for b, n in enumerate(q_lens)]

        def ragged(heavy):
            return lambda: hip.paged_prefill_attn_ragged(
                q, kpool, vpool, table, ctx, plans[heavy].tiles, scale)

        def padded():
            return hip.paged_prefill_attn(qpad, kpool, vpool, table, ctx,
                                          scale)

        def loop():
            return [hip.paged_prefill_attn(qb, kpool, vpool, tb, cb, scale)
                    for qb, tb, cb in per_seq]

        fns = {"ragged_heavy_first": ragged(True),
               "ragged_in_order": ragged(False)}
        equal = len(set(q_lens)) == 1
        if equal:
            fns["existing"] = padded
            same = torch.equal(ragged(True)().reshape(qpad.shape), padded())
        else:
            fns["loop"] = loop
            fns["padded"] = padded
            same = torch.equal(ragged(True)(),
                               torch.cat([o[0] for o in loop()]))
        n = iters if S >= 4096 else iters * 20
        res = _alternate(fns, n, rounds)
        _show(f"q_lens {q_lens} H{Hq}/{Hkv} P{P} bit-identical {same}", res,
              "existing" if equal else "loop")

    # fused rope + page append against split + 3 contiguous copies +
    # 2 ropes + 2 index_copy_ (what prefill_extend runs per layer)
    T = 2048
    torch.manual_seed(0)
    qkv = torch.randn(T, (Hq + 2 * Hkv) * D, device=dev,
                      dtype=torch.bfloat16)
    ang = torch.arange(T).float()[:, None] * (
        1.0 / 10000.0 ** (torch.arange(0, D, 2).float() / D))[None]
    cos, sin = ang.cos().to(dev), ang.sin().to(dev)
    pos = torch.arange(T, dtype=torch.int32, device=dev)
    g = torch.Generator().manual_seed(1)
    pages = (torch.randperm(T // P, generator=g) + 1).to(dev)
    slot = (pages[pos.long() // P] * P + pos.long() % P).int()
    slot_l = slot.long()
    kpool = torch.zeros(T // P + 1, P, Hkv, D, device=dev,
                        dtype=torch.bfloat16)
    vpool = torch.zeros_like(kpool)
    kflat, vflat = kpool.view(-1, Hkv, D), vpool.view(-1, Hkv, D)

    def fused():
        return hip.paged_prefill_rope_cache(qkv, kpool, vpool, cos, sin, pos,
                                            slot)

    def unfused():
        q, k, v = qkv.split([Hq * D, Hkv * D, Hkv * D], dim=-1)
        q = ops.rope(q.reshape(1, T, Hq, D).contiguous(), cos, sin)
        k = ops.rope(k.reshape(1, T, Hkv, D).contiguous(), cos, sin)
        v = v.reshape(1, T, Hkv, D).contiguous()
        kflat.index_copy_(0, slot_l, k[0])
        vflat.index_copy_(0, slot_l, v[0])
        return q

    qf = fused()
    kf = kpool.clone()
    same = torch.equal(qf, unfused()[0]) and torch.equal(kf, kpool)
    res = _alternate({"fused": fused, "unfused": unfused}, iters * 20, rounds)
    _show(f"rope + page append T{T} H{Hq}/{Hkv} P{P} bit-identical {same}",
          res, "unfused")


def bench_fwd_map(B, S, Hq, Hkv, iters, rounds=5):
    """attn_fwd (causal) under each block map, alternating within each
    round of one process: "legacy" (map_block_fwd), "adjacent" (the G heads
    of a unit adjacent on one XCD, tiles ascending) and "balanced" (the
    same, heaviest tiles first)."""
    hip = ops.hip_ops(required=True)
    dev = torch.device("cuda", 0)
    D = 128
    scale = D ** -0.5
    torch.manual_seed(0)
    q = torch.randn(B, S, Hq, D, device=dev, dtype=torch.bfloat16)
    k = torch.randn(B, S, Hkv, D, device=dev, dtype=torch.bfloat16)
    v = torch.randn(B, S, Hkv, D, device=dev, dtype=torch.bfloat16)
    before = ops.get_attn_fwd_map()

    def run(name):
        def fn():
            ops.set_attn_fwd_map(name)
            return hip.attn_fwd(q, k, v, scale, True)
        return fn

    fns = {name: run(name) for name in ("legacy", "adjacent", "balanced")}
    ref = fns["legacy"]()
    same = all(torch.equal(a, b) for name in ("adjacent", "balanced")
               for a, b in zip(fns[name](), ref))
    res = _alternate(fns, iters, rounds)
    ops.set_attn_fwd_map(before)
    fl = flops_fwd(B, S, Hq, D, True)
    _show(f"fwd map B{B} S{S} H{Hq}/{Hkv} bit-identical {same} "
          f"(legacy {fl / res['legacy'][0] / 1e9:.0f} TF/s, balanced "
          f"{fl / res['balanced'][0] / 1e9:.0f} TF/s)", res, "legacy")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--B", type=int, default=4)
    p.add_argument("--S", type=int, default=4096)
    p.add_argument("--Hq", type=int, default=32)
    p.add_argument("--Hkv", type=int, default=8)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--mode", type=str, default="both",
                   choices=["fwd", "bwd", "both", "fwd-map", "paged-prefill",
                            "paged-prefill-ragged"],
                   help="fwd-map: time attn_fwd at --B/--S/--Hq/--Hkv "
                        "under each block map (ops.set_attn_fwd_map) in "
                        "one process; paged-prefill: time paged_prefill_attn at ctx=0 "
                        "against attn_fwd (fixed shapes B4 S4096 and "
                        "B1 S512, H32/8, page sizes 16 and 64); "
                        "paged-prefill-ragged: time the ragged kernel "
                        "against paged_prefill_attn at equal and mixed "
                        "lengths, and the fused rope + page append against "
                        "the dispatches it replaces")
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
    if args.mode == "paged-prefill-ragged":
        bench_paged_prefill_ragged(args.iters)
        return
    B, S, Hq, Hkv, D = args.B, args.S, args.Hq, args.Hkv, 128
    if args.mode == "fwd-map":
        bench_fwd_map(B, S, Hq, Hkv, args.iters)
        return
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
