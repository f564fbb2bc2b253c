#!/usr/bin/env python3
"""Mixtral decode MLP probe: the grouped expert kernels on bf16 experts
(moe_gemv.hip) against the W8A16 ones (moe_gemv_fp8.hip).

Default: kernel level. 8x7B-shaped experts (H 4096, I 14336, E 8, k 2) at
B = 1, 4, 8 with a seeded top-k routing; kernel A, and kernel B with 2 and
with 4 output rows per wave, bf16 and fp8 alternated within each round,
device events, median of the rounds; us and weight TB/s of the active
experts. Every call takes the next of ``--sets`` weight sets, so that no
call finds its weights in the last-level cache.

``--step``: mixtral_8x7b, prompt 512, B = 1, 4, 8: decode steps with bf16
and with fp8 decode weights alternated in one process on the same caches
(4 warm + 48 timed steps from position 512 each, host clock around a
device synchronise), median [min..max] of three rounds. With ``--router``
every weight kind runs under the "torch" and the "fused" MoE router
(``ops.set_moe_router_impl``), the four alternated.

``--router`` alone: kernel level of the fused router (moe_route.hip),
H 4096, E 8, k 2 at B = 1, 4, 8: ``rmsnorm_res_route`` against the
sequence it replaces (``rmsnorm_res`` + router matmul, ``.float()``,
``topk``, ``softmax``, ``.to``) and against ``rmsnorm_res`` alone,
alternated, device events, median [min..max] of the rounds."""

import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from torchx_amd.ops import hip_ops, quantize_fp8_rows


def time_fn(fn, iters):
    s, e = torch.cuda.Event(True), torch.cuda.Event(True)
    for _ in range(8):
        fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3  # us


def kernel_level(args):
    dev = torch.device("cuda:0")
    hip = hip_ops()
    H, I, E, k = args.hidden, args.inter, 8, 2
    bf = torch.bfloat16
    torch.manual_seed(0)
    sets = []
    for _ in range(args.sets):
        wgu = [0.02 * torch.randn(2 * I, H, device=dev, dtype=bf)
               for _ in range(E)]
        wdown = [0.02 * torch.randn(H, I, device=dev, dtype=bf)
                 for _ in range(E)]
        qgu = [quantize_fp8_rows(w) for w in wgu]
        qdown = [quantize_fp8_rows(w) for w in wdown]
        sets.append((wgu, wdown, [q.w8 for q in qgu], [q.scale for q in qgu],
                     [q.w8 for q in qdown], [q.scale for q in qdown]))
    for B in (1, 4, 8):
        x = torch.randn(B, H, device=dev, dtype=bf)
        w, idx = torch.topk(torch.randn(B, E, device=dev), k, dim=-1)
        cw = torch.softmax(w, dim=-1).to(bf)
        groups = sorted(torch.bincount(idx.flatten(), minlength=E).tolist(),
                        reverse=True)
        active = sum(g > 0 for g in groups)
        h = hip.moe_gemv_swiglu(x, idx, sets[0][0])
        n = [0]

        def nxt():
            n[0] += 1
            return sets[n[0] % len(sets)]

        fns = {
            "A bf16": lambda: hip.moe_gemv_swiglu(x, idx, nxt()[0]),
            "A fp8": lambda: (lambda s: hip.moe_gemv_swiglu_fp8w(
                x, idx, s[2], s[3]))(nxt()),
            "B bf16": lambda: hip.moe_gemv_down_combine(h, idx, cw, nxt()[1]),
            "B fp8 rows=2": lambda: (lambda s: hip.moe_gemv_down_combine_fp8w(
                h, idx, cw, s[4], s[5], 2))(nxt()),
            "B fp8 rows=4": lambda: (lambda s: hip.moe_gemv_down_combine_fp8w(
                h, idx, cw, s[4], s[5], 4))(nxt()),
        }
        ts = {tag: [] for tag in fns}
        for _ in range(args.rounds):
            for tag, fn in fns.items():
                ts[tag].append(time_fn(fn, args.iters))
        print(f"B={B} active experts {active} group sizes {groups[:active]}")
        for tag, t in ts.items():
            t = sorted(t)
            rows = 2 * I if tag[0] == "A" else I
            gb = active * rows * H * (1 if "fp8" in tag else 2) / 1e9
            med = t[len(t) // 2]
            print(f"  {tag:13s} {med:7.1f} us [{t[0]:.1f}..{t[-1]:.1f}]  "
                  f"W {gb:.3f} GB  {gb / med * 1e3:5.2f} TB/s")
    return 0


def router_level(args):
    from torchx_amd import ops

    dev = torch.device("cuda:0")
    H, E, k = args.hidden, 8, 2
    bf = torch.bfloat16
    torch.manual_seed(0)
    w = (0.75 + 0.5 * torch.rand(H, device=dev)).to(bf)
    wr = (0.02 * torch.randn(E, H, device=dev)).to(bf)
    for B in (1, 4, 8):
        x = torch.randn(B, H, device=dev, dtype=bf)
        a = torch.randn(B, H, device=dev, dtype=bf)

        def parent():
            _, y = ops.rmsnorm_res(x, a, w, 1e-5)
            logits = (y @ wr.t()).float()
            v, idx = torch.topk(logits, k, dim=-1)
            return idx, torch.softmax(v, dim=-1).to(bf)

        fns = {
            "rmsnorm_res alone": lambda: ops.rmsnorm_res(x, a, w, 1e-5),
            "rmsnorm_res + torch router": parent,
            "rmsnorm_res_route": lambda: ops.rmsnorm_res_route(
                x, a, w, 1e-5, wr, k),
        }
        ts = {tag: [] for tag in fns}
        for _ in range(args.rounds):
            for tag, fn in fns.items():
                ts[tag].append(time_fn(fn, args.iters))
        print(f"B={B} H={H} E={E} k={k}")
        for tag, t in ts.items():
            t = sorted(t)
            print(f"  {tag:27s} {t[len(t) // 2]:7.2f} us "
                  f"[{t[0]:.2f}..{t[-1]:.2f}]", flush=True)
    return 0


def step_level(args):
    from torchx_amd import ops

    from torchx_amd.models.generate import (
        KVCache, decode_step, prefill, quantize_decode_weights,
    )
    from torchx_amd.models.mixtral import MixtralModel, mixtral_8x7b

    dev = torch.device("cuda:0")
    cfg = mixtral_8x7b()
    torch.manual_seed(0)
    model = quantize_decode_weights(MixtralModel(cfg, device=dev))
    lins = [lin for blk in model.blocks for lin in (
        blk.wqkv, blk.wo, *(w for ex in blk.moe.local_experts
                            for w in (ex.wgu, ex.wdown)))]
    fp8 = [lin.decode_weight for lin in lins]

    def use(mode):  # bf16: the snapped weights, no decode_weight anywhere
        for lin, q in zip(lins, fp8):
            if mode == "fp8":
                lin.decode_weight = q
            elif hasattr(lin, "decode_weight"):
                del lin.decode_weight

    S0, warm, steps = 512, 4, 48
    for B in (1, 4, 8):
        tokens = torch.randint(0, cfg.vocab_size, (B, S0), device=dev)
        caches = [KVCache.empty(cfg, B, S0 + warm + steps + 8, dev)
                  for _ in range(cfg.num_layers)]
        first = prefill(model, tokens, caches).argmax(-1, keepdim=True)
        routers = ("torch", "fused") if args.router else (None,)
        ms = {(wk, r): [] for wk in ("bf16", "fp8") for r in routers}
        for _ in range(3):
            for mode in ms:
                use(mode[0])
                if mode[1] is not None:
                    ops.set_moe_router_impl(mode[1])
                for c in caches:
                    c.length = S0
                nxt = first
                for _ in range(warm):
                    nxt = decode_step(model, nxt, caches).argmax(
                        -1, keepdim=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    nxt = decode_step(model, nxt, caches).argmax(
                        -1, keepdim=True)
                torch.cuda.synchronize()
                ms[mode].append((time.perf_counter() - t0) / steps * 1e3)
        med = {}
        for mode, t in ms.items():
            t = sorted(t)
            med[mode] = t[1]
            tag = mode[0] + (f" router={mode[1]}" if mode[1] else "")
            print(f"B={B} {tag:17s} {t[1]:7.3f} ms/step [{t[0]:.3f}.."
                  f"{t[2]:.3f}]  {B / t[1] * 1e3:7.1f} tok/s", flush=True)
        for r in routers:
            print(f"B={B} fp8 / bf16 time"
                  + (f" router={r}" if r else "")
                  + f" {med['fp8', r] / med['bf16', r]:.3f}", flush=True)
        if args.router:
            for wk in ("bf16", "fp8"):
                print(f"B={B} {wk} fused / torch router time "
                      f"{med[wk, 'fused'] / med[wk, 'torch']:.3f}",
                      flush=True)
    ops.set_moe_router_impl("torch")
    return 0


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--step", action="store_true")
    p.add_argument("--router", action="store_true")
    p.add_argument("--hidden", type=int, default=4096)
    p.add_argument("--inter", type=int, default=14336)
    p.add_argument("--sets", type=int, default=4)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--iters", type=int, default=100)
    args = p.parse_args()
    if args.step:
        return step_level(args)
    return router_level(args) if args.router else kernel_level(args)


if __name__ == "__main__":
    sys.exit(main())
