#!/usr/bin/env python3
"""Serving benchmark: prefill + KV-cache decode throughput for
Llama-3-8B on one MI355X (random weights, synthetic prompt)."""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def run_batcher(args, model, tokens):
    """Admit the rows one at a time through PagedBatcher (time to first
    token per admit, by device events), then time the ragged decode."""
    from torchx_amd.models.generate import PagedBatcher

    B, S0 = tokens.shape
    N, P = args.new, args.page_size
    shared = args.shared_prefix
    if shared is not None:
        assert 0 <= shared <= S0
        tokens[:, :shared] = tokens[0, :shared]
    max_len = S0 + N + 8

    def batcher():
        return PagedBatcher(model, B, max_len, B * -(-max_len // P) + 1, P,
                            prefix_sharing=shared is not None,
                            prefill_chunk=args.prefill_chunk)

    # warm every prefill shape (hipBLASLt algo selection) on a batcher
    # that is thrown away, then time on a fresh one
    warm = batcher()
    for b in range(B):
        warm.admit(b, tokens[b])
    del warm
    torch.cuda.synchronize()
    pb = batcher()
    free0 = pb.free_pages()
    ttft = []
    for b in range(B):
        start = torch.cuda.Event(enable_timing=True)
        stop = torch.cuda.Event(enable_timing=True)
        start.record()
        pb.admit(b, tokens[b])
        stop.record()
        torch.cuda.synchronize()
        ttft.append(start.elapsed_time(stop))
    pages_prefill = free0 - pb.free_pages()
    for _ in range(4):
        pb.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(N - 4):
        pb.step()
    torch.cuda.synchronize()
    t_dec = time.perf_counter() - t0
    print(json.dumps({
        "metric": "decode_tokens_per_second",
        "value": B * (N - 4) / t_dec,
        "ms_per_decode_step": t_dec / (N - 4) * 1e3,
        "ttft_ms_per_admit": [round(t, 3) for t in ttft],
        "shared_tokens": list(pb.shared_tokens),
        "pages_in_use_after_prefill": pages_prefill,
        "pages_in_use": free0 - pb.free_pages(),
        "pages_unshared": B * -(-(S0 + N) // P),
        "batch": B, "prompt": S0, "new_tokens": N,
        "model": args.model, "dtype": "bf16", "data": "synthetic",
        "kv_cache": "paged", "page_size": P, "batcher": True,
        "prefill_chunk": args.prefill_chunk, "shared_prefix": shared,
    }))
    return 0


def _spread(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def run_admit_many(args, model, tokens, rounds=5):
    """Time to first token of all rows: one ``admit_many`` call against
    the one-at-a-time ``admit`` loop and, for scale, the dense [B, S]
    ``prefill``. Each is warmed on throw-away state, then the three
    alternate within every round on fresh batchers; device-event times,
    median and [min..max] over the rounds. Then the ragged decode of the
    last ``admit_many`` batcher is timed as ``run_batcher`` does."""
    from torchx_amd.models.generate import KVCache, PagedBatcher, prefill

    B, S0 = tokens.shape
    N, P = args.new, args.page_size
    shared = args.shared_prefix
    if shared is not None:
        assert 0 <= shared <= S0
        tokens[:, :shared] = tokens[0, :shared]
    max_len = S0 + N + 8
    rows = list(range(B))
    prompts = [tokens[b] for b in rows]

    def batcher():
        return PagedBatcher(model, B, max_len, B * -(-max_len // P) + 1, P,
                            prefix_sharing=shared is not None,
                            prefill_chunk=args.prefill_chunk)

    def timed(fn):
        start = torch.cuda.Event(enable_timing=True)
        stop = torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop)

    def many(pb):
        return lambda: pb.admit_many(rows, prompts)

    def loop(pb):
        def go():
            for b in rows:
                pb.admit(b, prompts[b])
        return go

    def dense():
        caches = [KVCache.empty(model.cfg, B, max_len, tokens.device)
                  for _ in range(model.cfg.num_layers)]
        return lambda: prefill(model, tokens, caches)

    for make in (many, loop):                    # warm both (GEMM shapes)
        make(batcher())()
    dense()()
    torch.cuda.synchronize()
    t_many, t_loop, t_dense = [], [], []
    pb = None
    for _ in range(rounds):
        del pb
        t_loop.append(timed(loop(batcher())))
        t_dense.append(timed(dense()))
        pb = batcher()
        free0 = pb.free_pages()
        t_many.append(timed(many(pb)))
    pages_prefill = free0 - pb.free_pages()
    for _ in range(4):
        pb.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(N - 4):
        pb.step()
    torch.cuda.synchronize()
    t_dec = time.perf_counter() - t0

    def stats(ts):
        med, lo, hi = _spread(ts)
        return {"ms": round(med, 3), "ms_min": round(lo, 3),
                "ms_max": round(hi, 3),
                "prefill_tokens_per_second": round(B * S0 / med * 1e3)}

    print(json.dumps({
        "metric": "decode_tokens_per_second",
        "value": B * (N - 4) / t_dec,
        "ms_per_decode_step": t_dec / (N - 4) * 1e3,
        "ttft_admit_many": stats(t_many),
        "ttft_admit_loop": stats(t_loop),
        "ttft_dense_prefill": stats(t_dense),
        "admit_many_speedup": round(_spread(t_loop)[0] / _spread(t_many)[0],
                                    3),
        "rounds": rounds,
        "shared_tokens": list(pb.shared_tokens),
        "pages_in_use_after_prefill": pages_prefill,
        "pages_in_use": free0 - pb.free_pages(),
        "batch": B, "prompt": S0, "new_tokens": N,
        "model": args.model, "dtype": "bf16", "data": "synthetic",
        "kv_cache": "paged", "page_size": P, "batcher": True,
        "admit_many": True,
        "prefill_chunk": args.prefill_chunk, "shared_prefix": shared,
    }))
    return 0


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="llama3_8b",
                   choices=["llama3_8b", "gpu_tiny", "mixtral_8x7b",
                            "mixtral_gpu_tiny"])
    p.add_argument("--batch", type=int, default=4)
    p.add_argument("--prompt", type=int, default=512)
    p.add_argument("--new", type=int, default=128)
    p.add_argument("--graph", action="store_true",
                   help="hipGraph decode loop (whole step as one replay)")
    p.add_argument("--paged", action="store_true",
                   help="decode through paged KV caches (block-table "
                        "kernels) instead of dense [B, T] slabs")
    p.add_argument("--page-size", type=int, default=16,
                   help="tokens per page with --paged (power of two, "
                        "16..256)")
    p.add_argument("--batcher", action="store_true",
                   help="with --paged: admit the rows one at a time through "
                        "PagedBatcher and report the time to first token "
                        "of every admit and the pages in use")
    p.add_argument("--prefill-chunk", type=int, default=None,
                   help="implies --batcher: prefill in pieces of at most N "
                        "tokens (paged prefill attention)")
    p.add_argument("--shared-prefix", type=int, default=None,
                   help="implies --batcher with prefix sharing on: all "
                        "prompts begin with the same N tokens")
    p.add_argument("--admit-many", action="store_true",
                   help="implies --batcher: admit all rows in ONE "
                        "admit_many call (packed ragged prefill) and report "
                        "its time next to the one-at-a-time loop and the "
                        "dense prefill, alternated in this process")
    args = p.parse_args()
    if args.admit_many:
        args.batcher = True
    if args.paged and args.graph:
        print("--paged has no hipGraph loop", file=sys.stderr)
        return 1
    if args.prefill_chunk is not None or args.shared_prefix is not None:
        args.batcher = True
    if args.batcher and not args.paged:
        print("--batcher, --prefill-chunk, --shared-prefix and --admit-many "
              "need --paged", file=sys.stderr)
        return 1

    from torchx_amd.models.generate import (
        KVCache, PagedKVCache, decode_step, prefill,
    )
    from torchx_amd.models.llama import LlamaModel, llama3_8b, llama_gpu_tiny

    dev = torch.device("cuda:0")
    moe = args.model.startswith("mixtral")
    if moe:
        from torchx_amd.models.mixtral import (
            MixtralModel, mixtral_8x7b, mixtral_gpu_tiny,
        )

        if args.graph:
            print("--graph is dense-only (MoE routing is data-dependent)",
                  file=sys.stderr)
            return 1
        cfg = (mixtral_8x7b() if args.model == "mixtral_8x7b"
               else mixtral_gpu_tiny())
        torch.manual_seed(0)
        model = MixtralModel(cfg, device=dev)
    else:
        cfg = llama3_8b() if args.model == "llama3_8b" else llama_gpu_tiny()
        torch.manual_seed(0)
        model = LlamaModel(cfg, device=dev)
    B, S0, N = args.batch, args.prompt, args.new
    tokens = torch.randint(0, cfg.vocab_size, (B, S0), device=dev)
    if args.batcher:
        if args.admit_many:
            return run_admit_many(args, model, tokens)
        return run_batcher(args, model, tokens)
    if args.paged:
        # every sequence gets M pages; the table is a seeded permutation
        # of the physical pages so they are not accidentally contiguous
        P = args.page_size
        M = -(-(S0 + N + 8) // P)
        g = torch.Generator().manual_seed(0)
        table = (torch.randperm(B * M, generator=g) + 1).to(torch.int32)
        table = table.reshape(B, M).to(dev)
        caches = [PagedKVCache.empty(cfg, B * M + 1, P, table, dev)
                  for _ in range(cfg.num_layers)]
        pos = torch.full((B,), S0, dtype=torch.int32, device=dev)
        dense_step = decode_step

        def decode_step(model, tok, caches):  # noqa: F811
            logits = dense_step(model, tok, caches, pos_dev=pos)
            pos.add_(1)
            return logits
    else:
        caches = [KVCache.empty(cfg, B, S0 + N + 8, dev)
                  for _ in range(cfg.num_layers)]

    # warm prefill once (hipBLASLt algo selection etc.), then re-time it
    # on fresh caches so the printed number is the steady-state rate
    warm = [KVCache.empty(cfg, B, S0 + N + 8, dev)
            for _ in range(cfg.num_layers)]
    prefill(model, tokens, warm)
    del warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    logits = prefill(model, tokens, caches)
    torch.cuda.synchronize()
    t_prefill = time.perf_counter() - t0

    nxt = logits.argmax(-1, keepdim=True)
    steps = N
    if args.graph:
        from torchx_amd.models.generate import GraphedDecoder

        dec = GraphedDecoder(model, caches, B, nxt, start_pos=S0)
        for _ in range(2):
            dec.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            dec.step()
        torch.cuda.synchronize()
        t_dec = time.perf_counter() - t0
    else:
        # warm a few decode steps, then time
        for _ in range(4):
            nxt = decode_step(model, nxt, caches).argmax(-1, keepdim=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            nxt = decode_step(model, nxt, caches).argmax(-1, keepdim=True)
        torch.cuda.synchronize()
        t_dec = time.perf_counter() - t0

    print(json.dumps({
        "metric": "decode_tokens_per_second",
        "value": B * steps / t_dec,
        "ms_per_decode_step": t_dec / steps * 1e3,
        "prefill_tokens_per_second": B * S0 / t_prefill,
        "batch": B, "prompt": S0, "new_tokens": steps,
        "model": args.model, "dtype": "bf16", "data": "synthetic", "graphed": bool(args.graph),
        "kv_cache": "paged" if args.paged else "dense",
        "page_size": args.page_size if args.paged else None,
    }))
    return 0


if __name__ == "__main__":
    sys.exit(main())
