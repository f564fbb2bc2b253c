#!/usr/bin/env python3
"""Flagship benchmark: Llama-3-8B bf16 training step (the BASELINE.json
headline config: dist.ddp Llama-3-8B, RCCL over xGMI, synthetic data,
random-init weights).

Driver contract:
  python bench.py --gpus N --steps K --warmup W
launched for N>1 as torch.distributed.run with one rank per GPU; reads
RANK/LOCAL_RANK/WORLD_SIZE/MASTER_* from env; rank 0 prints ONE JSON line
with the whole-job aggregate tokens/s.

A plain run sets up, warms up, times K steps and prints that line.
--dump-outputs DIR also writes the last timed step's results as .npy;
--full adds the auxiliary measurements (launch->first-step latency).
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch


DUMP_SAMPLE = 1 << 20  # elements kept per dumped buffer (4 MiB as f32)


def dump_outputs(out_dir: str, loss: float, flat) -> None:
    """Write the last timed step's results as float32 .npy files: the loss
    it returned, and per param group the updated params and the grads it
    left behind.  Buffers larger than DUMP_SAMPLE are sampled at fixed
    seeded positions, so two builds dump the same elements."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "loss.npy"),
            np.asarray([loss], dtype=np.float32))
    for group, p16, grad in flat.groups():
        n = p16.numel()
        idx = None
        if n > DUMP_SAMPLE:
            pos = np.random.default_rng(0).integers(0, n, size=DUMP_SAMPLE)
            idx = torch.from_numpy(np.sort(pos)).to(p16.device)
        for name, buf in (("params", p16), ("grads", grad)):
            sel = buf if idx is None else buf[idx]
            np.save(os.path.join(out_dir, f"{name}_{group}.npy"),
                    sel.detach().float().cpu().numpy())


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--micro-batch", type=int, default=4)
    p.add_argument("--seq-len", type=int, default=4096)
    p.add_argument("--model", type=str, default="llama3_8b",
                   choices=["llama3_8b", "llama3_8b_small", "tiny",
                            "mixtral8x7b", "mixtral_small"])
    p.add_argument("--device", type=str, default=None)
    p.add_argument("--dtype", type=str, default="bf16",
                   choices=["bf16", "fp8"],
                   help="fp8: OCP e4m3/e5m2 GEMMs via hipBLASLt scaled-mm "
                        "(opt-in; the headline metric is bf16)")
    p.add_argument("--zero1", action="store_true",
                   help="ZeRO-1: reduce-scatter grads + sharded optimizer "
                        "state + all-gather params (default: FlatDDP "
                        "bucketed all-reduce)")
    p.add_argument("--hipgraph", type=str, default="off",
                   choices=["auto", "off"],
                   help="capture fwd+bwd in a hipGraph for 1-GPU runs "
                        "(measured neutral: the step is dense big-kernel "
                        "work; kept as an option)")
    p.add_argument("--launch-latency", type=str, default="auto",
                   choices=["auto", "on", "off"],
                   help="also measure launch->first-step latency through the "
                        "full dist.ddp launcher path (the other half of the "
                        "BASELINE metric); auto = on for 1-GPU runs with "
                        "--full")
    p.add_argument("--full", action="store_true",
                   help="also run the auxiliary measurements a plain run "
                        "skips (launch->first-step latency)")
    p.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                   help="after the timed steps, write what the last step "
                        "produced (loss, seeded samples of the updated "
                        "params and of the grads) as DIR/<name>.npy")
    args = p.parse_args()

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))

    use_gpu = torch.cuda.is_available() and args.device != "cpu"
    if use_gpu:
        # modulo: >1 ranks may share a device (single-GPU RCCL de-risk tests)
        dev_idx = local_rank % torch.cuda.device_count()
        torch.cuda.set_device(dev_idx)
        device = torch.device("cuda", dev_idx)
        # bind this rank's host threads to its GPU's NUMA node (the same
        # affinity the agent gives launched workers; best-effort)
        try:
            from torchx_amd.schedulers.devices import (
                numa_cpulist, numa_node_of, parse_cpulist,
            )

            cpus = parse_cpulist(numa_cpulist(numa_node_of(str(dev_idx))))
            if cpus:
                os.sched_setaffinity(0, cpus)
        except Exception:  # noqa: BLE001
            pass
        backend = "nccl"  # RCCL on ROCm
        # tuned hipBLASLt algorithm table (tools/gemm_tune.py), read-only
        tuned = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                             "torchx_amd", "ops", "tunableop_gfx950.csv")
        if os.path.exists(tuned):
            torch.cuda.tunable.enable(True)
            torch.cuda.tunable.tuning_enable(False)
            torch.cuda.tunable.read_file(tuned)
    else:
        device = torch.device("cpu")
        backend = "gloo"

    distributed = world > 1
    if distributed:
        import torch.distributed as dist

        dist.init_process_group(backend=backend)

    from torchx_amd.models.llama import (
        LlamaConfig, LlamaModel, llama3_8b, llama_tiny,
    )
    from torchx_amd.models.mixtral import MixtralConfig, MixtralModel, mixtral_8x7b
    from torchx_amd.parallel import FlatAdamW, FlatDDP, FlatParams

    is_moe = args.model.startswith("mixtral")
    if args.model == "llama3_8b":
        cfg = llama3_8b()
    elif args.model == "llama3_8b_small":
        cfg = LlamaConfig(num_layers=4)  # 8B shape, 4 layers (debug)
    elif args.model == "mixtral8x7b":
        cfg = mixtral_8x7b()
    elif args.model == "mixtral_small":
        cfg = MixtralConfig(num_layers=4)  # 8x7B shape, 4 layers (debug)
    else:
        cfg = llama_tiny()
        args.seq_len = min(args.seq_len, cfg.max_seq_len)
        args.micro_batch = 2

    cfg.max_seq_len = max(cfg.max_seq_len, args.seq_len)
    torch.manual_seed(1234 + rank)

    if use_gpu:
        from torchx_amd import ops

        ops.hip_ops(required=True)  # fail loudly if the extension is missing

    if is_moe:
        # expert parallelism over the whole job when it divides the
        # expert count (BASELINE config 5: EP all-to-all over xGMI);
        # expert params are EP-sharded -> excluded from the DP all-reduce
        ep_size = world if (world > 1 and cfg.num_experts % world == 0) else 1
        if use_gpu and args.model == "mixtral8x7b":
            # optimizer states are 16 B/param (bf16 p+g, fp32 p32/m/v):
            # 47B params need ~750 GB total -> at least EP4 on 288 GB GPUs
            params_b = 47e9 / max(ep_size, 1) + 2e9
            need_gb = params_b * 16 / 1e9
            if need_gb > 250:
                print(f"mixtral8x7b needs ~{need_gb:.0f} GB/GPU for "
                      f"optimizer state at ep_size={ep_size}; run with >=4 "
                      f"GPUs (EP-sharded) or use --model mixtral_small",
                      file=sys.stderr)
                return 2
        model = MixtralModel(cfg, device=device, ep_group=None,
                             ep_size=ep_size, ep_rank=rank % ep_size)

        def group_fn(name, param):
            if ep_size > 1 and "local_experts" in name:
                return "expert"
            return "decay" if param.dim() >= 2 else "no_decay"

        flat = FlatParams(model, device, group_fn=group_fn)
        ddp = FlatDDP(flat, local_groups={"expert"})
    else:
        model = LlamaModel(cfg, device=device)
        if args.dtype == "fp8":
            from torchx_amd.parallel import convert_to_fp8

            convert_to_fp8(model)
        flat = FlatParams(model, device)
        ddp = FlatDDP(flat) if not args.zero1 else None
    if args.zero1 and not is_moe:
        from torchx_amd.parallel import FlatZeRO1

        opt = FlatZeRO1(flat, lr=3e-4)
        ddp = opt  # .finish() is a no-op; reduction happens in step()
    else:
        opt = FlatAdamW(flat, lr=3e-4)

    B, S = args.micro_batch, args.seq_len
    # rotating pool of synthetic batches (pre-generated: no per-step host
    # work in the timed region; >1 batch so the loss is not pure
    # single-batch memorization)
    n_batches = 4
    batch_pool = [torch.randint(0, cfg.vocab_size, (B, S), device=device)
                  for _ in range(n_batches)]
    target_pool = [torch.roll(t, shifts=-1, dims=1) for t in batch_pool]
    step_i = [0]

    def one_step() -> float:
        i = step_i[0] % n_batches
        step_i[0] += 1
        opt.zero_grad()
        loss = model(batch_pool[i], target_pool[i])
        loss.backward()
        ddp.finish()
        opt.step()
        return float(loss.detach())

    # warmup (eager)
    for _ in range(args.warmup):
        one_step()

    # hipGraph capture of fwd+bwd for the single-GPU run: ~1300 kernel
    # launches per step replay from one graph, removing per-launch gaps.
    # The optimizer + zero_grad stay eager (host-computed bias correction
    # must keep evolving per step); multi-rank runs stay eager (RCCL
    # collectives + bucket hooks).  Full work per step is unchanged.
    if use_gpu and not distributed and args.hipgraph != "off":
        try:
            static_tokens = batch_pool[0].clone()
            static_targets = target_pool[0].clone()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            opt.zero_grad()
            with torch.cuda.graph(graph):
                cap_loss = model(static_tokens, static_targets)
                cap_loss.backward()
            torch.cuda.synchronize()

            def one_step() -> float:  # noqa: F811 — graph-backed step
                i = step_i[0] % n_batches
                step_i[0] += 1
                static_tokens.copy_(batch_pool[i])
                static_targets.copy_(target_pool[i])
                opt.zero_grad()
                graph.replay()
                ddp.finish()
                opt.step()
                return float(cap_loss.detach())

            one_step()  # re-warm once through the graph path
        except Exception as e:  # noqa: BLE001 — graphs are an optimization
            print(f"hipGraph capture failed, staying eager: {e}",
                  file=sys.stderr)

    if distributed:
        import torch.distributed as dist

        dist.barrier()
    if use_gpu:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    loss = 0.0
    for _ in range(args.steps):
        loss = one_step()
    if use_gpu:
        torch.cuda.synchronize()
    if distributed:
        import torch.distributed as dist

        dist.barrier()
    elapsed = time.perf_counter() - t0

    # MAX over ranks
    if distributed:
        import torch.distributed as dist

        t = torch.tensor([elapsed], device=device if use_gpu else None,
                         dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    ms_per_step = elapsed / args.steps * 1000.0
    tokens_per_step = B * S * world
    tok_s = tokens_per_step / (elapsed / args.steps)
    peak_hbm_gb = (round(torch.cuda.max_memory_allocated() / 1e9, 2)
                   if use_gpu else None)

    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, loss, flat)

    # launch->first-step latency (the other half of the BASELINE metric):
    # the full dist.ddp launcher path — materialize -> Popen -> agent ->
    # c10d rendezvous -> RCCL init -> first fwd+bwd+step (1x1, gpu_tiny)
    launch_latency = None
    measure_latency = (args.launch_latency == "on"
                       or (args.launch_latency == "auto" and args.full
                           and world == 1 and use_gpu))
    if measure_latency and rank == 0:
        try:
            # free the bench model's HBM first so the spawned trainer and
            # this process never contend for memory
            # free what we can (the spawned gpu_tiny trainer needs ~2 GB;
            # 288 GB HBM fits both either way)
            model = flat = ddp = opt = batch_pool = target_pool = None
            one_step = None
            if use_gpu:
                torch.cuda.empty_cache()
            from torchx_amd.utils.launch_latency import measure_launch_latency

            launch_latency = measure_launch_latency(nproc=1, timeout=180.0)
        except Exception as e:  # noqa: BLE001 — latency is auxiliary
            print(f"launch-latency measurement failed: {e}", file=sys.stderr)

    if rank == 0:
        result = {
            "metric": "tokens_per_second",
            "value": tok_s,
            "unit": "tokens/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": args.dtype,
            "data": "synthetic",
            "config": {
                "model": args.model,
                "global_batch": B * world,
                "seq_len": S,
                "parallelism": (f"dp{world}_ep{world}" if is_moe and world > 1 else f"dp{world}"),
                "final_loss": loss,
            },
        }
        if peak_hbm_gb is not None:
            result["peak_hbm_gb"] = peak_hbm_gb
        if launch_latency is not None:
            result["launch_to_first_step_s"] = launch_latency["value"]
            result["launch_submit_s"] = launch_latency["submit_seconds"]
        print(json.dumps(result), flush=True)

    if distributed:
        import torch.distributed as dist

        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
