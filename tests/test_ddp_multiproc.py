"""Multi-process (gloo, world_size=2) tests of the data-parallel training
path — the same code bench.py runs per rank on RCCL."""

import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.subprocess_heavy

REPO = Path(__file__).resolve().parent.parent

WORKER = r"""
import os, sys
sys.path.insert(0, %(repo)r)
import torch
import torch.distributed as dist
from torchx_amd.models.llama import llama_tiny, LlamaModel
from torchx_amd.parallel import FlatParams, FlatDDP, FlatAdamW

dist.init_process_group("gloo")
rank = dist.get_rank()
torch.manual_seed(42)  # same init on all ranks (FlatDDP also broadcasts)

cfg = llama_tiny()
model = LlamaModel(cfg)
flat = FlatParams(model, torch.device("cpu"))
ddp = FlatDDP(flat, bucket_bytes=1 << 18)
opt = FlatAdamW(flat, lr=1e-3)

# different data per rank
torch.manual_seed(100 + rank)
tokens = torch.randint(0, cfg.vocab_size, (2, 64))
targets = torch.randint(0, cfg.vocab_size, (2, 64))

for step in range(3):
    opt.zero_grad()
    loss = model(tokens, targets)
    loss.backward()
    ddp.finish()
    # grads must now be identical across ranks
    g = flat.flat_grad["decay"]
    gsum = g.float().sum()
    t = gsum.clone()
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    assert torch.allclose(gsum, t, rtol=1e-4), (gsum, t)
    opt.step()

# params identical across ranks after steps
p = flat.flat_p16["decay"].float().sum()
t = p.clone()
dist.all_reduce(t, op=dist.ReduceOp.MAX)
assert torch.allclose(p, t, rtol=1e-4), (p, t)
if rank == 0:
    print("DDP_MULTIPROC_OK", flush=True)
dist.destroy_process_group()
"""


def test_flatddp_gloo_world2(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(WORKER % {"repo": str(REPO)})
    env = {
        **os.environ,
        "MASTER_ADDR": "127.0.0.1",
        "MASTER_PORT": "0",
    }
    # launch via our own agent (also exercises the agent on a real payload)
    proc = subprocess.run(
        [
            sys.executable, "-m", "torchx_amd.agent",
            "--nnodes", "1", "--nproc-per-node", "2",
            "--rdzv-endpoint", "127.0.0.1:0",
            "--rdzv-id", "test_ddp", "--max-restarts", "0",
            str(script),
        ],
        cwd=str(REPO),
        env=env,
        capture_output=True,
        timeout=300,
    )
    out = proc.stdout.decode() + proc.stderr.decode()
    assert proc.returncode == 0, out[-4000:]
    assert "DDP_MULTIPROC_OK" in out, out[-4000:]


DIRECT_GRAD_WORKER = r"""
import os, sys
sys.path.insert(0, %(repo)r)
import torch
import torch.distributed as dist
from torchx_amd.models.llama import llama_tiny, LlamaModel
from torchx_amd.parallel import FlatParams, FlatDDP, FlatAdamW
from torchx_amd.parallel.ddp import grad_ready

dist.init_process_group("gloo")
rank = dist.get_rank()
torch.manual_seed(7)

cfg = llama_tiny()
model = LlamaModel(cfg)
flat = FlatParams(model, torch.device("cpu"))
ddp = FlatDDP(flat, bucket_bytes=1 << 18)
opt = FlatAdamW(flat, lr=1e-3)

# simulate fast_linear's DIRECT grad production: write each param's grad
# slot in place (rank-dependent) and notify the bucket hook manually —
# torch's post-accumulate hook never fires on this path
opt.zero_grad()
for slot in flat.slots:
    p = slot.param
    with torch.no_grad():
        p.grad.add_(torch.full_like(p, float(rank + 1)))
    grad_ready(p)
ddp.finish()

# after finish, every grad must be the cross-rank mean: (1+2)/2 = 1.5
for slot in flat.slots:
    g = slot.param.grad.float()
    assert torch.allclose(g, torch.full_like(g, 1.5), atol=1e-2), (
        slot.name if hasattr(slot, "name") else "param", g.mean())
if rank == 0:
    print("DIRECT_GRAD_OK", flush=True)
dist.destroy_process_group()
"""


def test_direct_grad_ready_bucket_path(tmp_path):
    """grad_ready() (the manual bucket notification fast_linear's direct
    wgrad accumulation uses) drives the same bucketed all-reduce as the
    torch post-accumulate hook — exactly what the 8-GPU run exercises."""
    script = tmp_path / "worker.py"
    script.write_text(DIRECT_GRAD_WORKER % {"repo": str(REPO)})
    env = dict(os.environ)
    env["PYTHONPATH"] = str(REPO) + os.pathsep + env.get("PYTHONPATH", "")
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes", "1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--standalone", str(script)],
        env=env, capture_output=True, text=True, timeout=300, cwd=str(REPO),
    )
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "DIRECT_GRAD_OK" in out.stdout + out.stderr


ZERO1_WORKER = r"""
import os, sys
sys.path.insert(0, %(repo)r)
import torch
import torch.distributed as dist
from torchx_amd.models.llama import llama_tiny, LlamaModel
from torchx_amd.parallel import FlatAdamW, FlatDDP, FlatParams, FlatZeRO1

dist.init_process_group("gloo")
rank = dist.get_rank()
ws = dist.get_world_size()

def build():
    torch.manual_seed(42)
    cfg = llama_tiny()
    model = LlamaModel(cfg)
    flat = FlatParams(model, torch.device("cpu"))
    return cfg, model, flat

def data(step):
    torch.manual_seed(500 + 10 * step + rank)  # different per rank
    cfg = llama_tiny()
    t = torch.randint(0, cfg.vocab_size, (2, 64))
    return t, torch.randint(0, cfg.vocab_size, (2, 64))

# --- reference: FlatDDP + full FlatAdamW ---
cfg, model, flat = build()
ddp = FlatDDP(flat, bucket_bytes=1 << 18)
opt = FlatAdamW(flat, lr=1e-3)
for s in range(2):
    opt.zero_grad()
    tok, tgt = data(s)
    model(tok, tgt).backward()
    ddp.finish()
    opt.step()
ref_p16 = {g: p.clone() for g, p, _ in flat.groups()}

# --- ZeRO-1 on identical init/data ---
cfg, model, flat = build()
z = FlatZeRO1(flat, lr=1e-3)
assert z.enabled and z.ws == ws
for s in range(2):
    z.zero_grad()
    tok, tgt = data(s)
    model(tok, tgt).backward()
    z.step()

for g, p16, _ in flat.groups():
    n = p16.numel()
    # sharded state is 1/ws of the group
    assert z.state[g]["p32"].numel() == n // ws, (g, n)
    diff = (p16.float() - ref_p16[g].float()).abs().max().item()
    assert diff < 1e-2, (g, diff)
    # params identical across ranks after the all-gather
    other = p16.clone()
    dist.broadcast(other, src=0)
    assert torch.equal(other, p16), g

# consolidation: gather both shards' state dicts and merge -> must match
# the full FlatAdamW state from the reference run
sd = z.state_dict()
gathered = [None, None]
dist.all_gather_object(gathered, sd)
full = FlatZeRO1.consolidate(gathered)
for g, st in opt.state.items():
    for k in ("p32", "m", "v"):
        d = (full["state"][g][k] - st[k]).abs().max().item()
        assert d < 1e-2, (g, k, d)

if rank == 0:
    print("ZERO1_OK", flush=True)
dist.destroy_process_group()
"""


def test_zero1_matches_ddp_adamw(tmp_path):
    """ZeRO-1 (reduce-scatter + sharded optimizer + all-gather) produces
    the same parameters as FlatDDP + full-state FlatAdamW, with 1/ws the
    optimizer state, and ranks stay bit-identical."""
    script = tmp_path / "worker.py"
    script.write_text(ZERO1_WORKER % {"repo": str(REPO)})
    env = dict(os.environ)
    env["PYTHONPATH"] = str(REPO) + os.pathsep + env.get("PYTHONPATH", "")
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes", "1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--standalone", str(script)],
        env=env, capture_output=True, text=True, timeout=300, cwd=str(REPO),
    )
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "ZERO1_OK" in out.stdout + out.stderr


def test_zero1_single_process_degenerates_to_adamw():
    import torch

    from torchx_amd.models.llama import LlamaModel, llama_tiny
    from torchx_amd.parallel import FlatParams, FlatZeRO1

    torch.manual_seed(1)
    cfg = llama_tiny()
    model = LlamaModel(cfg)
    flat = FlatParams(model, torch.device("cpu"))
    z = FlatZeRO1(flat, lr=1e-3)
    assert not z.enabled
    tok = torch.randint(0, cfg.vocab_size, (2, 64))
    losses = []
    for _ in range(3):
        z.zero_grad()
        loss = model(tok, torch.roll(tok, -1, 1))
        loss.backward()
        z.step()
        losses.append(float(loss.detach()))
    assert losses[-1] < losses[0]


def test_agent_two_nodes(tmp_path):
    """Two agent processes (nnodes=2) rendezvous and form one world of 4
    (the multi-node path of the launcher, on one host via 127.0.0.1)."""
    import socket
    import time

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]

    env = dict(os.environ)
    env["PYTHONPATH"] = str(REPO) + os.pathsep + env.get("PYTHONPATH", "")
    procs = []
    for node in range(2):
        procs.append(subprocess.Popen(
            [sys.executable, "-m", "torchx_amd.agent",
             "--nnodes", "2:2", "--nproc-per-node", "2",
             "--rdzv-endpoint", f"127.0.0.1:{port}",
             "--rdzv-id", "twonode", "--log-dir", str(tmp_path / str(node)),
             "--no-python", sys.executable, "-m",
             "torchx_amd.apps.compute_world_size"],
            env=env, cwd=str(REPO),
            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
        ))
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=240)
        except subprocess.TimeoutExpired:
            p.kill()
            out, _ = p.communicate()
        outs.append(out)
    assert all(p.returncode == 0 for p in procs), outs
    assert any("computed world size = 4" in o for o in outs), outs


def test_bench_contract_world2_cpu(tmp_path):
    """The driver's bench invocation shape (torch.distributed.run, one rank
    per device) must work end to end and print ONE valid JSON line."""
    env = dict(os.environ)
    env["PYTHONPATH"] = str(REPO) + os.pathsep + env.get("PYTHONPATH", "")
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes", "1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--standalone", str(REPO / "bench.py"),
         "--gpus", "2", "--steps", "2", "--warmup", "1",
         "--model", "tiny", "--device", "cpu"],
        env=env, cwd=str(REPO), capture_output=True, text=True, timeout=300,
    )
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    result = json.loads(line)
    assert result["metric"] == "tokens_per_second"
    assert result["n_gpus"] == 2
    assert result["value"] > 0
    assert result["config"]["parallelism"] == "dp2"


def _bench_tiny_cpu(*extra):
    env = dict(os.environ)
    env["PYTHONPATH"] = str(REPO) + os.pathsep + env.get("PYTHONPATH", "")
    out = subprocess.run(
        [sys.executable, str(REPO / "bench.py"), "--gpus", "1",
         "--steps", "2", "--warmup", "1", "--model", "tiny",
         "--device", "cpu", *extra],
        env=env, cwd=str(REPO), capture_output=True, text=True, timeout=300,
    )
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_bench_dump_outputs_reproducible(tmp_path):
    """--dump-outputs writes the last timed step's results as float .npy
    files, and two runs with the same arguments dump the same arrays."""
    import numpy as np

    dumps = []
    for name in ("a", "b"):
        out_dir = tmp_path / name
        result = _bench_tiny_cpu("--dump-outputs", str(out_dir))
        assert result["steps"] == 2
        assert result["ms_per_step"] > 0
        # a plain run carries no auxiliary measurement
        assert "launch_to_first_step_s" not in result
        arrays = {f.stem: np.load(f) for f in sorted(out_dir.glob("*.npy"))}
        assert {"loss", "params_decay", "grads_decay"} <= set(arrays)
        for arr in arrays.values():
            assert arr.dtype in (np.float32, np.float64)
            assert np.isfinite(arr).all()
        assert arrays["loss"][0] == np.float32(result["config"]["final_loss"])
        assert np.abs(arrays["grads_decay"]).max() > 0
        assert sum(a.nbytes for a in arrays.values()) <= 64 * 2**20
        dumps.append(arrays)
    assert dumps[0].keys() == dumps[1].keys()
    for name in dumps[0]:
        np.testing.assert_array_equal(dumps[0][name], dumps[1][name])
