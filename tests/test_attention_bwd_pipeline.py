"""Attention backward, merged dK/dV kernel: the rotated software pipeline.

The tile body runs one 32-q sub-tile per step and carries state from step
to step: S/dP of the next sub-tile and the P/dS fragments of the previous
one, whose accumulate MFMAs ride under the current sub-tile's softmax
VALU.  The pipeline fills and drains at every tile boundary.  What such a
body can get wrong is a stale carried fragment, a sub-tile accumulated
twice or dropped at a seam, or state leaking from one head of a GQA group
to the next.  None of these is a rounding difference, and the split kernel
is the bit reference, so every case asserts

  * dq, dk and dv are torch.equal between merged and split, in both dQ
    modes (the dQ kernels consume the dS the dkv kernel exports), and
  * two merged runs equal each other.

Cases (D = 128, bf16, B <= 2, seeded normal inputs):
  S=32, S=64 causal Hq4/Hkv4    fewer sub-tiles than the pipeline is deep:
                                fill and drain only (TFKV=64 instance)
  S=512 causal Hq8/Hkv2 B=1     G=4, four tiles per block at kt=0: the
                                seam between tiles and between the G heads
                                of one block
  S=512 full Hq8/Hkv2           no masked instance, every tile full
  S=416 causal Hq4/Hkv2         3*128+32: TFKV=64 instance, last tile has
                                one valid sub-tile, export skipped past S
  S=129 causal Hq4/Hkv4 B=2     one valid row in the last tile; B*Hkv = 8,
                                the XCD-swizzled block map
  S=384 causal Hq6/Hkv3 B=1     B*Hkv % 8 != 0, the linear map; G=2
  S=256 causal Hq4/Hkv4, q and dO of head h scaled by 2^h
                                a fragment carried over from the previous
                                head is at least 2x off

The staged-tile size (TORCHX_AMD_DKV_FKV) is latched at the first backward
call of a process, so a fresh child process runs the S=512 causal case
once through the 64-row instance.
"""

import math
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

D = 128
REPO = Path(__file__).resolve().parent.parent

# (id, B, S, causal, Hq, Hkv, scale heads by 2^h)
CASES = [
    ("S32-causal-h4x4", 2, 32, True, 4, 4, False),
    ("S64-causal-h4x4", 2, 64, True, 4, 4, False),
    ("S512-causal-h8x2-b1", 1, 512, True, 8, 2, False),
    ("S512-full-h8x2", 2, 512, False, 8, 2, False),
    ("S416-causal-h4x2", 2, 416, True, 4, 2, False),
    ("S129-causal-h4x4", 2, 129, True, 4, 4, False),
    ("S384-causal-h6x3-b1", 1, 384, True, 6, 3, False),
    ("S256-causal-h4x4-headscaled", 2, 256, True, 4, 4, True),
]
IDS = [c[0] for c in CASES]
DQ_MODES = ["stream", "recompute"]


def _inputs(dev, B, S, Hq, Hkv, head_scaled, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    q = torch.randn(B, S, Hq, D, device=dev, generator=gen)
    k = torch.randn(B, S, Hkv, D, device=dev, generator=gen)
    v = torch.randn(B, S, Hkv, D, device=dev, generator=gen)
    do = torch.randn(B, S, Hq, D, device=dev, generator=gen)
    if head_scaled:
        w = (2.0 ** torch.arange(Hq, device=dev)).view(1, 1, Hq, 1)
        q, do = q * w, do * w
    return q.bfloat16(), k.bfloat16(), v.bfloat16(), do.bfloat16()


def _run_variants(ops, hip, q, k, v, do, causal):
    """(dq, dk, dv) keyed by (variant, dq mode) for a merged run, a second
    merged run and a split run."""
    scale = 1.0 / math.sqrt(D)
    o, lse = hip.attn_fwd(q, k, v, scale, causal)
    res = {}
    for mode in DQ_MODES:
        ops.set_attn_bwd_dq_mode(mode)
        for name, impl in (("merged", "merged"), ("merged2", "merged"),
                           ("split", "split")):
            ops.set_attn_bwd_dkv_impl(impl)
            res[name, mode] = hip.attn_bwd(q, k, v, o, do, lse, scale, causal)
    return res


@pytest.fixture(scope="module")
def runs():
    """Per case the results of _run_variants; computed once, never
    modified."""
    assert torch.cuda.is_available()
    from torchx_amd import ops

    assert ops.extension_available(), "HIP extension must be built in-tree"
    hip = ops.hip_ops(required=True)
    dev = torch.device("cuda:0")
    initial_impl = ops.get_attn_bwd_dkv_impl()
    initial_mode = ops.get_attn_bwd_dq_mode()
    out = {}
    try:
        for cid, B, S, causal, Hq, Hkv, head_scaled in CASES:
            q, k, v, do = _inputs(dev, B, S, Hq, Hkv, head_scaled, 2000 + S)
            out[cid] = _run_variants(ops, hip, q, k, v, do, causal)
        torch.cuda.synchronize()
    finally:
        ops.set_attn_bwd_dkv_impl(initial_impl)
        ops.set_attn_bwd_dq_mode(initial_mode)
    return out


@pytest.mark.parametrize("mode", DQ_MODES)
@pytest.mark.parametrize("cid", IDS)
def test_pipeline_bit_identical_to_split(runs, cid, mode):
    r = runs[cid]
    for name, a, b in zip(("dq", "dk", "dv"), r["merged", mode],
                          r["split", mode]):
        assert torch.isfinite(a.float()).all(), f"{name} is not finite"
        assert torch.equal(a, b), f"{name} differs between merged and split"


@pytest.mark.parametrize("mode", DQ_MODES)
@pytest.mark.parametrize("cid", IDS)
def test_pipeline_reproducible(runs, cid, mode):
    r = runs[cid]
    for name, a, b in zip(("dq", "dk", "dv"), r["merged", mode],
                          r["merged2", mode]):
        assert torch.equal(a, b), f"{name} differs between two merged runs"


_CHILD = """
import sys
sys.path.insert(0, {repo!r})
sys.path.insert(0, {tests!r})
import torch
from torchx_amd import ops
import test_attention_bwd_pipeline as t

hip = ops.hip_ops(required=True)
dev = torch.device("cuda:0")
q, k, v, do = t._inputs(dev, 1, 512, 8, 2, False, 2512)
r = t._run_variants(ops, hip, q, k, v, do, True)
torch.cuda.synchronize()
for mode in t.DQ_MODES:
    for name, a, b, c in zip(("dq", "dk", "dv"), r["merged", mode],
                             r["split", mode], r["merged2", mode]):
        assert torch.isfinite(a.float()).all(), name
        assert torch.equal(a, b), (mode, name, "merged != split")
        assert torch.equal(a, c), (mode, name, "merged != merged")
print("fkv64 ok")
"""


def test_pipeline_fkv64_instance_child_process():
    """S=512 causal through the 64-row instance, which S % 128 == 0 only
    reaches with TORCHX_AMD_DKV_FKV=64 set before the first backward."""
    env = dict(os.environ, TORCHX_AMD_DKV_FKV="64")
    code = _CHILD.format(repo=str(REPO), tests=str(REPO / "tests"))
    p = subprocess.run([sys.executable, "-c", code], env=env, cwd=str(REPO),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "fkv64 ok" in p.stdout
