"""Attention backward, merged dK/dV kernel: one wave accumulates both dK
and dV for its 32 kv rows, so S, P and dP are computed once.  It keeps the
split kernel's expressions and accumulation order, so dq, dk and dv must
come out bit-identical to the split kernel in both dQ modes (the dQ
kernels consume the dS it exports), besides meeting the fp32 torch
reference.

Shapes are the smallest that reach each hazard (D = 128, B = 2), the set
of test_attention_bwd_stream.py:
  S=256 causal Hq8/Hkv2   two kv blocks, TFKV=128 instance, linear block
                          map (B*Hkv = 4)
  S=384 causal Hq4/Hkv4   group size 1, XCD-swizzled map (B*Hkv = 8)
  S=192 causal Hq8/Hkv2   S % 128 != 0 -> TFKV=64 instance; partial kv
                          block with two inactive waves (their barrier
                          count in the epilogue must match)
  S=160 causal            q sub-tile starting past the last row
  S=128 non-causal        nothing skipped
  packed S=256 Hq8/Hkv4   fused_attention_qkv: strided dk/dv writes into
                          the one dqkv buffer

The staged-tile size choice (TORCHX_AMD_DKV_FKV) is latched from the
environment at the first backward call of the process, so it cannot be
switched here; the TFKV=64 instance is covered by the S=192 and S=160
cases, which take it whatever the variable says.
"""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

D = 128
B = 2

# (S, causal, Hq, Hkv)
CASES = [
    (256, True, 8, 2),
    (384, True, 4, 4),
    (192, True, 8, 2),
    (160, True, 8, 2),
    (128, False, 8, 2),
]
IDS = [f"S{s}-{'causal' if c else 'full'}-h{hq}x{hkv}"
       for s, c, hq, hkv in CASES]
DQ_MODES = ["stream", "recompute"]


def _ops():
    from torchx_amd import ops

    assert ops.extension_available(), "HIP extension must be built in-tree"
    return ops


def rel_err(a, b):
    a, b = a.float(), b.float()
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-6)


def _reference_grads(q, k, v, do, causal):
    """fp32 torch attention backward over [B,S,H,D] inputs."""
    S, Hq, Hkv = q.shape[1], q.shape[2], k.shape[2]
    qr = q.detach().float().requires_grad_(True)
    kr = k.detach().float().requires_grad_(True)
    vr = v.detach().float().requires_grad_(True)
    g = Hq // Hkv
    qf = qr.permute(0, 2, 1, 3)
    kf = kr.permute(0, 2, 1, 3).repeat_interleave(g, dim=1)
    vf = vr.permute(0, 2, 1, 3).repeat_interleave(g, dim=1)
    s = qf @ kf.transpose(-1, -2) / math.sqrt(D)
    if causal:
        mask = torch.ones(S, S, dtype=torch.bool, device=q.device).triu(1)
        s = s.masked_fill(mask, float("-inf"))
    o_ref = (torch.softmax(s, -1) @ vf).permute(0, 2, 1, 3)
    o_ref.backward(do.float())
    return qr.grad, kr.grad, vr.grad


@pytest.fixture(scope="module")
def runs():
    """Per case: the reference grads and, keyed by (impl, dq mode), the
    (dq, dk, dv) of a merged run, a second merged run and a split run;
    computed once and never modified."""
    assert torch.cuda.is_available()
    ops = _ops()
    hip = ops.hip_ops(required=True)
    dev = torch.device("cuda:0")
    initial_impl = ops.get_attn_bwd_dkv_impl()
    initial_mode = ops.get_attn_bwd_dq_mode()
    scale = 1.0 / math.sqrt(D)
    variants = [("merged", "merged"), ("merged2", "merged"),
                ("split", "split")]
    out = {}
    try:
        for cid, (S, causal, Hq, Hkv) in zip(IDS, CASES):
            gen = torch.Generator(device=dev).manual_seed(1000 + S)
            q = torch.randn(B, S, Hq, D, device=dev, generator=gen).bfloat16()
            k = torch.randn(B, S, Hkv, D, device=dev, generator=gen).bfloat16()
            v = torch.randn(B, S, Hkv, D, device=dev, generator=gen).bfloat16()
            do = torch.randn(B, S, Hq, D, device=dev, generator=gen).bfloat16()
            o, lse = hip.attn_fwd(q, k, v, scale, causal)
            res = {"ref": _reference_grads(q, k, v, do, causal)}
            for mode in DQ_MODES:
                ops.set_attn_bwd_dq_mode(mode)
                for name, impl in variants:
                    ops.set_attn_bwd_dkv_impl(impl)
                    res[name, mode] = hip.attn_bwd(q, k, v, o, do, lse,
                                                   scale, causal)
            out[cid] = res

        # packed path through autograd (rope + strided grads in one buffer)
        S, Hq, Hkv = 256, 8, 4
        gen = torch.Generator(device=dev).manual_seed(77)
        qkv = torch.randn(B, S, (Hq + 2 * Hkv) * D, device=dev,
                          generator=gen).bfloat16()
        do = torch.randn(B, S, Hq, D, device=dev, generator=gen).bfloat16()
        cos, sin = ops.rope_tables(S, D, device=dev)
        from torchx_amd.ops import reference

        xr = qkv.detach().float().requires_grad_(True)
        qf, kf, vf = xr.split([Hq * D, Hkv * D, Hkv * D], dim=-1)
        o_ref = reference.attention(
            reference.rope(qf.reshape(B, S, Hq, D), cos, sin),
            reference.rope(kf.reshape(B, S, Hkv, D), cos, sin),
            vf.reshape(B, S, Hkv, D), causal=True, scale=scale)
        o_ref.backward(do.float())
        res = {"ref": xr.grad}
        for mode in DQ_MODES:
            ops.set_attn_bwd_dq_mode(mode)
            for name, impl in variants:
                ops.set_attn_bwd_dkv_impl(impl)
                x = qkv.detach().clone().requires_grad_(True)
                ops.fused_attention_qkv(x, cos, sin, Hq, Hkv, causal=True,
                                        scale=scale).backward(do)
                res[name, mode] = x.grad
        out["packed"] = (res, Hq, Hkv)
        torch.cuda.synchronize()
    finally:
        ops.set_attn_bwd_dkv_impl(initial_impl)
        ops.set_attn_bwd_dq_mode(initial_mode)
    return out


@pytest.mark.parametrize("mode", DQ_MODES)
@pytest.mark.parametrize("cid", IDS)
def test_merged_bit_identical_to_split(runs, cid, mode):
    r = runs[cid]
    for name, a, b in zip(("dq", "dk", "dv"), r["merged", mode],
                          r["split", mode]):
        assert torch.equal(a, b), f"{name} differs between merged and split"


@pytest.mark.parametrize("mode", DQ_MODES)
@pytest.mark.parametrize("cid", IDS)
def test_merged_matches_reference(runs, cid, mode):
    r = runs[cid]
    for name, got, ref in zip(("dq", "dk", "dv"), r["merged", mode],
                              r["ref"]):
        e = rel_err(got, ref)
        print(f"{cid} merged/{mode} {name} rel_err {e:.4g}")
        assert e < 4e-2, f"{name} err {e}"


@pytest.mark.parametrize("mode", DQ_MODES)
@pytest.mark.parametrize("cid", IDS)
def test_merged_reproducible(runs, cid, mode):
    r = runs[cid]
    for name, a, b in zip(("dq", "dk", "dv"), r["merged", mode],
                          r["merged2", mode]):
        assert torch.equal(a, b), f"{name} differs between two merged runs"


def _split(t, Hq, Hkv):
    return t.split([Hq * D, Hkv * D, Hkv * D], dim=-1)


@pytest.mark.parametrize("mode", DQ_MODES)
def test_packed_qkv(runs, mode):
    res, Hq, Hkv = runs["packed"]
    assert torch.equal(res["merged", mode], res["split", mode]), \
        "packed dqkv differs between merged and split"
    assert torch.equal(res["merged", mode], res["merged2", mode]), \
        "two merged runs differ"
    for name, got, want in zip(("dq", "dk", "dv"),
                               _split(res["merged", mode], Hq, Hkv),
                               _split(res["ref"], Hq, Hkv)):
        e = rel_err(got, want)
        print(f"packed merged/{mode} {name} rel_err {e:.4g}")
        assert e < 4e-2, f"{name} err {e}"


def test_impl_switch():
    ops = _ops()
    initial = ops.get_attn_bwd_dkv_impl()
    try:
        for impl in ("split", "merged"):
            ops.set_attn_bwd_dkv_impl(impl)
            assert ops.get_attn_bwd_dkv_impl() == impl
        with pytest.raises(RuntimeError):
            ops.set_attn_bwd_dkv_impl("fused")
        assert ops.get_attn_bwd_dkv_impl() == "merged"
    finally:
        ops.set_attn_bwd_dkv_impl(initial)
