"""Attention backward with the dS export: the dkv kernel writes the scaled
bf16 dS sub-tiles to a scratch buffer and the streamed dQ kernel sums
dS . K over them ("stream"), against the recompute dQ kernel and the fp32
torch reference.

Shapes are the smallest that reach each hazard (D = 128, B = 2):
  S=256 causal Hq8/Hkv2   two 128-row kv blocks -> dQ summed over two
                          exporting workgroups, TFKV=128 dkv instance
  S=384 causal Hq4/Hkv4   three blocks, group size 1
  S=192 causal            S % 128 != 0 -> TFKV=64 instance, partial kv block
  S=160 causal            last staged 64-row tile holds a q sub-tile that
                          starts past the last row (q 160..191)
  S=128 non-causal        full square, nothing skipped
  packed S=256 Hq8/Hkv4   fused_attention_qkv: strided dq/dk/dv in one buffer

Measured on MI355X: dq is bit-identical between the two modes at every
shape here (norm-relative difference 0.0 against the 2^-8 bound).
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


def _ops():
    from torchx_amd import ops

    assert ops.extension_available(), "HIP extension must be built in-tree"
    return ops


def rel_err(a, b):
    a, b = a.float(), b.float()
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-6)


def norm_rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / b.norm()).item()


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
    """Per case: reference grads and the (dq, dk, dv) of stream run 1,
    stream run 2 and the recompute run, computed once and never modified."""
    assert torch.cuda.is_available()
    ops = _ops()
    hip = ops.hip_ops(required=True)
    dev = torch.device("cuda:0")
    initial = ops.get_attn_bwd_dq_mode()
    scale = 1.0 / math.sqrt(D)
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
            for name, mode in [("stream", "stream"), ("stream2", "stream"),
                               ("recompute", "recompute")]:
                ops.set_attn_bwd_dq_mode(mode)
                res[name] = hip.attn_bwd(q, k, v, o, do, lse, scale, causal)
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
        for name, mode in [("stream", "stream"), ("stream2", "stream"),
                           ("recompute", "recompute")]:
            ops.set_attn_bwd_dq_mode(mode)
            x = qkv.detach().clone().requires_grad_(True)
            ops.fused_attention_qkv(x, cos, sin, Hq, Hkv, causal=True,
                                    scale=scale).backward(do)
            res[name] = x.grad
        out["packed"] = (res, Hq, Hkv)
        torch.cuda.synchronize()
    finally:
        ops.set_attn_bwd_dq_mode(initial)
    return out


@pytest.mark.parametrize("cid", IDS)
def test_stream_matches_reference(runs, cid):
    r = runs[cid]
    for name, got, ref in zip(("dq", "dk", "dv"), r["stream"], r["ref"]):
        e = rel_err(got, ref)
        print(f"{cid} stream {name} rel_err {e:.4g}")
        assert e < 4e-2, f"{name} err {e}"


@pytest.mark.parametrize("cid", IDS)
def test_recompute_matches_reference(runs, cid):
    r = runs[cid]
    for name, got, ref in zip(("dq", "dk", "dv"), r["recompute"], r["ref"]):
        e = rel_err(got, ref)
        print(f"{cid} recompute {name} rel_err {e:.4g}")
        assert e < 4e-2, f"{name} err {e}"


@pytest.mark.parametrize("cid", IDS)
def test_export_leaves_dk_dv_bit_identical(runs, cid):
    r = runs[cid]
    assert torch.equal(r["stream"][1], r["recompute"][1]), "dk differs"
    assert torch.equal(r["stream"][2], r["recompute"][2]), "dv differs"


@pytest.mark.parametrize("cid", IDS)
def test_dq_stream_vs_recompute(runs, cid):
    """Both paths feed bf16-rounded dS into an fp32 sum in the same k
    order: more than one bf16 ulp apart means a wrong or missing tile."""
    r = runs[cid]
    e = norm_rel(r["stream"][0], r["recompute"][0])
    print(f"{cid} dq stream-vs-recompute norm-relative {e:.4g}")
    assert e < 2.0 ** -8


@pytest.mark.parametrize("cid", IDS)
def test_stream_reproducible(runs, cid):
    r = runs[cid]
    for name, a, b in zip(("dq", "dk", "dv"), r["stream"], r["stream2"]):
        assert torch.equal(a, b), f"{name} differs between two stream runs"


def _split(t, Hq, Hkv):
    return t.split([Hq * D, Hkv * D, Hkv * D], dim=-1)


def test_packed_qkv(runs):
    res, Hq, Hkv = runs["packed"]
    ref = _split(res["ref"], Hq, Hkv)
    st = _split(res["stream"], Hq, Hkv)
    rc = _split(res["recompute"], Hq, Hkv)
    for name, got, want in zip(("dq", "dk", "dv"), st, ref):
        e = rel_err(got, want)
        print(f"packed stream {name} rel_err {e:.4g}")
        assert e < 4e-2, f"{name} err {e}"
    assert torch.equal(st[1], rc[1]), "dk differs between modes"
    assert torch.equal(st[2], rc[2]), "dv differs between modes"
    e = norm_rel(st[0], rc[0])
    print(f"packed dq stream-vs-recompute norm-relative {e:.4g}")
    assert e < 2.0 ** -8
    assert torch.equal(res["stream"], res["stream2"]), \
        "two stream runs differ"


def test_mode_switch_rejects_unknown():
    ops = _ops()
    with pytest.raises(RuntimeError):
        ops.set_attn_bwd_dq_mode("atomic")
