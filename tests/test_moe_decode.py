"""ops.moe_decode_mlp: the device-routed grouped expert GEMV kernels
against the per-expert loop (bit for bit) and against fp64."""

import functools

import pytest
import torch

from torchx_amd import ops
from torchx_amd.ops.bounds import E32, U, bound_ratio

# (B, H, I, E, k, routing): each runs one code path at its smallest size
CASES = {
    # tail-only K loop, single token
    "B1-tail": (1, 512, 512, 4, 2, "topk"),
    # H: one 4-chunk main iteration + one tail chunk; I: three tail chunks
    "B3-main+tail": (3, 2560, 1536, 8, 2, "topk"),
    # every row picks (5, 2): M = 8 bodies, six idle experts, slot order
    # against ascending expert order
    "B8-same": (8, 2560, 512, 8, 2, "same"),
    # row b picks expert 2b+1: M = 1 everywhere, E at its limit, k = 1
    "B8-spread": (8, 512, 512, 16, 1, "spread"),
    # k > 2: the ordered bf16 fold matters
    "B5-k3": (5, 1024, 1024, 4, 3, "topk"),
}


@functools.lru_cache(maxsize=None)
def _case(cid):
    """CPU inputs of a case with the fp64 result and its elementwise bound
    (computed once, shared by the tests, never modified)."""
    B, H, I, E, k, routing = CASES[cid]
    g = torch.Generator().manual_seed(sorted(CASES).index(cid))
    bf = torch.bfloat16
    x = torch.randn(B, H, generator=g).to(bf)
    wgu = [(0.02 * torch.randn(2 * I, H, generator=g)).to(bf)
           for _ in range(E)]
    wdown = [(0.02 * torch.randn(H, I, generator=g)).to(bf)
             for _ in range(E)]
    logits = torch.randn(B, E, generator=g)
    if routing == "topk":
        w, idx = torch.topk(logits, k, dim=-1)
    else:
        idx = (torch.tensor([[5, 2]]).expand(B, 2) if routing == "same"
               else 2 * torch.arange(B)[:, None] + 1).contiguous()
        w = logits.gather(1, idx)
    cw = torch.softmax(w, dim=-1).to(bf)

    out64 = torch.zeros(B, H, dtype=torch.float64)
    bound = torch.zeros(B, H, dtype=torch.float64)
    xd = x.double()
    for e in sorted(set(idx.flatten().tolist())):
        gu_w, wd = wgu[e].double(), wdown[e].double()
        for b, j in (idx == e).nonzero().tolist():
            g64, u64 = (gu_w @ xd[b]).chunk(2)
            gabs, uabs = (gu_w.abs() @ xd[b].abs()).chunk(2)
            silu = g64 * torch.sigmoid(g64)
            h64 = silu * u64
            dh = U * h64.abs() + E32 * (1.1 * u64.abs() * gabs
                                        + silu.abs() * uabs)
            c = cw[b, j].double()
            out64[b] += c * (wd @ h64)
            bound[b] += c.abs() * (wd.abs() @ (dh + (2 * U + E32) * h64.abs()))
    bound += U * out64.abs()
    return dict(x=x, idx=idx, cw=cw, wgu=wgu, wdown=wdown, out64=out64,
                bound=bound)


def _run(cid, device, impl):
    c = _case(cid)
    args = [c[n].to(device) for n in ("x", "idx", "cw")] + [
        [w.to(device) for w in c[n]] for n in ("wgu", "wdown")]
    before = ops.get_moe_decode_impl()
    ops.set_moe_decode_impl(impl)
    try:
        return ops.moe_decode_mlp(*args).cpu()
    finally:
        ops.set_moe_decode_impl(before)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(CASES))
def test_fused_is_bit_identical_to_loop(cid):
    assert torch.equal(_run(cid, "cuda:0", "fused"),
                       _run(cid, "cuda:0", "loop"))


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(CASES))
def test_fused_within_fp64_bound(cid):
    c = _case(cid)
    ratio, ok = bound_ratio(_run(cid, "cuda:0", "fused"), c["out64"],
                            c["bound"])
    print(f"{cid}: max err/bound = {ratio:.3f}")
    assert ok, ratio


@pytest.mark.gpu
def test_moe_mlp_decode_never_waits_for_the_device():
    from torchx_amd.models.generate_moe import _moe_mlp_decode
    from torchx_amd.models.mixtral import MoELayer, mixtral_gpu_tiny

    torch.manual_seed(0)
    cfg = mixtral_gpu_tiny()
    moe = MoELayer(cfg).to("cuda:0")
    x = torch.randn(4, cfg.hidden_size, device="cuda:0", dtype=torch.bfloat16)
    before = ops.get_moe_decode_impl()
    ops.set_moe_decode_impl("fused")
    _moe_mlp_decode(moe, x)  # library set-up of the router matmul
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = _moe_mlp_decode(moe, x)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
        ops.set_moe_decode_impl(before)
    assert out.shape == x.shape and bool(out.float().abs().sum() > 0)


@pytest.mark.parametrize("cid", ["B1-tail", "B5-k3"])
def test_cpu_matches_fp64(cid):
    out = _run(cid, "cpu", "fused")
    out64 = _case(cid)["out64"]
    atol = 4 * U * out64.abs().max().item()
    assert (out.double() - out64).abs().max().item() <= atol
