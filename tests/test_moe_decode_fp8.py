"""ops.moe_decode_mlp on ops.Fp8Weight experts (ops/csrc/moe_gemv_fp8.hip):
the W8A16 grouped expert kernels against fp64 per element, against the
per-expert loop bit for bit, and in a quantised Mixtral.

The bound is the one of test_moe_decode.py with g(K) = 2 (K + 2) 2^-24 in
place of e32 on the dot-product terms (test_gemv_fp8.py: K fp32 roundings
in any order plus the scale multiply, doubled for v_dot2c): with g64, u64
= scale * (w8 @ x), gabs, uabs the same on absolute values and h64 =
silu(g64) u64,
  dh = (u + e32) |h64| + g(H) (1.1 |u64| gabs + |silu(g64)| uabs),
every (token, slot) adds |c| scale_d (|wd8| @ (dh + (2u + g(I)) |h64|)),
and u |out64| is added once. Derived, not measured."""

import functools

import pytest
import torch

from torchx_amd import ops
from torchx_amd.ops.bounds import E32, U, bound_ratio

# (B, H, I, E, k, routing): each runs one code path at its smallest size
CASES = {
    # tail-only K loop, M = 1
    "B1-tail": (1, 1024, 1024, 4, 2, "topk"),
    # H: one 2-chunk iteration plus the tail; I: main loop only
    "B3-main+tail": (3, 3072, 2048, 4, 2, "topk"),
    # every row picks (5, 2): M = 8 bodies, six idle experts, slot order
    # against ascending expert order
    "B8-same": (8, 1024, 1024, 8, 2, "same"),
    # row b picks expert 2b+1: M = 1 everywhere, E at its limit, k = 1
    "B8-spread": (8, 1024, 1024, 16, 1, "spread"),
    # k > 2: the ordered bf16 fold matters
    "B5-k3": (5, 2048, 1024, 4, 3, "topk"),
}


@functools.lru_cache(maxsize=None)
def _case(cid):
    """CPU inputs of a case with the fp64 result and its elementwise bound
    (computed once, shared by the tests, never modified)."""
    B, H, I, E, k, routing = CASES[cid]
    g = torch.Generator().manual_seed(sorted(CASES).index(cid))
    x = torch.randn(B, H, generator=g).bfloat16()

    def quantised(n, kk):  # row r times 2^((r % 5) - 2): the scales differ
        w = 0.02 * torch.randn(n, kk, generator=g)
        return ops.quantize_fp8_rows(
            w * (2.0 ** ((torch.arange(n) % 5) - 2))[:, None])

    wgu = [quantised(2 * I, H) for _ in range(E)]
    wdown = [quantised(H, I) for _ in range(E)]
    logits = torch.randn(B, E, generator=g)
    if routing == "topk":
        w, idx = torch.topk(logits, k, dim=-1)
    else:
        idx = (torch.tensor([[5, 2]]).expand(B, 2) if routing == "same"
               else 2 * torch.arange(B)[:, None] + 1).contiguous()
        w = logits.gather(1, idx)
    cw = torch.softmax(w, dim=-1).bfloat16()

    gh, gi = 2 * (H + 2) * 2.0 ** -24, 2 * (I + 2) * 2.0 ** -24
    out64 = torch.zeros(B, H, dtype=torch.float64)
    bound = torch.zeros(B, H, dtype=torch.float64)
    xd = x.double()
    for e in sorted(set(idx.flatten().tolist())):
        sgu, sd = wgu[e].scale.double(), wdown[e].scale.double()
        gu_w, wd = wgu[e].w8.double(), wdown[e].w8.double()
        for b, j in (idx == e).nonzero().tolist():
            g64, u64 = (sgu * (gu_w @ xd[b])).chunk(2)
            gabs, uabs = (sgu * (gu_w.abs() @ xd[b].abs())).chunk(2)
            silu = g64 * torch.sigmoid(g64)
            h64 = silu * u64
            dh = (U + E32) * h64.abs() + gh * (1.1 * u64.abs() * gabs
                                               + silu.abs() * uabs)
            c = cw[b, j].double()
            out64[b] += c * sd * (wd @ h64)
            bound[b] += c.abs() * sd * (
                wd.abs() @ (dh + (2 * U + gi) * h64.abs()))
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
def test_fused_fp8_within_fp64_bound(cid):
    c = _case(cid)
    ratio, ok = bound_ratio(_run(cid, "cuda:0", "fused"), c["out64"],
                            c["bound"])
    print(f"{cid}: max err/bound = {ratio:.3f}")
    assert ok, ratio


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(CASES))
def test_fused_fp8_is_bit_identical_to_dot2_loop(cid, monkeypatch):
    """With the dot2 GEMVs for every group size; without the patch the loop
    sends the groups of 8 of B8-same to the MFMA kernels."""
    fused = _run(cid, "cuda:0", "fused")
    monkeypatch.setattr(ops, "FP8W_DOT2_MAX_M", 8)
    assert torch.equal(fused, _run(cid, "cuda:0", "loop"))


def _quantised_linears(model):
    """(quantised, left alone) linears of a Mixtral model."""
    lins = [lin for blk in model.blocks for lin in (
        blk.wqkv, blk.wo, *(w for ex in blk.moe.local_experts
                            for w in (ex.wgu, ex.wdown)))]
    return lins, [blk.moe.router for blk in model.blocks] + [model.lm_head]


@pytest.mark.gpu
def test_quantised_mixtral_decode():
    """num_experts = top_k = 2: every token uses both experts, so no
    rounding can change the expert set. The MLP half is the two fp8
    dispatches with no host sync, and one decode step after a short prefill
    meets the criterion of test_gemv_fp8.py: max|fp8 - ref| <= 2 max|bf16 -
    ref|, ref the fp32 CPU step on the dequantised weights, bf16 the GPU
    step on the snapped weights."""
    from torchx_amd.models.generate import (
        KVCache, decode_step, prefill, quantize_decode_weights,
    )
    from torchx_amd.models.generate_moe import _moe_mlp_decode
    from torchx_amd.models.mixtral import MixtralConfig, MixtralModel

    dev = torch.device("cuda:0")
    torch.manual_seed(12)
    cfg = MixtralConfig(vocab_size=512, hidden_size=2048,
                        intermediate_size=2048, num_layers=2, num_heads=8,
                        num_kv_heads=2, head_dim=128, max_seq_len=64,
                        num_experts=2, top_k=2)
    B, S, T = 3, 16, 32
    model = quantize_decode_weights(MixtralModel(cfg, device=dev))
    lins, kept = _quantised_linears(model)
    assert all(isinstance(lin.decode_weight, ops.Fp8Weight) for lin in lins)
    assert not any(hasattr(lin, "decode_weight") for lin in kept)

    moe = model.blocks[0].moe
    x = torch.randn(B, cfg.hidden_size, device=dev, dtype=torch.bfloat16)
    w, idx = torch.topk((x @ moe.router.weight.t()).float(), cfg.top_k, dim=-1)
    w = torch.softmax(w, dim=-1).to(x.dtype)
    want = ops.moe_decode_mlp(
        x, idx, w, [ex.wgu.decode_weight for ex in moe.local_experts],
        [ex.wdown.decode_weight for ex in moe.local_experts])
    assert torch.equal(_moe_mlp_decode(moe, x), want)  # and the warm-up call
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = _moe_mlp_decode(moe, x)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.equal(got, want)

    ref_model = MixtralModel(cfg)
    ref_model.load_state_dict(model.state_dict())
    ref_model.float()
    for lin, ref_lin in zip(lins, _quantised_linears(ref_model)[0]):
        ref_lin.weight.data = lin.decode_weight.dequant().cpu()
    tokens = torch.randint(0, cfg.vocab_size, (B, S), device=dev)
    caches = [KVCache.empty(cfg, B, T, dev) for _ in range(cfg.num_layers)]
    nxt = prefill(model, tokens, caches).argmax(-1, keepdim=True)

    def step(m, device, dtype):
        cs = [KVCache(c.k.to(device, dtype), c.v.to(device, dtype), S)
              for c in caches]
        return decode_step(m, nxt.to(device), cs).double().cpu()

    fp8 = step(model, dev, torch.bfloat16)
    for lin in lins:
        del lin.decode_weight
    bf16 = step(model, dev, torch.bfloat16)
    ref = step(ref_model, "cpu", torch.float32)
    d8, d16 = (fp8 - ref).abs().max().item(), (bf16 - ref).abs().max().item()
    print(f"decode step max|logits - ref|: fp8 {d8:.4g}, bf16 {d16:.4g}")
    assert d8 <= 2 * d16, (d8, d16)


@pytest.mark.parametrize("cid", ["B1-tail", "B5-k3"])
def test_cpu_fp8_matches_fp64(cid):
    out = _run(cid, "cpu", "fused")
    out64 = _case(cid)["out64"]
    atol = 4 * U * out64.abs().max().item()
    assert (out.double() - out64).abs().max().item() <= atol


def test_quantize_decode_weights_mixtral_cpu():
    from torchx_amd.models.generate import quantize_decode_weights
    from torchx_amd.models.mixtral import MixtralModel, mixtral_tiny

    torch.manual_seed(0)
    model = quantize_decode_weights(MixtralModel(mixtral_tiny()))
    lins, kept = _quantised_linears(model)
    assert all(isinstance(lin.decode_weight, ops.Fp8Weight)
               and lin.decode_weight.shape == tuple(lin.weight.shape)
               for lin in lins)
    assert not any(hasattr(lin, "decode_weight") for lin in kept)
