"""Fused MoE decode router (ops/csrc/moe_route.hip): ``ops.moe_route`` and
``ops.rmsnorm_res_route`` against fp64 on the bf16 operands, the tie rule,
batch invariance, and the Mixtral decode step under the "fused" router."""

import functools

import pytest
import torch

from torchx_amd import ops
from torchx_amd.models.generate_moe import (
    KVCache, decode_step_moe, prefill_moe,
)
from torchx_amd.models.mixtral import (
    MixtralModel, mixtral_gpu_tiny, mixtral_tiny,
)
from torchx_amd.ops import reference

BF = torch.bfloat16
SEED_CPU = SEED_GPU = 0  # see the two decode-step tests
# (H, E, k, B): ITERS 1; production; ITERS 3, 4 groups; ceiling; k 1; k = E
SHAPES = [(2048, 4, 2, 8), (4096, 8, 2, 8), (6144, 16, 4, 8),
          (8192, 16, 8, 8), (2048, 8, 1, 8), (4096, 8, 8, 8),
          (4096, 8, 2, 1), (4096, 8, 2, 33)]


def _inputs(H, E, B, family, seed=0):
    """(x, res, w, wr) on the CPU, x + res the row the norm sees. "planted":
    router row e is +-0.05 on the columns with col % E == e, and x carries
    a[b, e] = a permutation of 0.5 * {0..E-1} along row e's signs, so the
    logits of a row are well separated. "tie": planted with E = 8, router
    row 5 a copy of row 2 and their logit the largest. "randn": plain."""
    g = torch.Generator().manual_seed(seed)
    w = (0.75 + 0.5 * torch.rand(H, generator=g)).to(BF)
    if family == "randn":
        wr = 0.02 * torch.randn(E, H, generator=g)
        x = torch.randn(B, H, generator=g)
    else:
        col = torch.arange(H)
        sign = torch.randint(0, 2, (E, H), generator=g) * 2.0 - 1.0
        sign = sign * (col[None, :] % E == torch.arange(E)[:, None])
        a = 0.5 * torch.stack([torch.randperm(E, generator=g)
                               for _ in range(B)]).float()
        if family == "tie":
            sign[5] = sign[2]
            a[:, 2] = 0.5 * E
        wr = 0.05 * sign
        x = 0.5 * torch.randn(B, H, generator=g) + a @ sign
    res = (0.3 * x).to(BF)
    return (x - res.float()).to(BF), res, w, wr.to(BF)


def _check_route(y, wr, k, idx, cw, exact):
    """Selection and weight checks on one result (prints err / bound)."""
    y64, w64 = y.double().cpu(), wr.double().cpu()
    idx, cw = idx.cpu(), cw.double().cpu()
    H, E = y.shape[1], wr.shape[0]
    l64 = y64 @ w64.t()
    lb = (2 * (H + 2) * 2.0 ** -24 * (y64.abs() @ w64.abs().t())).amax(
        -1, keepdim=True)                       # max_e lb_e per row
    top, order = torch.sort(l64, dim=-1, descending=True, stable=True)
    if exact:  # precondition: fp64 alone decides the selection
        m = min(k + 1, E)
        assert (top[:, :m - 1] - top[:, 1:m] > 2 * lb).all()
    assert idx.dtype == torch.int64 and idx.shape == (y.shape[0], k)
    assert ((idx >= 0) & (idx < E)).all()
    assert all(len(set(r)) == k for r in idx.tolist())
    sel = l64.gather(1, idx)
    if exact:
        assert torch.equal(idx, order[:, :k])
    else:
        assert (sel >= top[:, k - 1:k] - 2 * lb).all()
        assert (sel[:, :-1] >= sel[:, 1:] - 2 * lb).all()
    cw64 = torch.softmax(sel, -1)
    bound = 2.0 ** -8 * cw64 + cw64 * (2 * lb + 2.0 ** -20)
    ratio = ((cw - cw64).abs() / bound).max().item()
    print(f"H={H} E={E} k={k} B={y.shape[0]} max err/bound {ratio:.3f}")
    assert ratio <= 1.0, ratio


@functools.lru_cache(maxsize=None)
def _gpu_run(shape, family):
    """Inputs and every GPU result of one shape, computed once."""
    H, E, k, B = shape
    x, res, w, wr = (t.cuda() for t in _inputs(H, E, B, family))
    out = {"in": (x, res, w, wr)}
    for tag, r in (("res", res), ("nores", None)):
        out["norm_" + tag] = ops.rmsnorm_res(x, r, w, 1e-5)
        out["fused_" + tag] = ops.rmsnorm_res_route(x, r, w, 1e-5, wr, k)
    out["route"] = ops.moe_route(out["fused_res"][1], wr, k)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_norm_bits(shape):
    run = _gpu_run(shape, "planted")
    for tag in ("res", "nores"):
        s, y = run["norm_" + tag]
        fs, fy = run["fused_" + tag][:2]
        assert torch.equal(fs, s) and torch.equal(fy, y), tag
    assert run["fused_nores"][0] is run["in"][0]  # no res: s is x itself


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["planted", "randn"])
@pytest.mark.parametrize("shape", SHAPES)
def test_selection_and_weights(shape, family):
    """Exact fp64 top-k (planted) or the 2 max lb slack (randn), and the
    derived bound on the softmax weights."""
    run = _gpu_run(shape, family)
    wr, k = run["in"][3], shape[2]
    for tag in ("res", "nores"):
        _, y, idx, cw = run["fused_" + tag]
        _check_route(y, wr, k, idx, cw, exact=family == "planted")
    idx, cw = run["route"]
    assert torch.equal(idx, run["fused_res"][2])
    assert torch.equal(cw, run["fused_res"][3])


@pytest.mark.gpu
def test_tie_rule_and_batch_invariance():
    x, res, w, wr = (t.cuda() for t in _inputs(4096, 8, 8, "tie"))
    _, y, idx, cw = ops.rmsnorm_res_route(x, res, w, 1e-5, wr, 2)
    assert idx.tolist() == [[2, 5]] * 8
    assert ops.moe_route(y, wr, 1)[0].tolist() == [[2]] * 8
    for b in range(8):
        one = ops.rmsnorm_res_route(x[b:b + 1], res[b:b + 1], w, 1e-5, wr, 2)
        assert torch.equal(one[2], idx[b:b + 1])
        assert torch.equal(one[3], cw[b:b + 1])


@pytest.mark.parametrize("shape", SHAPES)
def test_reference_cpu(shape):
    """``reference.moe_route`` (what ``ops`` runs on the CPU) meets the
    selection and weight checks on the planted family, and the tie rule."""
    H, E, k, B = shape
    x, res, w, wr = _inputs(H, E, B, "planted")
    s, y, idx, cw = ops.rmsnorm_res_route(x, res, w, 1e-5, wr, k)
    assert torch.equal(s, x + res)
    assert torch.equal(y, reference.rmsnorm(s, w, 1e-5))
    _check_route(y, wr, k, idx, cw, exact=True)
    got = ops.moe_route(y, wr, k)
    assert torch.equal(got[0], idx) and torch.equal(got[1], cw)
    assert torch.equal(ops.moe_route(y[:1], wr, k)[0], idx[:1])
    if shape == SHAPES[1]:
        x, res, w, wr = _inputs(H, E, B, "tie")
        y = reference.rmsnorm(x + res, w, 1e-5)
        assert reference.moe_route(y, wr, 2)[0].tolist() == [[2, 5]] * B
        assert reference.moe_route(y, wr, 1)[0].tolist() == [[2]] * B


def test_fused_router_decode_matches_full_forward_cpu():
    """``test_cached_moe_decode_matches_full_forward`` under the "fused"
    router. Seed SEED_CPU: the first from 0 upward for which, in every layer
    and row of the three compared steps, the fp64 gap between the k-th and
    the (k+1)-th logit exceeds the bf16 rounding of the logits
    (2^-8 max|l|), so fp32 and bf16-rounded logits pick the same experts."""
    assert ops.get_moe_router_impl() == "torch"  # the default
    with pytest.raises(ValueError):
        ops.set_moe_router_impl("triton")
    torch.manual_seed(SEED_CPU)
    cfg = mixtral_tiny()
    model = MixtralModel(cfg)
    B, S0 = 2, 12
    cur = torch.randint(0, cfg.vocab_size, (B, S0))
    caches = [KVCache.empty(cfg, B, S0 + 6, torch.device("cpu"))
              for _ in range(cfg.num_layers)]
    nxt = prefill_moe(model, cur, caches).argmax(-1, keepdim=True)
    ops.set_moe_router_impl("fused")
    try:
        for _ in range(3):
            dec = decode_step_moe(model, nxt, caches)
            cur = torch.cat([cur, nxt], dim=1)
            with torch.no_grad():
                full = model(cur)[:, -1]
            assert torch.allclose(dec.float(), full.float(), atol=4e-2), (
                (dec - full).abs().max())
            nxt = dec.argmax(-1, keepdim=True)
    finally:
        ops.set_moe_router_impl("torch")


@pytest.mark.gpu
def test_fused_router_decode_step_gpu(monkeypatch):
    """One ``decode_step`` of mixtral_gpu_tiny after a prefill: under "fused"
    a layer's MLP half is one ``rmsnorm_res_route`` and one
    ``moe_decode_mlp`` and ``torch.topk`` is never called; its logits agree
    with the "torch" step, which still goes through ``_moe_mlp_decode``.
    Seed SEED_GPU: chosen on the CPU by the condition of the CPU test, with
    a factor 4 of margin for the kernels' activations."""
    from test_generate import _record_calls
    from torchx_amd.models import generate_moe

    dev = torch.device("cuda:0")
    torch.manual_seed(SEED_GPU)
    cfg = mixtral_gpu_tiny()
    model = MixtralModel(cfg).to(dev)
    tokens = torch.randint(0, cfg.vocab_size, (2, 32)).to(dev)
    calls = _record_calls(monkeypatch, [
        (ops, "rmsnorm_res_route"), (ops, "moe_decode_mlp"), (torch, "topk"),
        (generate_moe, "_moe_mlp_decode")])
    logits = {}
    try:
        for impl in ("torch", "fused"):
            ops.set_moe_router_impl(impl)
            caches = [KVCache.empty(cfg, 2, 48, dev)
                      for _ in range(cfg.num_layers)]
            prefill_moe(model, tokens, caches)
            del calls[:]
            logits[impl] = decode_step_moe(model, tokens[:, -1:], caches)
            want = (["_moe_mlp_decode"] if impl == "torch"
                    else ["rmsnorm_res_route", "moe_decode_mlp"])
            assert calls == cfg.num_layers * want, (impl, calls)
    finally:
        ops.set_moe_router_impl("torch")
    ref = logits["torch"].float()
    err = (logits["fused"].float() - ref).abs().max().item()
    assert err < 5e-2 * (ref.abs().max().item() + 1e-6), err
