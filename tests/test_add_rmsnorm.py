"""ops.add_rmsnorm (the residual add fused into the RMSNorm that consumes
it) and the LlamaModel restructured around it: everything is compared for
exact equality with the unfused composition — a tensor add followed by
ops.rmsnorm, and the block formula written out below."""

import pytest
import torch

from torchx_amd import ops
from torchx_amd.models.llama import (LlamaModel, _lin, llama_gpu_tiny,
                                     llama_tiny)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _inputs(rows, H, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).to(
            torch.bfloat16).to(dev)

    x = rnd(rows, H, scale=2.0)
    delta = rnd(rows, H)
    w = (1.0 + 0.25 * torch.randn(H, generator=g)).to(torch.bfloat16).to(dev)
    ds = rnd(rows, H)
    dy = rnd(rows, H)
    return x, delta, w, ds, dy


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [1, 5, 67])
@pytest.mark.parametrize("H", [2048, 4096, 6144, 8192])
def test_add_rmsnorm_matches_add_then_rmsnorm(dev, H, rows):
    eps = 1e-5
    x, delta, w, ds, dy = _inputs(rows, H, dev, seed=H + rows)
    hip = ops.hip_ops()

    # forward, invrms included
    s, y, invrms = hip.add_rmsnorm_fwd(x, delta, w, eps)
    s_ref = x + delta
    y_ref, invrms_ref = hip.rmsnorm_fwd(s_ref, w, eps)
    assert torch.equal(s, s_ref)
    assert torch.equal(y, y_ref)
    assert torch.equal(invrms, invrms_ref)

    # backward with cotangents on both outputs
    xf, df, wf = (t.clone().requires_grad_(True) for t in (x, delta, w))
    sf, yf = ops.add_rmsnorm(xf, df, wf, eps)
    assert torch.equal(sf, s_ref) and torch.equal(yf, y_ref)
    torch.autograd.backward([sf, yf], [ds, dy])

    xu, du, wu = (t.clone().requires_grad_(True) for t in (x, delta, w))
    su = xu + du
    yu = ops.rmsnorm(su, wu, eps)
    torch.autograd.backward([su, yu], [ds, dy])

    assert torch.equal(xf.grad, xu.grad)
    assert torch.equal(df.grad, du.grad)
    assert torch.equal(wf.grad, wu.grad)


@pytest.mark.gpu
def test_add_rmsnorm_no_cotangent_on_s(dev):
    """The final-norm use: s is dropped, backward sees ds = None and runs
    the plain dx kernel."""
    eps = 1e-5
    x, delta, w, _, dy = _inputs(67, 4096, dev, seed=7)
    xf, df, wf = (t.clone().requires_grad_(True) for t in (x, delta, w))
    yf = ops.add_rmsnorm(xf, df, wf, eps)[1]
    yf.backward(dy)

    xu, du, wu = (t.clone().requires_grad_(True) for t in (x, delta, w))
    yu = ops.rmsnorm(xu + du, wu, eps)
    yu.backward(dy)

    assert torch.equal(yf, yu)
    assert torch.equal(xf.grad, xu.grad)
    assert torch.equal(df.grad, du.grad)
    assert torch.equal(wf.grad, wu.grad)


@pytest.mark.gpu
def test_rmsnorm_res_decode_entry_unchanged(dev):
    """ops.rmsnorm_res (decode) shares the kernel: same (s, y) as before,
    with and without a residual."""
    x, delta, w, _, _ = _inputs(5, 2048, dev, seed=3)
    s, y = ops.rmsnorm_res(x, delta, w, 1e-5)
    assert torch.equal(s, x + delta)
    assert torch.equal(y, ops.rmsnorm(x + delta, w, 1e-5))
    s0, y0 = ops.rmsnorm_res(x, None, w, 1e-5)
    assert s0.data_ptr() == x.data_ptr()
    assert torch.equal(y0, ops.rmsnorm(x, w, 1e-5))


def _unfused_loss(model, tokens, targets):
    """The model with every residual add as its own tensor add and every
    norm a plain ops.rmsnorm, on the same modules' weights."""
    cfg = model.cfg
    x = model.embed(tokens)
    cos, sin = model.rope_cos, model.rope_sin
    for blk in model.blocks:
        B, S, _ = x.shape
        xn = ops.rmsnorm(x, blk.attn_norm, cfg.rms_eps)
        qkv = _lin(blk.wqkv, xn)
        attn = ops.fused_attention_qkv(
            qkv, cos, sin, cfg.num_heads, cfg.num_kv_heads, causal=True)
        x = x + _lin(blk.wo, attn.reshape(B, S, cfg.q_dim))
        xn = ops.rmsnorm(x, blk.mlp_norm, cfg.rms_eps)
        x = x + _lin(blk.wdown, ops.swiglu_packed(_lin(blk.wgu, xn)))
    x = ops.rmsnorm(x, model.final_norm, cfg.rms_eps)
    return ops.fused_linear_cross_entropy(x, model.lm_head.weight, targets)


def _check_model_equals_unfused(cfg, device, B, S):
    torch.manual_seed(0)
    model = LlamaModel(cfg, device=device)
    # norm weights off 1.0 so their grads and the scale path matter
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("norm"):
                p.add_(0.1 * torch.randn_like(p))
    tokens = torch.randint(0, cfg.vocab_size, (B, S), device=device)
    targets = torch.roll(tokens, -1, 1)

    loss = model(tokens, targets)
    loss.backward()
    grads = {n: p.grad.clone() for n, p in model.named_parameters()}
    model.zero_grad(set_to_none=True)

    loss_ref = _unfused_loss(model, tokens, targets)
    loss_ref.backward()

    assert torch.equal(loss, loss_ref)
    for n, p in model.named_parameters():
        assert p.grad is not None and n in grads, n
        assert torch.equal(grads[n], p.grad), n


def test_llama_tiny_equals_unfused_cpu():
    _check_model_equals_unfused(llama_tiny(), None, B=2, S=48)


@pytest.mark.gpu
def test_llama_gpu_tiny_equals_unfused(dev):
    _check_model_equals_unfused(llama_gpu_tiny(), dev, B=2, S=200)
