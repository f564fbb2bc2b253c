"""Wgrad from transposed operands: the SwiGLU backward kernel that also
writes dgu^T, the operand forms of fast_linear's wgrad, and the lm_head
wgrad inside fused_linear_cross_entropy.

There is no h / h^T pair to check: wdown's wgrad did not gain from a
transposed x (profiles/README.md, r9a), so no SwiGLU forward that writes
h^T exists.

Bound on every dW: the GEMM accumulates in fp32 and the sum is rounded once
to bf16; bf16 spacing is 2^-7 relative, so the half-spacing is 2^-8 — taken
as a bound on the norm-relative error against an fp64 reference (the bound
tests/test_attention_bwd_stream.py uses)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

BOUND = 2.0 ** -8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _ops():
    from torchx_amd import ops

    assert ops.extension_available(), "HIP extension must be built in-tree"
    return ops


def _nrel(a, ref):
    a, ref = a.double(), ref.double()
    return ((a - ref).norm() / ref.norm()).item()


# ---------------------------------------------------------------------------
# fused SwiGLU backward (+ transposed copy)
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("rows", [64, 192])
@pytest.mark.parametrize("inter", [64, 4096])
def test_swiglu_gu_bwd_t(dev, rows, inter):
    hip = _ops().hip_ops()
    torch.manual_seed(rows + inter)
    gu = torch.randn(rows, 2 * inter, device=dev, dtype=torch.bfloat16)
    dout = torch.randn(rows, inter, device=dev, dtype=torch.bfloat16)
    dgu, dgut = hip.swiglu_gu_bwd_t(dout, gu)
    assert dgut.shape == (2 * inter, rows) and dgut.is_contiguous()
    assert torch.equal(dgu, hip.swiglu_gu_bwd(dout, gu))
    assert torch.equal(dgut, dgu.t().contiguous())


def test_swiglu_gu_bwd_t_block_groups(dev):
    """The kernel walks the row tiles in groups of 32: 33 row tiles make a
    full group and a last group of one, over two column tiles."""
    hip = _ops().hip_ops()
    torch.manual_seed(7)
    rows, inter = 33 * 64, 128
    gu = torch.randn(rows, 2 * inter, device=dev, dtype=torch.bfloat16)
    dout = torch.randn(rows, inter, device=dev, dtype=torch.bfloat16)
    dgu, dgut = hip.swiglu_gu_bwd_t(dout, gu)
    assert torch.equal(dgu, hip.swiglu_gu_bwd(dout, gu))
    assert torch.equal(dgut, dgu.t().contiguous())


def test_swiglu_gu_bwd_t_rejects_unaligned(dev):
    hip = _ops().hip_ops()
    gu = torch.randn(5, 128, device=dev, dtype=torch.bfloat16)
    dout = torch.randn(5, 64, device=dev, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        hip.swiglu_gu_bwd_t(dout, gu)
    gu = torch.randn(64, 80, device=dev, dtype=torch.bfloat16)
    dout = torch.randn(64, 40, device=dev, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        hip.swiglu_gu_bwd_t(dout, gu)


@pytest.mark.parametrize("rows", [5, 192])
def test_linear_swiglu_equals_separate_ops(dev, rows):
    """linear_swiglu against swiglu_packed(fast_linear()): same bits for
    the output and both grads; rows=5 is off the fused kernel's entry
    point and runs the plain swiglu_gu_bwd. swiglu_packed itself against
    the kernel it has always called."""
    ops = _ops()
    hip = ops.hip_ops()
    torch.manual_seed(3)
    K, inter = 256, 192
    x = torch.randn(rows, K, device=dev, dtype=torch.bfloat16)
    w = torch.randn(2 * inter, K, device=dev, dtype=torch.bfloat16) * 0.05
    dh = torch.randn(rows, inter, device=dev, dtype=torch.bfloat16)

    gu = (x @ w.t()).requires_grad_(True)
    h_old = ops.swiglu_packed(gu)
    assert torch.equal(h_old, hip.swiglu_gu_fwd(gu.detach()))
    h_old.backward(dh)
    assert torch.equal(gu.grad, hip.swiglu_gu_bwd(dh, gu.detach()))

    res = []
    for fn in (lambda a, b: ops.swiglu_packed(ops.fast_linear(a, b)),
               ops.linear_swiglu):
        xa = x.clone().requires_grad_(True)
        wa = w.clone().requires_grad_(True)
        h = fn(xa, wa)
        h.backward(dh)
        res.append((h.detach(), xa.grad, wa.grad))
    assert torch.equal(res[0][0], h_old.detach())
    for old, new in zip(res[0], res[1]):
        assert torch.equal(old, new)


# ---------------------------------------------------------------------------
# fast_linear wgrad
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("M,N,K", [(64, 64, 64), (192, 128, 320),
                                   (256, 12288, 1024)])
@pytest.mark.parametrize("slot", ["none", "first", "second"])
def test_fast_linear_wgrad(dev, M, N, K, slot):
    ops = _ops()
    hip = ops.hip_ops()
    torch.manual_seed(M + N + K)
    x = torch.randn(M, K, device=dev, dtype=torch.bfloat16,
                    requires_grad=True)
    w = (torch.randn(N, K, device=dev, dtype=torch.bfloat16)
         * 0.05).requires_grad_(True)
    dy = torch.randn(M, N, device=dev, dtype=torch.bfloat16)
    ref = dy.double().t() @ x.detach().double()
    if slot == "first":
        # as FlatParams.zero_grad leaves it: zeroed slot, first-touch flag
        w.grad = torch.zeros_like(w)
        w._wgrad_fresh = True
    elif slot == "second":
        seed = torch.randn_like(w) * (M ** 0.5)  # the size of dy^T x
        w.grad = seed.clone()
        w._wgrad_fresh = False
        ref = seed.double() + ref
    slot_ptr = w.grad.data_ptr() if w.grad is not None else None
    ops.fast_linear(x, w).backward(dy)
    if slot_ptr is not None:
        assert w.grad.data_ptr() == slot_ptr  # accumulated in place
        assert w._wgrad_fresh is False
    err = _nrel(w.grad, ref)
    print(f"fast_linear wgrad M={M} N={N} K={K} slot={slot}: "
          f"nrel={err:.3e} bound={BOUND:.3e}")
    assert err <= BOUND
    # dgrad is untouched: dy @ Wt^T with Wt = transpose_bf16(W)
    assert torch.equal(x.grad, dy @ hip.transpose_bf16(w.detach()).t())


# ---------------------------------------------------------------------------
# lm_head wgrad inside fused_linear_cross_entropy
# ---------------------------------------------------------------------------


@pytest.fixture(scope="module")
def ce_case(dev):
    torch.manual_seed(11)
    T, H, V = 384, 1024, 4096
    x = torch.randn(T, H, device=dev, dtype=torch.bfloat16)
    w = torch.randn(V, H, device=dev, dtype=torch.bfloat16) * 0.02
    targets = torch.randint(0, V, (T,), device=dev)
    xr = x.double()
    wr = w.double().requires_grad_(True)
    torch.nn.functional.cross_entropy(xr @ wr.t(), targets).backward()
    return x, w, targets, wr.grad


@pytest.mark.parametrize("chunk", [128, 16384])
def test_fused_linear_ce(dev, ce_case, chunk):
    ops = _ops()
    hip = ops.hip_ops()
    x, w, targets, dw_ref = ce_case
    T = x.shape[0]
    xa = x.clone().requires_grad_(True)
    wa = w.clone().requires_grad_(True)
    loss = ops.fused_linear_cross_entropy(xa, wa, targets, chunk=chunk)
    # the op's forward as it has always been: per chunk the logits GEMM and
    # ce_fwd, chunk sums added in fp32 in order, scaled by 1/T at the end
    loss_sum = torch.zeros((), device=dev, dtype=torch.float32)
    for s in range(0, T, chunk):
        e = min(T, s + chunk)
        loss_c, _ = hip.ce_fwd(x[s:e] @ w.t(), targets[s:e].contiguous())
        loss_sum += loss_c.sum()
    assert torch.equal(loss.detach(), loss_sum * (1.0 / T))
    loss.backward()
    err = _nrel(wa.grad, dw_ref)
    print(f"fused_linear_ce chunk={chunk}: dW nrel={err:.3e} "
          f"bound={BOUND:.3e}")
    assert err <= BOUND


# ---------------------------------------------------------------------------
# model: the forward is untouched
# ---------------------------------------------------------------------------


def test_llama_gpu_tiny_loss_unchanged(dev, monkeypatch):
    from torchx_amd import ops
    from torchx_amd.models import llama

    torch.manual_seed(0)
    cfg = llama.llama_gpu_tiny()
    model = llama.LlamaModel(cfg, device=dev)
    tokens = torch.randint(0, cfg.vocab_size, (2, 256), device=dev)
    targets = torch.roll(tokens, -1, 1)
    loss = model(tokens, targets).detach().clone()
    # the block as it was composed before linear_swiglu
    monkeypatch.setattr(
        llama, "_lin_swiglu",
        lambda mod, x: ops.swiglu_packed(llama._lin(mod, x)))
    loss_old = model(tokens, targets).detach()
    assert torch.equal(loss, loss_old)
