"""torchx_amd.ops — CDNA4 HIP hot-op library with autograd bindings.

On a GPU (MI355X) these ops REQUIRE the in-tree `_hip_ops.so` extension and
fail loudly if it is missing — there is no silent eager fallback on the GPU
path.  On CPU (CI containers have no GPU) they fall back to the fp32 torch
reference implementations in `torchx_amd.ops.reference`, which are also the
ground truth the GPU numerics tests compare against.
"""

from __future__ import annotations

import importlib.util
import math
import os
from pathlib import Path
from typing import Optional, Sequence, Tuple

import torch

from . import reference

_SO = Path(__file__).resolve().parent / "_hip_ops.so"
_hip = None
_load_err: Optional[str] = None


def _load():
    global _hip, _load_err
    if _hip is not None:
        return _hip
    if not _SO.exists():
        _load_err = f"{_SO} not built (run torchx_amd/ops/build.py)"
        return None
    try:
        # name must match TORCH_EXTENSION_NAME (PyInit__hip_ops)
        spec = importlib.util.spec_from_file_location("_hip_ops", _SO)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)  # type: ignore[union-attr]
        _hip = mod
    except Exception as e:  # noqa: BLE001
        _load_err = str(e)
    return _hip


def hip_ops(required: bool = True):
    """The raw extension module.  On a GPU box this must exist."""
    mod = _load()
    if mod is None and required:
        raise RuntimeError(
            f"torchx_amd HIP extension not available: {_load_err}. "
            "GPU execution requires the native kernels; refusing to fall "
            "back to eager."
        )
    return mod


def extension_available() -> bool:
    return _load() is not None


def _on_gpu(*ts: torch.Tensor) -> bool:
    return any(t.is_cuda for t in ts)


# ---------------------------------------------------------------------------
# RMSNorm
# ---------------------------------------------------------------------------


class _RMSNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor, w: torch.Tensor, eps: float):
        y, invrms = hip_ops().rmsnorm_fwd(x.contiguous(), w.contiguous(), eps)
        ctx.save_for_backward(x, w, invrms)
        return y

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        x, w, invrms = ctx.saved_tensors
        dx, dw = hip_ops().rmsnorm_bwd(dy.contiguous(), x, w, invrms)
        return dx, dw.to(w.dtype), None


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    if _on_gpu(x):
        return _RMSNorm.apply(x, w, eps)
    return reference.rmsnorm(x, w, eps)


class _AddRMSNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor, delta: torch.Tensor, w: torch.Tensor,
                eps: float):
        s, y, invrms = hip_ops().add_rmsnorm_fwd(
            x.contiguous(), delta.contiguous(), w.contiguous(), eps)
        ctx.save_for_backward(s, w, invrms)
        # an unused output (s behind the final norm) arrives as None, not
        # as a zero tensor to be added
        ctx.set_materialize_grads(False)
        return s, y

    @staticmethod
    def backward(ctx, ds: Optional[torch.Tensor],
                 dy: Optional[torch.Tensor]):
        if dy is None:
            return ds, ds, None, None
        s, w, invrms = ctx.saved_tensors
        # ds rides along: the dx kernel adds it to its own (bf16-rounded)
        # dx, which is the accumulate-add autograd would run at the fork
        dx, dw = hip_ops().rmsnorm_bwd(
            dy.contiguous(), s, w, invrms,
            ds.contiguous() if ds is not None else None)
        return dx, dx, dw.to(w.dtype), None


def add_rmsnorm(x: torch.Tensor, delta: torch.Tensor, w: torch.Tensor,
                eps: float = 1e-5) -> Tuple[torch.Tensor, torch.Tensor]:
    """Residual add fused into the RMSNorm that consumes it: returns
    ``(s, y)`` with ``s = x + delta`` (the new residual stream, bf16) and
    ``y = rmsnorm(s, w)``. One kernel forward and one dx kernel backward
    instead of add + norm and norm-dx + accumulate-add; outputs and the
    grads of ``x``, ``delta`` and ``w`` are bit-identical to the unfused
    pair."""
    if _on_gpu(x):
        return _AddRMSNorm.apply(x, delta, w, eps)
    s = x + delta
    return s, reference.rmsnorm(s, w, eps)


# ---------------------------------------------------------------------------
# RoPE
# ---------------------------------------------------------------------------


def rope_tables(
    seq_len: int, head_dim: int, theta: float = 500000.0,
    device: Optional[torch.device] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Host-precomputed f32 cos/sin tables [S, D/2] (guide: on-device trig
    turns a memory-bound elementwise op VALU-bound)."""
    inv_freq = 1.0 / (
        theta ** (torch.arange(0, head_dim, 2, dtype=torch.float32) / head_dim)
    )
    pos = torch.arange(seq_len, dtype=torch.float32)
    ang = torch.outer(pos, inv_freq)  # [S, D/2]
    cos, sin = torch.cos(ang), torch.sin(ang)
    if device is not None:
        cos, sin = cos.to(device), sin.to(device)
    return cos, sin


class _RoPE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
                heads: int):
        ctx.save_for_backward(cos, sin)
        ctx.heads = heads
        return hip_ops().rope(x.contiguous(), cos, sin, heads, 1.0)

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        cos, sin = ctx.saved_tensors
        dx = hip_ops().rope(dy.contiguous(), cos, sin, ctx.heads, -1.0)
        return dx, None, None, None


def rope(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """x: [B, S, H, D] bf16; rotate-half (Llama) convention. cos/sin are
    f32 [>= S, D/2] tables; position s uses row s."""
    heads = x.shape[2]
    if _on_gpu(x):
        # the kernel takes a row's position modulo the table length, so it
        # gets exactly the S rows this x uses
        S = x.shape[1]
        if cos.shape[0] < S or sin.shape[0] < S:
            raise ValueError(
                f"rope: tables of {cos.shape[0]} rows for a sequence of {S}")
        return _RoPE.apply(x, cos[:S], sin[:S], heads)
    return reference.rope(x, cos, sin)


# ---------------------------------------------------------------------------
# SwiGLU
# ---------------------------------------------------------------------------


class _SwiGLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g: torch.Tensor, u: torch.Tensor):
        g, u = g.contiguous(), u.contiguous()
        ctx.save_for_backward(g, u)
        return hip_ops().swiglu_fwd(g, u)

    @staticmethod
    def backward(ctx, dout: torch.Tensor):
        g, u = ctx.saved_tensors
        dg, du = hip_ops().swiglu_bwd(dout.contiguous(), g, u)
        return dg, du


def swiglu(g: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    if _on_gpu(g):
        return _SwiGLU.apply(g, u)
    return reference.swiglu(g, u)


# ---------------------------------------------------------------------------
# Fused cross entropy (mean reduction over T tokens)
# ---------------------------------------------------------------------------


class _CrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits: torch.Tensor, targets: torch.Tensor):
        V = logits.shape[-1]
        logits2d = logits.contiguous().view(-1, V)
        targets = targets.contiguous().view(-1)
        loss, lse = hip_ops().ce_fwd(logits2d, targets)
        ctx.save_for_backward(logits2d, targets, lse)
        ctx.orig_shape = logits.shape
        return loss.mean()

    @staticmethod
    def backward(ctx, gout: torch.Tensor):
        logits2d, targets, lse = ctx.saved_tensors
        T = logits2d.shape[0]
        gscale = (gout.float() / T).expand(T).contiguous()
        dlogits = hip_ops().ce_bwd(logits2d, targets, lse, gscale)
        return dlogits.view(ctx.orig_shape), None


def cross_entropy(logits: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
    """Mean cross entropy of logits [..., V] bf16 against int64 targets.
    ``ignore_index`` is not supported on the GPU path: every target must lie
    in [0, V). A target outside it (torch's default -100 included, which
    the CPU path skips) gives that row a NaN loss, and with it a NaN mean;
    its dlogits row is the plain softmax."""
    if _on_gpu(logits):
        return _CrossEntropy.apply(logits, targets)
    return reference.cross_entropy(logits, targets)


# ---------------------------------------------------------------------------
# Fused lm_head GEMM + cross entropy (chunked — the [T, V] logits are never
# fully materialized or saved).  The CE loss is the last op of the step, so
# its input grads are known in forward up to the scalar gout: each token
# chunk runs  logits GEMM -> ce_fwd -> ce_bwd -> dx GEMM -> dW accumulation
# back-to-back while the chunk's logits are hot, then the chunk buffers are
# recycled.  dW accumulates in fp32 (bf16 += across chunks would drift).
# Cuts the saved-tensor footprint by 2*T*V bf16 (8.4 GB at the bench shape)
# and keeps the GEMM sizes fat (chunk=4096 rows).
# ---------------------------------------------------------------------------


class _FusedLinearCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x2: torch.Tensor, w: torch.Tensor,
                targets: torch.Tensor, chunk: int):
        hip = hip_ops()
        T, H = x2.shape
        dx = torch.empty_like(x2)
        single = T <= chunk
        # multi-chunk dW accumulates in fp32 (bf16 += across chunks drifts);
        # a single chunk writes the bf16 wgrad GEMM output directly
        dw_acc = None if single else torch.zeros_like(w, dtype=torch.float32)
        loss_sum = torch.zeros((), device=x2.device, dtype=torch.float32)
        inv_t = 1.0 / T
        gscale = torch.full((min(chunk, T),), inv_t, device=x2.device,
                            dtype=torch.float32)
        # dx via the transposed-weight operand order (same ~15% dgrad win
        # as fast_linear); w transposed once for all chunks
        wt = (hip.transpose_bf16(w)
              if w.shape[0] % 64 == 0 and w.shape[1] % 64 == 0 else None)
        for s in range(0, T, chunk):
            e = min(T, s + chunk)
            x_c = x2[s:e]
            t_c = targets[s:e].contiguous()
            logits_c = x_c @ w.t()
            loss_c, lse_c = hip.ce_fwd(logits_c, t_c)
            loss_sum += loss_c.sum()
            dlog_c = hip.ce_bwd(logits_c, t_c, lse_c, gscale[:e - s])
            # the logits are dead from here: released before dW is allocated
            del logits_c
            if wt is not None:
                torch.matmul(dlog_c, wt.t(), out=dx[s:e])
            else:
                torch.matmul(dlog_c, w, out=dx[s:e])
            # the wgrad stays dlog^T @ x: from transposed operands (see
            # _wgrad) it is 13% faster at the lm_head shape, but there the
            # stream-K TN kernel splits tiles and sums them in another
            # order — ~10^4 of 5*10^8 elements round to the other bf16,
            # and 15 AdamW steps turn that into another loss curve. The
            # wgu shape has no such tiles: same bits either way.
            if single:
                dw_acc = dlog_c.t() @ x_c
            else:
                dw_acc += dlog_c.t() @ x_c
            del dlog_c
        ctx.save_for_backward(dx, dw_acc)
        return loss_sum * inv_t

    @staticmethod
    def backward(ctx, gout: torch.Tensor):
        dx, dw_acc = ctx.saved_tensors
        # single scale(+cast) pass for dW; dx scales in place
        if dw_acc.dtype == dx.dtype:
            dw = dw_acc * gout.to(dx.dtype)
        else:
            dw = (dw_acc * gout.to(torch.float32)).to(dx.dtype)
        dx = dx * gout.to(dx.dtype)
        return dx, dw, None, None


def fused_linear_cross_entropy(
    x: torch.Tensor, w: torch.Tensor, targets: torch.Tensor,
    chunk: int = 16384,
) -> torch.Tensor:
    """mean CE of ``x @ w.T`` against ``targets`` without materializing the
    full logits. x [..., H] bf16, w [V, H] bf16, targets [...] int64."""
    H = x.shape[-1]
    x2 = x.reshape(-1, H)
    t = targets.reshape(-1)
    if _on_gpu(x):
        if torch.is_grad_enabled() and (x.requires_grad or w.requires_grad):
            return _FusedLinearCE.apply(x2.contiguous(), w, t, chunk)
        # eval path: loss only, no dx/dW work
        hip = hip_ops()
        x2 = x2.contiguous()
        T = x2.shape[0]
        loss_sum = torch.zeros((), device=x.device, dtype=torch.float32)
        for s in range(0, T, chunk):
            e = min(T, s + chunk)
            loss_c, _ = hip.ce_fwd(x2[s:e] @ w.t(), t[s:e].contiguous())
            loss_sum += loss_c.sum()
        return loss_sum / T
    return reference.cross_entropy(x2 @ w.t(), t)


# ---------------------------------------------------------------------------
# Flash attention (causal, GQA), BSHD layout
# ---------------------------------------------------------------------------


class _FlashAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                causal: bool, scale: float):
        o, lse = hip_ops().attn_fwd(
            q.contiguous(), k.contiguous(), v.contiguous(), scale, causal
        )
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.causal = causal
        ctx.scale = scale
        return o

    @staticmethod
    def backward(ctx, dout: torch.Tensor):
        q, k, v, o, lse = ctx.saved_tensors
        dq, dk, dv = hip_ops().attn_bwd(
            q, k, v, o, dout.contiguous(), lse, ctx.scale, ctx.causal
        )
        return dq, dk, dv, None, None


def set_attn_bwd_dq_mode(mode: str) -> None:
    """Select the dQ path of the attention backward: "stream" (default; the
    dkv kernel exports dS and dQ is one streamed GEMM over it) or
    "recompute" (the dQ kernel rebuilds dS itself).  The initial value comes
    from TORCHX_AMD_DQ_MODE."""
    hip_ops().set_attn_bwd_dq_mode(mode)


def get_attn_bwd_dq_mode() -> str:
    return hip_ops().get_attn_bwd_dq_mode()


def set_attn_bwd_dkv_impl(impl: str) -> None:
    """Select the dK/dV kernel of the attention backward: "merged" (default;
    one wave per SIMD accumulates both outputs, so S, P and dP are computed
    once) or "split" (separate dV and dK waves).  Both produce the same
    bits.  The initial value comes from TORCHX_AMD_DKV_IMPL."""
    hip_ops().set_attn_bwd_dkv_impl(impl)


def get_attn_bwd_dkv_impl() -> str:
    return hip_ops().get_attn_bwd_dkv_impl()


def set_attn_fwd_map(name: str) -> None:
    """Select the block map of the dense attention forward: "balanced"
    (default; the G heads of a (batch, kv head, q tile) adjacent on one
    XCD, heaviest tiles dispatched first), "legacy" (whole (batch, kv head)
    groups, q tiles ascending) or "adjacent" (the balanced layout with
    tiles ascending, for A/B).  All produce the same bits.  The initial
    value comes from TORCHX_AMD_FWD_MAP."""
    hip_ops().set_attn_fwd_map(name)


def get_attn_fwd_map() -> str:
    return hip_ops().get_attn_fwd_map()


def flash_attention(
    q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
    causal: bool = True, scale: Optional[float] = None,
) -> torch.Tensor:
    """q [B,S,Hq,D], k/v [B,S,Hkv,D] bf16 -> o [B,S,Hq,D]."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if _on_gpu(q):
        return _FlashAttention.apply(q, k, v, causal, scale)
    return reference.attention(q, k, v, causal=causal, scale=scale)


# ---------------------------------------------------------------------------
# Fused AdamW (flat-buffer optimizer step; see torchx_amd.parallel.optim)
# ---------------------------------------------------------------------------


def adamw_step(
    p32: torch.Tensor, p16: torch.Tensor, grad: torch.Tensor,
    m: torch.Tensor, v: torch.Tensor, *, lr: float, beta1: float = 0.9,
    beta2: float = 0.95, eps: float = 1e-8, weight_decay: float = 0.1,
    step: int = 1,
) -> None:
    if p32.is_cuda:
        hip_ops().adamw_step(p32, p16, grad, m, v, lr, beta1, beta2, eps,
                             weight_decay, step)
    else:
        reference.adamw_step(p32, p16, grad, m, v, lr=lr, beta1=beta1,
                             beta2=beta2, eps=eps, weight_decay=weight_decay,
                             step=step)


def mfma_probe(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return hip_ops().mfma_probe(a, b)


# ---------------------------------------------------------------------------
# fast_linear: bias-free linear whose dgrad uses the transposed-weight
# operand order.  dy @ Wt^T (Wt = transpose_bf16(W)) measures ~15% faster
# than dy @ W on every llama GEMM shape (tools/gemm_probe.py dgrad-NT vs
# dgrad-NN, ~1.55 vs ~1.33 PF/s); the transpose itself is an LDS-tiled
# kernel at HBM rate (~0.06 ms for the largest weight), so the swap nets
# ~17 ms/step at the bench config.
# ---------------------------------------------------------------------------


class _FastLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor, w: torch.Tensor):
        ctx.save_for_backward(x, w)
        return x @ w.t()

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        x, w = ctx.saved_tensors
        hip = hip_ops()
        wt = hip.transpose_bf16(w)                      # [K, N]
        dy2 = dy.reshape(-1, dy.shape[-1]).contiguous()
        x2 = x.reshape(-1, x.shape[-1])
        dx = (dy2 @ wt.t()).view_as(x)
        return dx, _wgrad(hip, w, dy2, x2)


def _wgrad(hip, w: torch.Tensor, dy2: torch.Tensor, x2: torch.Tensor,
           dyt: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """dW [N, K] = dy2^T [N, M] @ x2 [M, K] of a fast_linear weight, in the
    operand form that tools/gemm_probe.py --wgrad measures fastest for the
    shape (transposes included):
      - fat outputs (the gu shape): both operands transposed,
        dyT @ xT^T — both contiguous along the reduction dimension M, which
        is the form of the forward GEMM (~1.35 vs ~1.2 PF/s); at the gu
        shape the result has the bits of dy^T @ x;
      - narrow outputs (qkv/wo/down shapes): dy transposed once, dyT @ x;
        transposing x as well gains less than its own transpose costs;
      - M or N not a multiple of 64: plain dy^T @ x.
    ``dyt`` is dy2 already transposed, if the producer of dy2 had it.
    Returns dW, or None after accumulating into the weight's grad slot."""
    M, N = dy2.shape
    K = x2.shape[1]
    aligned = M % 64 == 0 and N % 64 == 0
    both_t = aligned and N > 8192 and K % 64 == 0
    if both_t or (aligned and N <= 8192):
        a = dyt if dyt is not None else hip.transpose_bf16(dy2)
    else:
        a = dy2.t()
    b = hip.transpose_bf16(x2.contiguous()).t() if both_t else x2
    # direct accumulation: when the param already has a (flat-buffer)
    # grad slot, the wgrad GEMM accumulates straight into it with
    # beta=1 — no dw buffer write/read and no AccumulateGrad RMW pass.
    # Safe because each weight is consumed once per step; the DDP
    # bucket hook is notified manually (grad_ready).
    wg = w.grad if w.is_leaf else None
    if wg is not None and wg.is_contiguous():
        if getattr(w, "_wgrad_fresh", False):
            # first touch since zero_grad: overwrite (beta=0) — skips
            # both the zeroed-C read in the GEMM and staleness
            torch.matmul(a, b, out=wg)
            w._wgrad_fresh = False
        else:
            wg.addmm_(a, b)
        from torchx_amd.parallel.ddp import grad_ready

        grad_ready(w)
        return None
    return a @ b


def fast_linear(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """``x @ w.T`` with the NT-dgrad backward; falls back to F.linear off
    the fast path (CPU, or dims not 64-aligned)."""
    if (x.is_cuda and w.dtype == torch.bfloat16
            and w.shape[0] % 64 == 0 and w.shape[1] % 64 == 0):
        return _FastLinear.apply(x, w)
    return torch.nn.functional.linear(x, w)


# ---------------------------------------------------------------------------
# Fused qkv attention: rope(q,k) + flash attention straight off the packed
# qkv GEMM output — no split/contiguous copies forward, no torch.cat
# backward (the grads dq/dk/dv are written strided into one dqkv buffer and
# inverse-roped in place).
# ---------------------------------------------------------------------------


class _FusedAttentionQKV(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
                Hq: int, Hkv: int, causal: bool, scale: float):
        hip = hip_ops()
        roped = hip.rope_qkv(qkv.contiguous(), cos, sin, Hq, Hkv, 1.0, False)
        o, lse = hip.attn_fwd_qkv(roped, Hq, Hkv, scale, causal)
        ctx.save_for_backward(roped, o, lse, cos, sin)
        ctx.dims = (Hq, Hkv, causal, scale)
        return o

    @staticmethod
    def backward(ctx, dout: torch.Tensor):
        roped, o, lse, cos, sin = ctx.saved_tensors
        Hq, Hkv, causal, scale = ctx.dims
        hip = hip_ops()
        dqkv = hip.attn_bwd_qkv(roped, o, dout.contiguous(), lse, Hq, Hkv,
                                scale, causal)
        # inverse rotation on the dq/dk regions, in place on our own buffer
        hip.rope_qkv(dqkv, cos, sin, Hq, Hkv, -1.0, True)
        return dqkv, None, None, None, None, None, None


def fused_attention_qkv(
    qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
    Hq: int, Hkv: int, causal: bool = True,
    scale: Optional[float] = None,
) -> torch.Tensor:
    """qkv [B, S, (Hq+2*Hkv)*128] bf16 -> o [B, S, Hq, 128]."""
    D = qkv.shape[-1] // (Hq + 2 * Hkv)
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    if _on_gpu(qkv):
        return _FusedAttentionQKV.apply(qkv, cos, sin, Hq, Hkv, causal, scale)
    # CPU reference path: split + rope + attention
    B, S, _ = qkv.shape
    q, k, v = qkv.split([Hq * D, Hkv * D, Hkv * D], dim=-1)
    q = reference.rope(q.reshape(B, S, Hq, D), cos, sin)
    k = reference.rope(k.reshape(B, S, Hkv, D), cos, sin)
    return reference.attention(q, k, v.reshape(B, S, Hkv, D),
                               causal=causal, scale=scale)


class _SwiGLUPacked(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gu: torch.Tensor):
        gu = gu.contiguous()
        ctx.save_for_backward(gu)
        return hip_ops().swiglu_gu_fwd(gu)

    @staticmethod
    def backward(ctx, dout: torch.Tensor):
        (gu,) = ctx.saved_tensors
        return hip_ops().swiglu_gu_bwd(dout.contiguous(), gu)


def swiglu_packed(gu: torch.Tensor) -> torch.Tensor:
    """gu [..., 2I] (gate | up) -> silu(gate) * up, [..., I]."""
    if _on_gpu(gu):
        return _SwiGLUPacked.apply(gu)
    g, u = gu.chunk(2, dim=-1)
    return reference.swiglu(g, u)


class _LinearSwiGLU(torch.autograd.Function):
    """fast_linear + swiglu_packed as one autograd node, so that the SwiGLU
    backward can hand the wgrad its input already transposed: dgu and
    dgu^T come out of one kernel (swiglu_gu_bwd_t) instead of dgu being
    read back by a stand-alone transpose.  Forward and saved tensors are
    those of the two separate nodes."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, w: torch.Tensor):
        hip = hip_ops()
        gu = x @ w.t()
        ctx.save_for_backward(x, w, gu)
        return hip.swiglu_gu_fwd(gu)

    @staticmethod
    def backward(ctx, dout: torch.Tensor):
        x, w, gu = ctx.saved_tensors
        hip = hip_ops()
        dout = dout.contiguous()
        gu2 = gu.view(-1, gu.shape[-1])
        if gu2.shape[0] % 64 == 0 and gu2.shape[1] % 128 == 0:
            dgu2, dgut = hip.swiglu_gu_bwd_t(dout.view(-1, dout.shape[-1]),
                                             gu2)
        else:
            dgu2, dgut = hip.swiglu_gu_bwd(dout, gu2), None
        wt = hip.transpose_bf16(w)                      # [K, N]
        dx = (dgu2 @ wt.t()).view_as(x)
        return dx, _wgrad(hip, w, dgu2, x.reshape(-1, x.shape[-1]), dgut)


def linear_swiglu(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """``swiglu_packed(fast_linear(x, w))`` for the packed gate|up weight
    ``w`` [2I, K]: the same values forward and backward, with the wgrad's
    transposed operand written by the SwiGLU backward kernel itself. Off
    the fast path (CPU, dims not 64-aligned) it is the two separate ops."""
    if (x.is_cuda and w.dtype == torch.bfloat16 and x.dtype == w.dtype
            and w.shape[0] % 64 == 0 and w.shape[1] % 64 == 0):
        return _LinearSwiGLU.apply(x, w)
    return swiglu_packed(fast_linear(x, w))


# ---------------------------------------------------------------------------
# Decode attention (serving): single-position attention over a KV cache —
# ops/csrc/decode_attn.hip, flash-decode style (wave-local online softmax,
# one merge barrier). No training/backward path: inference only.
# ---------------------------------------------------------------------------


def decode_attention(q: torch.Tensor, kcache: torch.Tensor,
                     vcache: torch.Tensor, length: int,
                     scale: Optional[float] = None) -> torch.Tensor:
    """q [B, Hq, 128] bf16; k/v caches [B, T, Hkv, 128] bf16 with the
    first ``length`` positions valid -> o [B, Hq, 128]."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if _on_gpu(q):
        return hip_ops().decode_attn(q.contiguous(), kcache, vcache,
                                     length, scale)
    return reference.decode_attention(q, kcache, vcache, length, scale)


def rmsnorm_res(x: torch.Tensor, res: Optional[torch.Tensor],
                w: torch.Tensor, eps: float = 1e-5):
    """Fused residual-add + RMSNorm for the decode path: returns
    ``(s, y)`` with ``s = x + res`` (the new residual stream, ``x`` when
    ``res`` is None) and ``y = rmsnorm(s) * w``. Inference only."""
    if _on_gpu(x):
        s, y = hip_ops().rmsnorm_res(x.contiguous(),
                                     res.contiguous() if res is not None
                                     else None, w.contiguous(), eps)
        return s, y
    s = x if res is None else (x + res)
    return s, reference.rmsnorm(s, w, eps)


def decode_rope_cache(qkv: torch.Tensor, kcache: torch.Tensor,
                      vcache: torch.Tensor, cos: torch.Tensor,
                      sin: torch.Tensor, pos,
                      num_heads: int) -> torch.Tensor:
    """Fused decode rope + KV-cache append: qkv [B, (Hq+2*Hkv)*D] for one
    position -> roped q [B, Hq, D]; ropes k and appends k/v to the caches
    at row ``pos`` (host int, or int32 device scalar for hipGraph capture).
    cos/sin are the FULL f32 [S, D/2] tables."""
    B = qkv.shape[0]
    Hkv, D = kcache.shape[2], kcache.shape[3]
    if _on_gpu(qkv):
        if isinstance(pos, torch.Tensor):
            return hip_ops().decode_rope_cache(qkv.contiguous(), kcache,
                                               vcache, cos, sin, 0, pos)
        return hip_ops().decode_rope_cache(qkv.contiguous(), kcache, vcache,
                                           cos, sin, int(pos), None)
    q, k, v = qkv.split([num_heads * D, Hkv * D, Hkv * D], dim=-1)
    q = q.reshape(B, 1, num_heads, D)
    k = k.reshape(B, 1, Hkv, D)
    v = v.reshape(B, 1, Hkv, D)
    if isinstance(pos, torch.Tensor) and pos.numel() > 1:
        outs = []  # ragged: each row ropes/appends at its own position
        for b in range(B):
            p = int(pos[b].item())
            cs, sn = cos[p:p + 1], sin[p:p + 1]
            outs.append(rope(q[b:b + 1].contiguous(), cs, sn))
            kcache[b, p:p + 1] = rope(k[b:b + 1].contiguous(), cs, sn)[0]
            vcache[b, p:p + 1] = v[b]
        return torch.cat(outs, dim=0).reshape(B, num_heads, D)
    p = int(pos.item()) if isinstance(pos, torch.Tensor) else int(pos)
    cs, sn = cos[p:p + 1], sin[p:p + 1]
    q = rope(q.contiguous(), cs, sn)
    k = rope(k.contiguous(), cs, sn)
    kcache[:, p:p + 1] = k
    vcache[:, p:p + 1] = v
    return q.reshape(B, num_heads, D)


# ---------------------------------------------------------------------------
# W8A16 decode weights: fp8 e4m3 rows with one fp32 scale each, consumed by
# the gemv_fp8.hip and gemm_fp8w_mfma.hip kernels. ``decode_linear`` / ``decode_linear_swiglu``
# take an ``Fp8Weight`` wherever they take a bf16 weight tensor.
# ---------------------------------------------------------------------------

FP8_E4M3_MAX = 448.0


class Fp8Weight:
    """A row-scaled fp8 weight: ``w8`` [N, K] float8_e4m3fn and ``scale``
    [N] fp32; the weight it stands for is ``w8 * scale[:, None]``."""

    def __init__(self, w8: torch.Tensor, scale: torch.Tensor):
        assert w8.dim() == 2 and w8.dtype == torch.float8_e4m3fn
        assert scale.dtype == torch.float32 and scale.shape == w8.shape[:1]
        self.w8 = w8.contiguous()
        self.scale = scale.contiguous()

    @property
    def shape(self) -> Tuple[int, int]:
        return tuple(self.w8.shape)

    def dequant(self) -> torch.Tensor:
        return self.w8.float() * self.scale[:, None]

    def to(self, device) -> "Fp8Weight":
        return Fp8Weight(self.w8.to(device), self.scale.to(device))


def quantize_fp8_rows(w: torch.Tensor) -> Fp8Weight:
    """Per-row absmax quantisation of w [N, K] to e4m3: ``scale[n] =
    amax_k |w[n, k]| / 448`` (1 for a zero row). A load-time one-off in
    torch. The quotient is clamped to +-448 before the cast: it can pass
    448 by one fp32 rounding, and the hardware convert turns overflow
    into NaN (docs/fp8.md)."""
    wf = w.detach().float()
    amax = wf.abs().amax(dim=1)
    scale = torch.where(amax > 0, amax / FP8_E4M3_MAX, torch.ones_like(amax))
    q = (wf / scale[:, None]).clamp_(-FP8_E4M3_MAX, FP8_E4M3_MAX)
    return Fp8Weight(q.to(torch.float8_e4m3fn), scale)


# Largest M that the dot2 kernels (gemv_fp8.hip) keep; M above it, up to 32,
# goes to the MFMA kernels (gemm_fp8w_mfma.hip). Measured on the four
# llama3-8B block shapes (profiles/README.md r13a): the MFMA kernels are
# faster on all four at M = 6, 7, 8 (by 2% on wqkv at M = 6, 22-58%
# elsewhere) and slower on wqkv at M = 4 and 5 (by 24% and 10%).
FP8W_DOT2_MAX_M = 5
FP8W_MAX_M = 32


def _fp8w_kernel_ok(x2: torch.Tensor, w: Fp8Weight) -> bool:
    """Whether x2 [M, K] bf16 against ``w`` runs on the fp8-weight kernels
    (any N: the bf16 path's N <= 32768 rule does not apply)."""
    M, K = x2.shape
    return _on_gpu(x2, w.w8, w.scale) and x2.dtype == torch.bfloat16 \
        and M <= FP8W_MAX_M and K % 1024 == 0


def decode_linear_swiglu(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """Fused decode MLP front half: ``silu(x @ gate.T) * (x @ up.T)`` for
    the packed wgu weight ``w = [gate; up]`` [2I, K] — one GEMV-shaped
    dispatch, no [M, 2I] intermediate. Inference only. The bf16 kernel
    takes M <= 8 rows, an ``Fp8Weight`` M <= 32 (see ``decode_linear``)."""
    x2 = x.reshape(-1, x.shape[-1])
    M, K = x2.shape
    if isinstance(w, Fp8Weight):
        if _fp8w_kernel_ok(x2, w):
            fn = hip_ops().gemv_swiglu_fp8w if M <= FP8W_DOT2_MAX_M \
                else hip_ops().gemm_swiglu_fp8w_mfma
            out = fn(x2.contiguous(), w.w8, w.scale)
        else:
            out = reference.decode_linear_swiglu_fp8w(x2, w.dequant())
    elif _on_gpu(x) and M <= 8 and K % 512 == 0 and w.shape[0] % 2 == 0 \
            and w.dtype == torch.bfloat16 and w.is_contiguous():
        out = hip_ops().gemv_swiglu_bf16(x2.contiguous(), w)
    else:
        gu = x2 @ w.t()
        g, u = gu.chunk(2, dim=-1)
        out = torch.nn.functional.silu(g.float()).to(u.dtype) * u
    return out.reshape(*x.shape[:-1], w.shape[0] // 2)


def decode_attention_dev(q: torch.Tensor, kcache: torch.Tensor,
                         vcache: torch.Tensor, pos: torch.Tensor,
                         scale: Optional[float] = None) -> torch.Tensor:
    """Decode attention with the cache position(s) read from a tensor:
    ``pos`` is int32, a scalar (all rows at the same position — the
    hipGraph path) or [B] (ragged / continuous batching — each sequence
    attends over its own ``pos[b] + 1`` cache rows)."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if _on_gpu(q):
        return hip_ops().decode_attn_dev(q.contiguous(), kcache, vcache,
                                         pos.contiguous(), scale)
    if pos.numel() == 1:
        return reference.decode_attention(q, kcache, vcache,
                                          int(pos.item()) + 1, scale)
    outs = [reference.decode_attention(q[b:b + 1], kcache[b:b + 1],
                                       vcache[b:b + 1],
                                       int(pos[b].item()) + 1, scale)
            for b in range(q.shape[0])]
    return torch.cat(outs, dim=0)


# ---------------------------------------------------------------------------
# fp8 KV cache (dense decode): k8 / v8 [B, T, Hkv, 128] float8_e4m3fn with
# one fp32 scale per (token, kv head) in ks / vs [B, T, Hkv]; the value stood
# for is ``k8 * ks[..., None]`` — ops/csrc/decode_attn_fp8kv.hip.
# ---------------------------------------------------------------------------


def quantize_kv_rows(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The KV-cache quantisation, by definition: per row of the last
    dimension, ``scale = amax |x| / 448`` (1 for a zero row) and
    ``x8 = e4m3(clamp(f32(x) / scale, -448, 448))``, both divisions in
    fp32 and the cast round-to-nearest-even. x [..., D] -> (x8 [..., D]
    float8_e4m3fn, scale [...] fp32). The HIP quantisers equal this bit
    for bit; it is also the CPU path. The clamp precedes the cast as in
    ``quantize_fp8_rows``. 448 is a tensor operand: torch turns a division
    by a Python scalar on the GPU into a multiplication by its reciprocal,
    which is not the IEEE quotient."""
    xf = x.detach().float()
    amax = xf.abs().amax(dim=-1)
    scale = torch.where(amax > 0,
                        amax / torch.full_like(amax, FP8_E4M3_MAX),
                        torch.ones_like(amax))
    y = (xf / scale[..., None]).clamp_(-FP8_E4M3_MAX, FP8_E4M3_MAX)
    return y.to(torch.float8_e4m3fn), scale


def dequantize_kv(x8: torch.Tensor, scale: torch.Tensor,
                  dtype=torch.float32) -> torch.Tensor:
    """``x8 * scale[..., None]`` in ``dtype``."""
    return x8.to(dtype) * scale[..., None].to(dtype)


def kv_quantize_store(k: torch.Tensor, v: torch.Tensor, k8: torch.Tensor,
                      v8: torch.Tensor, ks: torch.Tensor, vs: torch.Tensor,
                      start: int) -> None:
    """Quantise k, v [B, S, Hkv, 128] bf16 (k already roped) into rows
    ``start .. start+S-1`` of the fp8 cache, K and V in one launch."""
    S = k.shape[1]
    assert 0 <= start and start + S <= k8.shape[1], "rows outside the cache"
    if _on_gpu(k, k8):
        hip_ops().kv_quantize_store(k.contiguous(), v.contiguous(), k8, v8,
                                    ks, vs, int(start))
        return
    k8[:, start:start + S], ks[:, start:start + S] = quantize_kv_rows(k)
    v8[:, start:start + S], vs[:, start:start + S] = quantize_kv_rows(v)


def decode_rope_cache_fp8kv(qkv: torch.Tensor, k8: torch.Tensor,
                            v8: torch.Tensor, ks: torch.Tensor,
                            vs: torch.Tensor, cos: torch.Tensor,
                            sin: torch.Tensor, pos,
                            num_heads: int) -> torch.Tensor:
    """``decode_rope_cache`` over an fp8 cache: same qkv / ``pos`` contract
    and the same roped q; the roped, bf16-rounded k and the raw v are
    quantised (``quantize_kv_rows``) into row ``pos`` with their scales."""
    if _on_gpu(qkv):
        if isinstance(pos, torch.Tensor):
            return hip_ops().decode_rope_cache_fp8kv(
                qkv.contiguous(), k8, v8, ks, vs, cos, sin, 0,
                pos.contiguous())
        return hip_ops().decode_rope_cache_fp8kv(
            qkv.contiguous(), k8, v8, ks, vs, cos, sin, int(pos), None)
    # CPU: the bf16 op into a one-row scratch cache per sequence position
    B = qkv.shape[0]
    Hkv, D = k8.shape[2], k8.shape[3]
    kc = torch.zeros(B, 1, Hkv, D, dtype=qkv.dtype)
    vc = torch.zeros_like(kc)
    if isinstance(pos, torch.Tensor):
        rows = [int(p) for p in pos.reshape(-1).tolist()]
        rows = rows * B if len(rows) == 1 else rows
    else:
        rows = [int(pos)] * B
    outs = []
    for b, p in enumerate(rows):
        outs.append(decode_rope_cache(qkv[b:b + 1], kc[b:b + 1], vc[b:b + 1],
                                      cos[p:p + 1], sin[p:p + 1], 0,
                                      num_heads))
        k8[b, p], ks[b, p] = quantize_kv_rows(kc[b, 0])
        v8[b, p], vs[b, p] = quantize_kv_rows(vc[b, 0])
    return torch.cat(outs, dim=0)


def decode_attention_fp8kv(q: torch.Tensor, k8: torch.Tensor,
                           v8: torch.Tensor, ks: torch.Tensor,
                           vs: torch.Tensor, length_or_pos,
                           scale: Optional[float] = None,
                           split: Optional[int] = None) -> torch.Tensor:
    """Decode attention of q [B, Hq, 128] bf16 over an fp8 cache -> o
    [B, Hq, 128]. ``length_or_pos`` is a host int (the number of valid
    rows), or an int32 tensor of positions as in ``decode_attention_dev``
    (a scalar, or [B] for ragged rows; sequence b attends ``pos[b] + 1``
    rows). One block serves the q heads of a GQA group from one read of
    each row; Hq / Hkv must be 1, 2, 4 or 8. ``split`` forces the number
    of length slices (1 = single pass); by default the launcher picks it."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    dev_pos = isinstance(length_or_pos, torch.Tensor)
    if _on_gpu(q):
        return hip_ops().decode_attn_fp8kv(
            q.contiguous(), k8, v8, ks, vs,
            0 if dev_pos else int(length_or_pos),
            length_or_pos.contiguous() if dev_pos else None, scale,
            int(split or 0))
    # the fp32 reference over the fp32 dequantised caches
    kc = dequantize_kv(k8, ks)
    vc = dequantize_kv(v8, vs)
    if dev_pos:
        return decode_attention_dev(q, kc, vc, length_or_pos, scale)
    return reference.decode_attention(q, kc, vc, int(length_or_pos), scale)


# ---------------------------------------------------------------------------
# Paged KV cache (serving): block-table counterparts of decode_attention_dev
# and decode_rope_cache — ops/csrc/paged_attn.hip. kpool/vpool are
# [num_pages, P, Hkv, D]; block_table int32 [B, M] maps logical page j of
# sequence b to a physical page; pos int32 [B] as in decode_attention_dev.
# ---------------------------------------------------------------------------


def paged_decode_attention(q: torch.Tensor, kpool: torch.Tensor,
                           vpool: torch.Tensor, block_table: torch.Tensor,
                           pos: torch.Tensor,
                           scale: Optional[float] = None) -> torch.Tensor:
    """q [B, Hq, D]; each sequence attends over its own ``pos[b] + 1``
    logical cache rows, row t read from
    ``pool[block_table[b, t // P], t % P]`` -> o [B, Hq, D]. On the GPU
    the result is bit-identical to ``decode_attention_dev`` on the same
    logical cache."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if _on_gpu(q):
        return hip_ops().paged_decode_attn(q.contiguous(), kpool, vpool,
                                           block_table, pos.contiguous(),
                                           scale)
    outs = []
    for b in range(q.shape[0]):
        n = int(pos[b].item()) + 1
        outs.append(reference.decode_attention(
            q[b:b + 1], reference.paged_gather(kpool, block_table[b], n),
            reference.paged_gather(vpool, block_table[b], n), n, scale))
    return torch.cat(outs, dim=0)


def paged_prefill_attention(q: torch.Tensor, kpool: torch.Tensor,
                            vpool: torch.Tensor, block_table: torch.Tensor,
                            ctx: torch.Tensor,
                            scale: Optional[float] = None) -> torch.Tensor:
    """Causal attention of a prompt chunk behind a cached prefix. q
    [B, S, Hq, D] holds the rows at logical positions ``ctx[b] ..
    ctx[b]+S-1`` of sequence b; the pools already hold that sequence's
    ``ctx[b] + S`` rows (the chunk's own K/V included), row t at
    ``pool[block_table[b, t // P], t % P]``. Row i attends t <= ctx[b] + i
    -> o [B, S, Hq, D]. ``ctx`` is int32 [B]. On the GPU (D = 128), for
    ``ctx[b] % 128 == 0`` the result is bit-identical to rows ``ctx[b]:``
    of ``flash_attention`` (causal) over the gathered dense sequence."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if _on_gpu(q):
        return hip_ops().paged_prefill_attn(q.contiguous(), kpool, vpool,
                                            block_table, ctx.contiguous(),
                                            scale)
    S = q.shape[1]
    outs = []
    for b in range(q.shape[0]):
        c = int(ctx[b].item())
        outs.append(reference.attention_prefix(
            q[b:b + 1], reference.paged_gather(kpool, block_table[b], c + S),
            reference.paged_gather(vpool, block_table[b], c + S), c, scale))
    return torch.cat(outs, dim=0)


class RaggedPlan:
    """Host-side launch plan of ``paged_prefill_attention_ragged`` for one
    packing: ``q_lens`` (chunk length per sequence), ``cu`` (first packed
    row per sequence, plus the total ``T``) and the device tile list
    int32 [ntiles, 4] = (sequence, q tile, cu, chunk length), one entry per
    128-row q tile. Everything comes from host lengths, so building a plan
    never waits on the device; build it once per forward pass and hand it
    to every layer (one host-to-device copy in all).

    ``heavy_first`` lists the tiles by falling number of keys they attend
    (``ctx[b] + 128 * (qt + 1)``, from the host ``ctx`` if given), so the
    longest-running blocks are dispatched first; otherwise tiles are
    listed sequence by sequence."""

    HEAVY_FIRST = True

    def __init__(self, q_lens, device, ctx=None,
                 heavy_first: Optional[bool] = None):
        self.q_lens = [int(n) for n in q_lens]
        assert self.q_lens and min(self.q_lens) >= 1, "q_lens must be >= 1"
        self.cu = [0]
        for n in self.q_lens:
            self.cu.append(self.cu[-1] + n)
        self.T = self.cu[-1]
        ctx = [0] * len(self.q_lens) if ctx is None else [int(c) for c in ctx]
        assert len(ctx) == len(self.q_lens)
        tiles = [(b, qt, self.cu[b], n)
                 for b, n in enumerate(self.q_lens)
                 for qt in range(-(-n // 128))]
        if heavy_first is None:
            heavy_first = self.HEAVY_FIRST
        if heavy_first:
            # stable: equal costs keep the sequence order
            tiles.sort(key=lambda t: -(ctx[t[0]] + min(128 * (t[1] + 1),
                                                       t[3])))
        self.tiles_host = tiles
        self.tiles = torch.tensor(tiles, dtype=torch.int32, device=device)


def paged_prefill_attention_ragged(q: torch.Tensor, kpool: torch.Tensor,
                                   vpool: torch.Tensor,
                                   block_table: torch.Tensor, q_lens,
                                   ctx: torch.Tensor,
                                   scale: Optional[float] = None,
                                   plan: Optional[RaggedPlan] = None
                                   ) -> torch.Tensor:
    """``paged_prefill_attention`` over chunks of different lengths. q
    [T, Hq, D] holds the query rows of B sequences packed back to back:
    sequence b owns rows ``cu[b] .. cu[b]+q_lens[b]-1`` at logical
    positions ``ctx[b] ..``; the pools already hold its
    ``ctx[b] + q_lens[b]`` rows through ``block_table[b]``. ``q_lens`` is a
    host sequence of ints >= 1 summing to T, ``ctx`` int32 [B] on the
    device. Row i of sequence b attends t <= ctx[b] + i -> o [T, Hq, D].
    On the GPU (D = 128) sequence b's rows are bit-identical to
    ``paged_prefill_attention`` on that sequence alone, at every ctx.
    ``plan`` is the ``RaggedPlan`` of ``q_lens``; pass one plan to all
    layers of a forward pass (without it one is built per call)."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if plan is None:
        plan = RaggedPlan(q_lens, q.device)
    assert plan.q_lens == [int(n) for n in q_lens], "plan of other lengths"
    assert q.dim() == 3 and q.shape[0] == plan.T, (q.shape, plan.T)
    assert block_table.shape[0] == len(plan.q_lens) == ctx.numel()
    if _on_gpu(q):
        return hip_ops().paged_prefill_attn_ragged(
            q.contiguous(), kpool, vpool, block_table.contiguous(),
            ctx.contiguous(), plan.tiles, scale)
    outs = []
    for b, n in enumerate(plan.q_lens):
        c = int(ctx[b].item())
        qb = q[plan.cu[b]:plan.cu[b] + n][None]
        outs.append(reference.attention_prefix(
            qb, reference.paged_gather(kpool, block_table[b], c + n),
            reference.paged_gather(vpool, block_table[b], c + n), c,
            scale)[0])
    return torch.cat(outs, dim=0)


def paged_prefill_rope_cache(qkv: torch.Tensor, kpool: torch.Tensor,
                             vpool: torch.Tensor, cos: torch.Tensor,
                             sin: torch.Tensor, pos: torch.Tensor,
                             slot: torch.Tensor,
                             num_heads: int) -> torch.Tensor:
    """Fused rope + page append for a packed prefill: qkv
    [T, (Hq+2*Hkv)*D] is the wqkv output of T tokens, token t at logical
    position ``pos[t]``. Returns the roped q [T, Hq, D] (contiguous) and
    writes the roped k and the raw v of token t to physical pool row
    ``slot[t]`` (= page * P + pos % P). cos/sin are the FULL f32 [S, D/2]
    tables; ``pos`` and ``slot`` are int32 [T], computed once per forward
    pass. Bit-identical to ``rope`` + ``PagedKVCache.store_rows``."""
    T = qkv.shape[0]
    Hkv, D = kpool.shape[2], kpool.shape[3]
    if _on_gpu(qkv):
        return hip_ops().paged_prefill_rope_cache(
            qkv.contiguous(), kpool, vpool, cos, sin, pos.contiguous(),
            slot.contiguous())
    q, k, v = qkv.split([num_heads * D, Hkv * D, Hkv * D], dim=-1)
    p = pos.long()
    # rope takes [B, S, H, D] with cos/sin [S, D/2]: one batch of T rows
    cs, sn = cos[p], sin[p]
    q = rope(q.reshape(1, T, num_heads, D).contiguous(), cs, sn)[0]
    k = rope(k.reshape(1, T, Hkv, D).contiguous(), cs, sn)[0]
    kpool.view(-1, Hkv, D).index_copy_(0, slot.long(), k)
    vpool.view(-1, Hkv, D).index_copy_(0, slot.long(),
                                       v.reshape(T, Hkv, D).contiguous())
    return q.contiguous()


def paged_decode_rope_cache(qkv: torch.Tensor, kpool: torch.Tensor,
                            vpool: torch.Tensor, block_table: torch.Tensor,
                            cos: torch.Tensor, sin: torch.Tensor,
                            pos: torch.Tensor,
                            num_heads: int) -> torch.Tensor:
    """Fused decode rope + paged cache append: qkv [B, (Hq+2*Hkv)*D] for
    one position -> roped q [B, Hq, D]; the roped k and raw v of sequence
    b land in pool slot ``block_table[b, pos[b] // P] * P + pos[b] % P``.
    cos/sin are the FULL f32 [S, D/2] tables; ``pos`` is int32 [B]."""
    B = qkv.shape[0]
    P, Hkv, D = kpool.shape[1], kpool.shape[2], kpool.shape[3]
    if _on_gpu(qkv):
        return hip_ops().paged_decode_rope_cache(
            qkv.contiguous(), kpool, vpool, block_table, cos, sin,
            pos.contiguous())
    q, k, v = qkv.split([num_heads * D, Hkv * D, Hkv * D], dim=-1)
    q = q.reshape(B, 1, num_heads, D)
    k = k.reshape(B, 1, Hkv, D)
    v = v.reshape(B, 1, Hkv, D)
    outs = []
    for b in range(B):
        p = int(pos[b].item())
        page = int(block_table[b, p // P].item())
        cs, sn = cos[p:p + 1], sin[p:p + 1]
        outs.append(rope(q[b:b + 1].contiguous(), cs, sn))
        kpool[page, p % P] = rope(k[b:b + 1].contiguous(), cs, sn)[0, 0]
        vpool[page, p % P] = v[b, 0]
    return torch.cat(outs, dim=0).reshape(B, num_heads, D)


# ---------------------------------------------------------------------------
# Paged fp8 KV cache: the block-table forms of the three fp8 KV ops —
# ops/csrc/paged_attn_fp8kv.hip. k8pool / v8pool [num_pages, P, Hkv, 128]
# float8_e4m3fn, kspool / vspool [num_pages, P, Hkv] fp32; block_table and
# pos as for the bf16 pools. The CPU paths gather the logical cache and run
# the dense fp8 ops' CPU paths.
# ---------------------------------------------------------------------------


def _paged_gather_fp8kv(k8pool, v8pool, kspool, vspool, table_row, n: int):
    """The first ``n`` logical rows of one sequence as a dense fp8 cache
    (k8, v8, ks, vs) of batch 1. The bytes are gathered as uint8."""
    k8, v8 = (reference.paged_gather(p.view(torch.uint8), table_row, n)
              .view(torch.float8_e4m3fn) for p in (k8pool, v8pool))
    return (k8, v8, reference.paged_gather(kspool, table_row, n),
            reference.paged_gather(vspool, table_row, n))


def paged_decode_attention_fp8kv(q: torch.Tensor, k8pool: torch.Tensor,
                                 v8pool: torch.Tensor, kspool: torch.Tensor,
                                 vspool: torch.Tensor,
                                 block_table: torch.Tensor, pos: torch.Tensor,
                                 scale: Optional[float] = None,
                                 split: Optional[int] = None,
                                 rows_hint: Optional[int] = None
                                 ) -> torch.Tensor:
    """``decode_attention_fp8kv`` over paged fp8 pools: q [B, Hq, 128];
    sequence b attends its ``pos[b] + 1`` logical rows, row t read from
    ``pool[block_table[b, t // P], t % P]`` -> o [B, Hq, 128]. ``pos`` is
    int32 [B]. On the GPU, for the same split count the result is
    bit-identical to ``decode_attention_fp8kv`` on the same logical cache.
    ``split`` forces the number of length slices (1 = single pass). By
    default the launcher sizes it for ``rows_hint`` rows, a host bound on
    the rows any sequence attends (``PagedBatcher`` passes its host mirror
    of ``pos``); without a hint it assumes the table's capacity M * P."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if _on_gpu(q):
        return hip_ops().paged_decode_attn_fp8kv(
            q.contiguous(), k8pool, v8pool, kspool, vspool, block_table,
            pos.contiguous(), scale, int(split or 0), int(rows_hint or 0))
    outs = []
    for b in range(q.shape[0]):
        n = int(pos[b].item()) + 1
        outs.append(decode_attention_fp8kv(
            q[b:b + 1], *_paged_gather_fp8kv(k8pool, v8pool, kspool, vspool,
                                             block_table[b], n), n, scale))
    return torch.cat(outs, dim=0)


def paged_decode_rope_cache_fp8kv(qkv: torch.Tensor, k8pool: torch.Tensor,
                                  v8pool: torch.Tensor, kspool: torch.Tensor,
                                  vspool: torch.Tensor,
                                  block_table: torch.Tensor,
                                  cos: torch.Tensor, sin: torch.Tensor,
                                  pos: torch.Tensor,
                                  num_heads: int) -> torch.Tensor:
    """``decode_rope_cache_fp8kv`` through the table: qkv
    [B, (Hq+2*Hkv)*128] for one position -> roped q [B, Hq, 128]; the
    roped, bf16-rounded k and the raw v of sequence b are quantised
    (``quantize_kv_rows``) into pool slot
    ``block_table[b, pos[b] // P] * P + pos[b] % P``. cos/sin are the FULL
    f32 [S, 64] tables; ``pos`` is int32 [B]."""
    if _on_gpu(qkv):
        return hip_ops().paged_decode_rope_cache_fp8kv(
            qkv.contiguous(), k8pool, v8pool, kspool, vspool, block_table,
            cos, sin, pos.contiguous())
    # CPU: the dense op into a one-row scratch cache, then the page slot
    B = qkv.shape[0]
    P, Hkv, D = k8pool.shape[1:]
    k8 = torch.zeros(B, 1, Hkv, D, dtype=torch.float8_e4m3fn)
    v8 = torch.zeros_like(k8)
    ks = torch.ones(B, 1, Hkv)
    vs = torch.ones(B, 1, Hkv)
    outs = []
    for b in range(B):
        p = int(pos[b].item())
        outs.append(decode_rope_cache_fp8kv(
            qkv[b:b + 1], k8[b:b + 1], v8[b:b + 1], ks[b:b + 1], vs[b:b + 1],
            cos[p:p + 1], sin[p:p + 1], 0, num_heads))
        page = int(block_table[b, p // P].item())
        k8pool[page, p % P], kspool[page, p % P] = k8[b, 0], ks[b, 0]
        v8pool[page, p % P], vspool[page, p % P] = v8[b, 0], vs[b, 0]
    return torch.cat(outs, dim=0)


def paged_kv_quantize_store(k: torch.Tensor, v: torch.Tensor,
                            k8pool: torch.Tensor, v8pool: torch.Tensor,
                            kspool: torch.Tensor, vspool: torch.Tensor,
                            table_rows: torch.Tensor, start: int) -> None:
    """``kv_quantize_store`` into pages: k, v [B, S, Hkv, 128] bf16 (k
    already roped) become the logical rows ``start .. start+S-1`` of the
    sequences whose block-table rows are ``table_rows`` int32 [B, M], K and
    V in one launch."""
    B, S = k.shape[:2]
    P = k8pool.shape[1]
    assert table_rows.shape[0] == B, "one table row per sequence"
    assert 0 <= start and start + S <= table_rows.shape[1] * P, \
        "rows outside the table"
    if _on_gpu(k, k8pool):
        hip_ops().paged_kv_quantize_store(
            k.contiguous(), v.contiguous(), k8pool, v8pool, kspool, vspool,
            table_rows.contiguous(), int(start))
        return
    t = torch.arange(start, start + S)
    for x, pool8, pools in ((k, k8pool, kspool), (v, v8pool, vspool)):
        x8, xs = quantize_kv_rows(x)
        for b in range(B):
            pages = table_rows[b, t // P].long()
            pool8.view(torch.uint8)[pages, t % P] = x8[b].view(torch.uint8)
            pools[pages, t % P] = xs[b]


def paged_prefill_attention_fp8kv(q: torch.Tensor, k8pool: torch.Tensor,
                                  v8pool: torch.Tensor, kspool: torch.Tensor,
                                  vspool: torch.Tensor,
                                  block_table: torch.Tensor,
                                  ctx: torch.Tensor,
                                  scale: Optional[float] = None
                                  ) -> torch.Tensor:
    """``paged_prefill_attention`` over paged fp8 pools: q [B, S, Hq, 128]
    holds the rows at positions ``ctx[b] ..`` of sequence b, whose
    ``ctx[b] + S`` quantised rows (the chunk's own included) the pools
    already hold -> o [B, S, Hq, 128]. On the GPU the e4m3 bytes reach the
    bf16 MFMA unscaled (exact) and the row scales are applied in fp32, to
    the score and to P; the error against fp64 attention over the
    dequantised rows is bounded by ``bounds.prefill_fp8kv_ref_bound``."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if _on_gpu(q):
        return hip_ops().paged_prefill_attn_fp8kv(
            q.contiguous(), k8pool, v8pool, kspool, vspool, block_table,
            ctx.contiguous(), scale)
    S = q.shape[1]
    outs = []
    for b in range(q.shape[0]):
        c = int(ctx[b].item())
        k8, v8, ks, vs = _paged_gather_fp8kv(k8pool, v8pool, kspool, vspool,
                                             block_table[b], c + S)
        outs.append(reference.attention_prefix(
            q[b:b + 1], dequantize_kv(k8, ks), dequantize_kv(v8, vs), c,
            scale))
    return torch.cat(outs, dim=0)


def paged_prefill_attention_ragged_fp8kv(q: torch.Tensor,
                                         k8pool: torch.Tensor,
                                         v8pool: torch.Tensor,
                                         kspool: torch.Tensor,
                                         vspool: torch.Tensor,
                                         block_table: torch.Tensor, q_lens,
                                         ctx: torch.Tensor,
                                         scale: Optional[float] = None,
                                         plan: Optional[RaggedPlan] = None
                                         ) -> torch.Tensor:
    """``paged_prefill_attention_ragged`` over paged fp8 pools: q
    [T, Hq, 128] packed, the same ``q_lens`` / ``ctx`` / ``RaggedPlan``
    contract. On the GPU sequence b's rows are bit-identical to
    ``paged_prefill_attention_fp8kv`` on that sequence alone, at every
    ctx."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if plan is None:
        plan = RaggedPlan(q_lens, q.device)
    assert plan.q_lens == [int(n) for n in q_lens], "plan of other lengths"
    assert q.dim() == 3 and q.shape[0] == plan.T, (q.shape, plan.T)
    assert block_table.shape[0] == len(plan.q_lens) == ctx.numel()
    if _on_gpu(q):
        return hip_ops().paged_prefill_attn_ragged_fp8kv(
            q.contiguous(), k8pool, v8pool, kspool, vspool,
            block_table.contiguous(), ctx.contiguous(), plan.tiles, scale)
    return torch.cat([
        paged_prefill_attention_fp8kv(
            q[plan.cu[b]:plan.cu[b] + n][None], k8pool, v8pool, kspool,
            vspool, block_table[b:b + 1], ctx[b:b + 1], scale)[0]
        for b, n in enumerate(plan.q_lens)], dim=0)


def paged_prefill_rope_cache_fp8kv(qkv: torch.Tensor, k8pool: torch.Tensor,
                                   v8pool: torch.Tensor, kspool: torch.Tensor,
                                   vspool: torch.Tensor, cos: torch.Tensor,
                                   sin: torch.Tensor, pos: torch.Tensor,
                                   slot: torch.Tensor,
                                   num_heads: int) -> torch.Tensor:
    """``paged_prefill_rope_cache`` over paged fp8 pools: the same roped q
    [T, Hq, 128], bit for bit; the roped, bf16-rounded k and the raw v of
    token t are quantised (``quantize_kv_rows``) into pool row ``slot[t]``
    with their scales."""
    if _on_gpu(qkv):
        return hip_ops().paged_prefill_rope_cache_fp8kv(
            qkv.contiguous(), k8pool, v8pool, kspool, vspool, cos, sin,
            pos.contiguous(), slot.contiguous())
    # CPU: the bf16 op into one scratch row per token, then the pool rows
    T = qkv.shape[0]
    Hkv, D = k8pool.shape[2], k8pool.shape[3]
    kc = torch.zeros(T, 1, Hkv, D, dtype=qkv.dtype)
    vc = torch.zeros_like(kc)
    q = paged_prefill_rope_cache(qkv, kc, vc, cos, sin, pos,
                                 torch.arange(T, dtype=torch.int32),
                                 num_heads)
    rows = slot.long()
    for x, pool8, pools in ((kc, k8pool, kspool), (vc, v8pool, vspool)):
        x8, xs = quantize_kv_rows(x[:, 0])
        pool8.view(torch.uint8).view(-1, Hkv, D)[rows] = x8.view(torch.uint8)
        pools.view(-1, Hkv)[rows] = xs
    return q


def decode_linear(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """Skinny-M linear for the decode path: x [..., M, K] with M <= 8
    total rows -> x @ w.T via the W-stream-bound ``gemv_bf16`` kernel
    (ops/csrc/gemv.hip). hipBLASLt's tile kernels reach only ~1/3 of the
    HBM roof at decode batch sizes; this kernel reads each weight byte
    exactly once. Falls back to torch.matmul off-GPU or when the shape
    doesn't qualify (M > 8 or K % 512 != 0). Inference only (no autograd).

    An ``Fp8Weight`` runs on the W8A16 kernels for M <= 32 total rows and
    K % 1024 == 0, any N: the dot2 GEMV (ops/csrc/gemv_fp8.hip) up to
    ``FP8W_DOT2_MAX_M`` rows, the MFMA GEMM (ops/csrc/gemm_fp8w_mfma.hip)
    above. Other shapes dequantise and take the reference path.
    """
    x2 = x.reshape(-1, x.shape[-1])
    M, K = x2.shape
    if isinstance(w, Fp8Weight):
        if _fp8w_kernel_ok(x2, w):
            fn = hip_ops().gemv_fp8w if M <= FP8W_DOT2_MAX_M \
                else hip_ops().gemm_fp8w_mfma
            out = fn(x2.contiguous(), w.w8, w.scale)
        else:
            out = reference.decode_linear_fp8w(x2, w.dequant())
        return out.reshape(*x.shape[:-1], w.shape[0])
    # N > 32k (lm_head-sized): hipBLASLt's split-K kernels stream W
    # slightly faster there (5.8 vs 5.0 TB/s measured) — route to matmul
    if _on_gpu(x) and M <= 8 and K % 512 == 0 and w.shape[0] <= 32768 \
            and w.dtype == torch.bfloat16 and w.is_contiguous():
        out = hip_ops().gemv_bf16(x2.contiguous(), w)
    else:
        out = x2 @ w.t()
    return out.reshape(*x.shape[:-1], w.shape[0])


# ---------------------------------------------------------------------------
# MoE decode MLP (serving): top-k expert FFNs of a decode micro-batch —
# ops/csrc/moe_gemv.hip. The grouped kernels read the routing from device
# memory, so the fused path is two dispatches and never waits for the
# device; its result is bit-identical to the per-expert loop.
# ---------------------------------------------------------------------------

_MOE_DECODE_IMPLS = ("fused", "loop")
_moe_decode_impl = os.environ.get("TORCHX_AMD_MOE_DECODE", "fused")
assert _moe_decode_impl in _MOE_DECODE_IMPLS, (
    f"TORCHX_AMD_MOE_DECODE must be one of {_MOE_DECODE_IMPLS}")


def set_moe_decode_impl(impl: str) -> None:
    """Select the GPU path of ``moe_decode_mlp``: "fused" (default; the two
    grouped expert GEMV kernels, routing read on the device) or "loop" (one
    host sync, then the per-expert GEMV loop). Both produce the same bits.
    The initial value comes from TORCHX_AMD_MOE_DECODE."""
    global _moe_decode_impl
    if impl not in _MOE_DECODE_IMPLS:
        raise ValueError(f"moe decode impl must be 'fused' or 'loop', "
                         f"got {impl!r}")
    _moe_decode_impl = impl


def get_moe_decode_impl() -> str:
    return _moe_decode_impl


def moe_decode_mlp_loop(x: torch.Tensor, idx: torch.Tensor, cw: torch.Tensor,
                        wgu: Sequence[torch.Tensor],
                        wdown: Sequence[torch.Tensor]) -> torch.Tensor:
    """The per-expert loop of ``moe_decode_mlp``: one host sync for the
    routing, then every active expert runs the skinny-M GEMV + fused SwiGLU
    path on its tokens and is folded into ``out`` in ascending order."""
    idx_h = idx.cpu()  # ONE host sync; partitioning is host-side
    out = torch.zeros_like(x)
    for e in range(len(wgu)):
        rows_h = (idx_h == e).any(-1).nonzero(as_tuple=True)[0]
        if rows_h.numel() == 0:
            continue
        rows = rows_h.to(x.device, non_blocking=True)
        h = decode_linear_swiglu(x[rows], wgu[e])
        ye = decode_linear(h, wdown[e])
        coef = (cw * (idx == e)).sum(-1)[rows]            # [n], on device
        out[rows] += ye * coef[:, None]
    return out


def _moe_fused_ok(x, idx, cw, wgu, wdown) -> bool:
    if not (x.is_cuda and x.dim() == 2 and x.dtype == torch.bfloat16):
        return False
    B, H = x.shape
    E = len(wgu)
    if not (1 <= B <= 8 and 1 <= E <= 16 and len(wdown) == E):
        return False
    if idx.dtype != torch.int64 or idx.dim() != 2 or idx.shape[0] != B \
            or not 1 <= idx.shape[1] <= min(8, E) \
            or cw.shape != idx.shape or cw.dtype != torch.bfloat16:
        return False
    # all-bf16 or all-Fp8Weight experts; a mixed list takes the loop
    fp8 = isinstance(wgu[0], Fp8Weight)
    if any(isinstance(w, Fp8Weight) != fp8 for w in (*wgu, *wdown)):
        return False
    two_i = wgu[0].shape[0]
    I = two_i // 2
    tile = 1024 if fp8 else 512
    if two_i % 2 or H % tile or I % tile or H == 0 or I == 0 \
            or two_i * H >= 2 ** 31:
        return False
    if fp8:  # Fp8Weight keeps w8 and scale contiguous, e4m3 and fp32
        if not all(w.w8.device == x.device and w.scale.device == x.device
                   for w in (*wgu, *wdown)):
            return False
    elif not all(w.dtype == torch.bfloat16 and w.is_contiguous()
                 and w.device == x.device for w in (*wgu, *wdown)):
        return False
    return all(w.shape == (two_i, H) for w in wgu) \
        and all(w.shape == (H, I) for w in wdown)


def moe_decode_mlp(x: torch.Tensor, idx: torch.Tensor, cw: torch.Tensor,
                   wgu: Sequence[torch.Tensor],
                   wdown: Sequence[torch.Tensor]) -> torch.Tensor:
    """Top-k MoE MLP of a decode micro-batch: x [B, H] bf16, ``idx`` [B, k]
    int64 and ``cw`` [B, k] bf16 as ``torch.topk`` / ``softmax`` return them
    (the experts of a row distinct), ``wgu`` / ``wdown`` the E experts'
    packed gate|up [2I, H] and down [H, I] weights (separate tensors, never
    stacked) -> ``out[b] = sum_j cw[b, j] * down_e(swiglu(wgu_e x[b]))``,
    e = idx[b, j], [B, H] bf16. Inference only. The experts may also all
    be ``Fp8Weight``s (W8A16, ops/csrc/moe_gemv_fp8.hip).

    On the GPU with B <= 8, k <= 8, E <= 16 and H, I multiples of 512
    (1024 for ``Fp8Weight`` experts) this is two dispatches
    (``moe_gemv_swiglu``, ``moe_gemv_down_combine`` or their ``_fp8w``
    forms) and no host sync; everything else (CPU, larger batches, other
    shapes, lists that mix bf16 and fp8 experts, or
    ``set_moe_decode_impl("loop")``) runs ``moe_decode_mlp_loop``. The
    kernels reproduce its bits; with ``Fp8Weight`` experts they do so
    where the loop runs the dot2 GEMVs (groups of up to
    ``FP8W_DOT2_MAX_M`` tokens), and differ in the last bits from the
    MFMA kernels it takes above."""
    if _moe_decode_impl == "fused" and _moe_fused_ok(x, idx, cw, wgu, wdown):
        hip = hip_ops()
        x, idx, cw = x.contiguous(), idx.contiguous(), cw.contiguous()
        if isinstance(wgu[0], Fp8Weight):
            h = hip.moe_gemv_swiglu_fp8w(x, idx, [w.w8 for w in wgu],
                                         [w.scale for w in wgu])
            return hip.moe_gemv_down_combine_fp8w(
                h, idx, cw, [w.w8 for w in wdown], [w.scale for w in wdown])
        h = hip.moe_gemv_swiglu(x, idx, list(wgu))
        return hip.moe_gemv_down_combine(h, idx, cw, list(wdown))
    return moe_decode_mlp_loop(x, idx, cw, wgu, wdown)


# ---------------------------------------------------------------------------
# MoE decode router (serving): gate GEMV + top-k + softmax in one kernel,
# alone or behind the residual add + RMSNorm that feeds it —
# ops/csrc/moe_route.hip. fp32 logits, ties to the lower expert index, a
# row's result independent of the batch it is in.
# ---------------------------------------------------------------------------

_MOE_ROUTER_IMPLS = ("torch", "fused")
_moe_router_impl = os.environ.get("TORCHX_AMD_MOE_ROUTER", "torch")
assert _moe_router_impl in _MOE_ROUTER_IMPLS, (
    f"TORCHX_AMD_MOE_ROUTER must be one of {_MOE_ROUTER_IMPLS}")


def set_moe_router_impl(impl: str) -> None:
    """Select the routing of the Mixtral decode step: "torch" (default; the
    router matmul, ``torch.topk`` and ``softmax`` on bf16-rounded logits)
    or "fused" (``rmsnorm_res_route``: one kernel for norm and routing,
    fp32 logits). The two can pick different experts at a near-tie. The
    initial value comes from TORCHX_AMD_MOE_ROUTER."""
    global _moe_router_impl
    if impl not in _MOE_ROUTER_IMPLS:
        raise ValueError(f"moe router impl must be 'torch' or 'fused', "
                         f"got {impl!r}")
    _moe_router_impl = impl


def get_moe_router_impl() -> str:
    return _moe_router_impl


def _moe_route_ok(y: torch.Tensor, wr: torch.Tensor, k: int) -> bool:
    if not (y.is_cuda and y.dim() == 2 and y.dtype == torch.bfloat16
            and wr.dim() == 2 and wr.dtype == torch.bfloat16
            and wr.device == y.device and wr.is_contiguous()):
        return False
    B, H = y.shape
    E = wr.shape[0]
    return B >= 1 and wr.shape[1] == H and H % 2048 == 0 \
        and 2048 <= H <= 8192 and 1 <= E <= 16 and 1 <= k <= min(8, E)


def moe_route(y: torch.Tensor, wr: torch.Tensor, k: int):
    """Top-k routing of a decode micro-batch: y [B, H] bf16 (normed
    activations), router weight ``wr`` [E, H] bf16 -> ``(idx, cw)``, [B, k]
    int64 and bf16, the layout ``moe_decode_mlp`` reads: the k largest fp32
    logits in descending order, ties to the lower expert index, and their
    softmax. One dispatch on the GPU for H a multiple of 2048 up to 8192,
    E <= 16 and k <= min(8, E); the CPU and every other shape run
    ``reference.moe_route``, which defines the result."""
    if _moe_route_ok(y, wr, k):
        idx, cw = hip_ops().moe_route(y.contiguous(), wr, k)
        return idx, cw
    return reference.moe_route(y, wr, k)


def rmsnorm_res_route(x: torch.Tensor, res: Optional[torch.Tensor],
                      w: torch.Tensor, eps: float, wr: torch.Tensor, k: int):
    """``rmsnorm_res`` and ``moe_route`` on its output in one dispatch:
    returns ``(s, y, idx, cw)``. ``s`` and ``y`` are the bits of
    ``rmsnorm_res``; the normed row goes from the norm to the router dot
    products in registers. Inference only."""
    if _moe_route_ok(x, wr, k):
        s, y, idx, cw = hip_ops().rmsnorm_res_route(
            x.contiguous(), res.contiguous() if res is not None else None,
            w.contiguous(), eps, wr, k)
        return s, y, idx, cw
    s, y = rmsnorm_res(x, res, w, eps)
    return (s, y, *reference.moe_route(y, wr, k))
