"""fp64 references, per-element error bounds, input families, case lists and
plain torch emulations for the kernels of the training step: RMSNorm (fwd,
dx, dw, the residual forms), RoPE (flat and packed qkv), SwiGLU (flat,
packed, transposing), cross entropy, AdamW, the fp8 cast+transpose and the
bf16 transpose.

Pure torch, CPU or GPU tensors, no dependency on the HIP extension; laid out
like ``bounds.py``, whose ``U``, ``E32``, ``bound_ratio`` (with its +1e-30)
and ``case_seed`` are reused.

Notation (references and bounds are fp64, computed from the values the
kernel holds: bf16 inputs, fp32 tables and constants; ``|.|`` elementwise):

  u    = 2^-8    bf16 round-to-nearest-even unit roundoff (f32_to_bf16)
  f    = 2^-24   one fp32 operation (add, multiply, fma, sqrtf, division)
  e32  = 2^-16   the one cover used for every approximate intrinsic
                 (v_exp_f32 through __expf / __builtin_amdgcn_exp2f,
                 rsqrtf, __logf), relative to its result
  tiny = 2^-126  smallest normal fp32: results below it may be flushed
  sub  = 2^-133  spacing of the bf16 subnormals

Every bound is first order in these; the fp32 terms are multiplied by
(1 + u) because the output rounding acts on the computed value, not on the
exact one.  No constant is fitted to a kernel's output: each is a count of
rounding points read off the kernel source and named in the docstring of
the function that uses it.
"""

from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import torch

from .bounds import E32, U, bound_ratio, case_seed, global_rel_err  # noqa: F401

F = 2.0 ** -24
TINY = 2.0 ** -126
SUB = 2.0 ** -133
FLT_MAX = 3.4028234663852886e38
LOG2E_F32 = 1.44269504          # the literal of the SwiGLU kernels
CE_NEG = -3.4e38                # running max of a CE thread that saw nothing

FAMILIES = ("flat", "edges")

_BF = torch.bfloat16
_F32 = torch.float32
_F64 = torch.float64


def _f32(x: float) -> float:
    """The fp32 value a ``(float)x`` cast in the binding holds."""
    return torch.tensor(x, dtype=_F32).item()


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def _fma32(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """fmaf on fp32 tensors: the product is exact in fp64, one rounding."""
    return (a.double() * b.double() + c.double()).float()


# ---------------------------------------------------------------------------
# RMSNorm
# ---------------------------------------------------------------------------

# relative error of invrms: the sum of squares is a chain of 8 * ITERS <= 32
# fmas per thread, 6 wave-reduction adds and 3 LDS adds (41 roundings on a
# sum of non-negative terms: no cancellation), then total / H and + eps (2
# more); rsqrt halves the relative error of its argument (43 f / 2 < 22 f)
# and adds its own cover
REL_INVRMS = 22 * F + E32


def rmsnorm_fwd_ref_bound(x: torch.Tensor, w: torch.Tensor,
                          eps: float) -> Dict[str, torch.Tensor]:
    """x [rows, H], w [H] bf16 -> fp64 ``y`` [rows, H], ``invrms`` [rows] and
    ``y_bound``, ``invrms_bound`` (rmsnorm_fwd_kernel, rmsnorm_res_fwd_kernel).

      invrms: REL_INVRMS |r64|                       (see REL_INVRMS)
      y:      (u + (REL_INVRMS + 2 f)(1 + u)) |y64|  y = bf16((x * r) * w):
              two fp32 products and the output rounding.

    ``eps`` enters as the fp32 value the binding passes.  A row whose sum of
    squares is beyond the fp32 range is pinned to what the kernel's fp32 sum
    gives: total = inf, r = rsqrtf(inf) = 0, y = x * 0 * w = 0 exactly (the
    fp64 value of such a row would be finite; the kernel's overflow is its
    documented behaviour, not an error to bound).  ``add_rmsnorm`` and
    ``rmsnorm_res`` are this reference applied to s = bf16(x + delta), which
    the caller forms (and checks with torch.equal)."""
    xf, wf = x.double(), w.double()
    H = x.shape[-1]
    sumsq = (xf * xf).sum(-1)
    r = torch.rsqrt(sumsq / H + _f32(eps))
    r = torch.where(sumsq > FLT_MAX, torch.zeros_like(r), r)
    y = xf * r[..., None] * wf
    return {
        "invrms": r, "invrms_bound": REL_INVRMS * r.abs(),
        "y": y, "y_bound": (U + (REL_INVRMS + 2 * F) * (1 + U)) * y.abs(),
    }


def rmsnorm_dx_ref_bound(dy: torch.Tensor, x: torch.Tensor, w: torch.Tensor,
                         invrms: torch.Tensor,
                         dres: Optional[torch.Tensor] = None
                         ) -> Dict[str, torch.Tensor]:
    """fp64 ``dx`` [rows, H] of rmsnorm_bwd_dx_kernel's own inputs, the
    ``invrms`` (r, fp32) the forward kernel saved included, and ``dx_bound``.

      dx64 = dy w r - x (r^3 / H) ts,   ts = sum_j dy_j w_j x_j,
      A    = sum_j |dy_j w_j x_j|.

    dy * w is exact in fp32 (two 8-bit significands).  ts is the same
    32 + 6 + 3 chain as the forward sum, but it cancels: |ts - ts64| <=
    41 f A.  kk = ts r r r / H is 4 more roundings, |kk - kk64| <= 45 f
    (r^3 / H) A.  The output is bf16(fma(dyw, r, -(x kk))): one rounding on
    x kk, one on the fma, each at most f (|dy w| r + |x| (r^3 / H) A).  So

      e1 = u |dx64| + (1 + u) f (|dy w| r + 47 |x| (r^3 / H) A).

    With ``dres`` the kernel rounds twice, bf16(bf16(dx) + dres): the
    reference is dx64 + dres and the bound e1 + u (|dx64 + dres| + e1)."""
    dyf, xf, wf = dy.double(), x.double(), w.double()
    r = invrms.double()[..., None]
    H = x.shape[-1]
    dyw = dyf * wf
    ts = (dyw * xf).sum(-1, keepdim=True)
    a = (dyw * xf).abs().sum(-1, keepdim=True)
    dx = dyw * r - xf * (r ** 3 / H) * ts
    e1 = U * dx.abs() + (1 + U) * F * (
        dyw.abs() * r + 47 * xf.abs() * (r ** 3 / H) * a)
    if dres is None:
        return {"dx": dx, "dx_bound": e1}
    out = dx + dres.double()
    return {"dx": out, "dx_bound": e1 + U * (out.abs() + e1)}


def rmsnorm_dw_ref_bound(dy: torch.Tensor, x: torch.Tensor,
                         invrms: torch.Tensor) -> Dict[str, torch.Tensor]:
    """fp64 ``dw`` [H] = sum_rows dy x r and ``dw_bound``: each of the
    ``rows`` adds / fmas of the chunked column reduction rounds by at most f
    relative to a running sum bounded by sum |terms|, doubled for the
    product rounding: rows * 2^-23 * sum_rows |dy x r|."""
    rows = x.shape[0]
    terms = dy.double() * x.double() * invrms.double()[:, None]
    return {"dw": terms.sum(0),
            "dw_bound": rows * 2.0 ** -23 * terms.abs().sum(0)}


def rmsnorm_inputs(family: str, rows: int, H: int, seed: int):
    """bf16 (x, w, dy, other): ``other`` serves as the delta of add_rmsnorm
    and as the dres of its backward.  ``edges`` gives row i, by i % 4: all
    zero (r = 1 / sqrt(eps)); +-2^60 (the squares overflow fp32: pinned, see
    rmsnorm_fwd_ref_bound); 1e-3 randn with one element of 1e4; randn."""
    assert family in FAMILIES, family
    g = _gen(seed)
    x = torch.randn(rows, H, generator=g)
    w = torch.randn(H, generator=g)
    dy = torch.randn(rows, H, generator=g)
    other = torch.randn(rows, H, generator=g)
    if family == "edges":
        for i in range(rows):
            if i % 4 == 0:
                x[i] = 0.0
            elif i % 4 == 1:
                x[i] = torch.where(x[i] < 0, -1.0, 1.0) * 2.0 ** 60
            elif i % 4 == 2:
                x[i] *= 1e-3
                x[i, (7 * i + 5) % H] = 1e4
    return tuple(t.to(_BF) for t in (x, w, dy, other))


def emulate_rmsnorm_fwd(x, w, eps: float, fault: Optional[str] = None):
    """fp32 emulation of rmsnorm_fwd_kernel -> (y bf16, invrms f32).
    ``fault``: "no_eps" (eps left out), "mean_2048" (the sum of squares is
    divided by 2048, the one-iteration instance's width, instead of H)."""
    xf, wf = x.float(), w.float()
    H = 2048 if fault == "mean_2048" else x.shape[-1]
    total = (xf * xf).sum(-1)
    mean = total / H
    if fault != "no_eps":
        mean = mean + torch.tensor(eps, dtype=_F32)
    r = torch.rsqrt(mean)
    return (xf * r[..., None] * wf).to(_BF), r


def emulate_rmsnorm_dx(dy, x, w, invrms, dres=None,
                       fault: Optional[str] = None):
    """fp32 emulation of rmsnorm_bwd_dx_kernel -> dx bf16.  ``fault``:
    "kk_r2" (the x * kk term taken with r^2 instead of r^3),
    "dres_before_round" (dres added in fp32, one rounding instead of two)."""
    xf = x.float()
    dyw = dy.float() * w.float()
    r = invrms.float()[..., None]
    H = x.shape[-1]
    ts = (dyw * xf).sum(-1, keepdim=True)
    kk = ts * r * r / H if fault == "kk_r2" else ts * r * r * r / H
    d32 = _fma32(dyw, r, -(xf * kk))
    if dres is None:
        return d32.to(_BF)
    if fault == "dres_before_round":
        return (d32 + dres.float()).to(_BF)
    return (d32.to(_BF).float() + dres.float()).to(_BF)


def emulate_rmsnorm_dw(dy, x, invrms) -> torch.Tensor:
    """fp32 emulation of the two dw kernels (any summation order is within
    the bound) -> dw f32 [H]."""
    return ((dy.float() * x.float()) * invrms.float()[:, None]).sum(0)


# the four template instances x rows below, at and off one block
RMSNORM_CASES = [("r%d-H%d" % (r, H), r, H)
                 for H in (2048, 4096, 6144, 8192) for r in (1, 3, 65)]
RMSNORM_EPS = 1e-5


# ---------------------------------------------------------------------------
# RoPE
# ---------------------------------------------------------------------------


def rope_ref_bound(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
                   sign: float = 1.0) -> Dict[str, torch.Tensor]:
    """x [B, S, H, D] bf16, fp32 tables with at least S rows of D/2 ->
    fp64 ``y`` and ``y_bound``; position s uses table row s (``cos[:S]``),
    the table values taken as given.  sign = +1 forward, -1 backward.

      y1 = x1 c - sign s x2,  y2 = x2 c + sign s x1
      bound = (u + 3 f) (|x1 c| + |x2 s|)   resp. (|x2 c| + |x1 s|):

    the kernels compute fmaf(x1, c, -(sign s) x2): one rounding on the
    s x2 product, one on the fma, each at most f times the sum of the
    absolute terms, the third f for the (1 + u) of the output rounding.
    Serves rope_fwdbwd_kernel and, per head of the q and k regions,
    rope_qkv_kernel."""
    B, S, H, D = x.shape
    h = D // 2
    xf = x.double()
    x1, x2 = xf[..., :h], xf[..., h:]
    c = cos[:S].double().view(1, S, 1, h)
    s = sin[:S].double().view(1, S, 1, h)
    y = torch.cat([x1 * c - sign * s * x2, x2 * c + sign * s * x1], -1)
    a = torch.cat([(x1 * c).abs() + (x2 * s).abs(),
                   (x2 * c).abs() + (x1 * s).abs()], -1)
    return {"y": y, "y_bound": (U + 3 * F) * a}


def rope_qkv_ref_bound(qkv: torch.Tensor, cos, sin, Hq: int, Hkv: int,
                       sign: float = 1.0) -> Dict[str, torch.Tensor]:
    """qkv [B, S, (Hq + 2 Hkv) * 128]: ``rope_ref_bound`` on the Hq + Hkv
    heads of the q and k regions; the v region is the input itself under a
    zero bound (the tests also hold it to torch.equal)."""
    B, S, _ = qkv.shape
    nh = Hq + Hkv
    r = rope_ref_bound(qkv[..., :nh * 128].reshape(B, S, nh, 128), cos, sin,
                       sign)
    v = qkv[..., nh * 128:].double()
    return {"y": torch.cat([r["y"].reshape(B, S, nh * 128), v], -1),
            "y_bound": torch.cat([r["y_bound"].reshape(B, S, nh * 128),
                                  torch.zeros_like(v)], -1)}


def rope_inputs(B: int, S: int, H: int, D: int, table_rows: int, seed: int):
    """x bf16 [B, S, H, D] (randn) and fp32 tables of ``table_rows`` rows
    whose angles are drawn at random, so that no two rows agree."""
    g = _gen(seed)
    x = torch.randn(B, S, H, D, generator=g).to(_BF)
    ang = torch.rand(table_rows, D // 2, generator=g) * (2 * math.pi)
    return x, torch.cos(ang), torch.sin(ang)


def emulate_rope(x, cos, sin, sign: float = 1.0,
                 fault: Optional[str] = None) -> torch.Tensor:
    """fp32 emulation of rope_fwdbwd_kernel / rope_qkv_kernel on x
    [B, S, H, D] -> bf16.  ``fault``: "pos_mod_table" (the position of row
    (b, s) is (b S + s) modulo the table length instead of s: wrong for
    b >= 1 under a table longer than S), "sin_sign_second_half" (the sign of
    the sin term flipped in the second half only)."""
    B, S, H, D = x.shape
    h = D // 2
    pos = torch.arange(S)[None, :].expand(B, S)
    if fault == "pos_mod_table":
        pos = (torch.arange(B)[:, None] * S + pos) % cos.shape[0]
    c = cos[pos].view(B, S, 1, h)
    s = sin[pos].view(B, S, 1, h) * torch.tensor(sign, dtype=_F32)
    x1, x2 = x.float()[..., :h], x.float()[..., h:]
    s2 = -s if fault == "sin_sign_second_half" else s
    y1 = _fma32(x1, c.expand_as(x1), -(s * x2))
    y2 = _fma32(x2, c.expand_as(x2), s2 * x1)
    return torch.cat([y1, y2], -1).to(_BF)


# (id, B, S, H, D, table rows): D = 8 is one thread's 4 pairs; the last case
# is the first under a table longer than S
ROPE_CASES = [
    ("b2s5h3d128", 2, 5, 3, 128, 5),
    ("b1s1h1d8", 1, 1, 1, 8, 1),
    ("b3s4h2d64", 3, 4, 2, 64, 4),
    ("b2s5h3d128-table16", 2, 5, 3, 128, 16),
]
# (id, B, S, Hq, Hkv): nh * 16 = 96 threads of one block; 640 > 256, a
# second x block
ROPE_QKV_CASES = [("b2s5q4kv2", 2, 5, 4, 2), ("b1s3q32kv8", 1, 3, 32, 8)]


# ---------------------------------------------------------------------------
# SwiGLU
# ---------------------------------------------------------------------------


def _sigmoid_terms(g: torch.Tensor):
    """sig, 1 - sig (both without cancellation) and the relative error of
    the kernels' sig = 1 / (1 + exp2(-1.44269504f g)):

      the exponent argument is one fp32 product with a constant that is
      log2(e) rounded to fp32: relative 2 f, which the exponential turns
      into 2 f |g| relative; v_exp_f32 adds e32.  An error of the
      exponential reaches sig scaled by e / (1 + e) = 1 - sig.  1 + e is
      one rounding; the division is covered by 2 f.

      rel(sig) = (e32 + 2 f |g|) (1 - sig) + 3 f."""
    sig = torch.sigmoid(g)
    om = torch.sigmoid(-g)
    return sig, om, (E32 + 2 * F * g.abs()) * om + 3 * F


def swiglu_ref_bound(g: torch.Tensor, u: torch.Tensor
                     ) -> Dict[str, torch.Tensor]:
    """fp64 ``out`` = silu(g) u and ``out_bound`` for every SwiGLU forward
    kernel (flat, packed):

      (u + (rel(sig) + 2 f)(1 + u)) |out64|  +  |g u| tiny + sub.

    out = bf16((g * sig) * u): two fp32 products.  The absolute floor: for
    g < -88.7 exp2 overflows to inf and sig is exactly 0, and a sig below
    the fp32 normal range may be flushed, an absolute error of at most
    ``tiny`` on sig; a result in the bf16 subnormal range is rounded to
    their spacing ``sub``."""
    gf, uf = g.double(), u.double()
    sig, _, rs = _sigmoid_terms(gf)
    out = gf * sig * uf
    return {"out": out,
            "out_bound": (U + (rs + 2 * F) * (1 + U)) * out.abs()
            + (gf * uf).abs() * TINY + SUB}


def swiglu_bwd_ref_bound(dout: torch.Tensor, g: torch.Tensor,
                         u: torch.Tensor) -> Dict[str, torch.Tensor]:
    """fp64 ``dg``, ``du`` and their bounds for every SwiGLU backward kernel
    (flat, packed, transposing).

      du = dout (g sig):            (u + (rel(sig) + 2 f)(1 + u)) |du64|
      dg = dout u dsilu,  dsilu = sig (1 + g (1 - sig)).

    dsilu cancels near g = -1.28, so its error is taken in absolute terms
    (om = 1 - sig, rs = rel(sig)):

      1 - sig:         rs sig + f om
      g (1 - sig):     |g| (rs sig + f om) + f |g| om
      1 + g (1 - sig): the above + f (1 + |g| om)
      dsilu:           sig * the above + (rs + f) dabs,
                       dabs = sig (1 + |g| om)   (the absolute-value form)

    and dg = bf16((dout * u) * dsilu) adds 2 f dabs:

      u |dg64| + (1 + u) |dout u| (err(dsilu) + 2 f dabs).

    Floors as in ``swiglu_ref_bound``: |dout g| tiny + sub for du,
    |dout u| (1 + |g|) tiny + sub for dg."""
    dof, gf, uf = dout.double(), g.double(), u.double()
    sig, om, rs = _sigmoid_terms(gf)
    ga = gf.abs()
    du = dof * gf * sig
    du_bound = ((U + (rs + 2 * F) * (1 + U)) * du.abs()
                + (dof * gf).abs() * TINY + SUB)
    dsilu = sig * (1 + gf * om)
    dabs = sig * (1 + ga * om)
    e_om = rs * sig + F * om
    e_one = ga * e_om + F * ga * om + F * (1 + ga * om)
    e_ds = sig * e_one + (rs + F) * dabs
    dg = dof * uf * dsilu
    dou = (dof * uf).abs()
    dg_bound = (U * dg.abs() + (1 + U) * dou * (e_ds + 2 * F * dabs)
                + dou * (1 + ga) * TINY + SUB)
    return {"dg": dg, "dg_bound": dg_bound, "du": du, "du_bound": du_bound}


SWIGLU_EDGE_G = (0.0, 2.0 ** -100, -2.0 ** -100, -1.28, 20.0, -20.0, 88.0,
                 -88.0, 100.0, -100.0)
SWIGLU_SENTINEL = 12345.0      # bf16(12345) = 12352: no SwiGLU result here


def swiglu_inputs(family: str, n: int, seed: int):
    """bf16 (g, u, dout) of n elements.  ``edges``: g cycles through
    SWIGLU_EDGE_G (sigmoid 1/2, the smallest arguments, the zero of dsilu,
    saturation, the last finite exp2 and its overflow), u and dout randn."""
    assert family in FAMILIES, family
    gen = _gen(seed)
    g = torch.randn(n, generator=gen)
    u = torch.randn(n, generator=gen)
    dout = torch.randn(n, generator=gen)
    if family == "edges":
        g = torch.tensor(SWIGLU_EDGE_G, dtype=_F64)[torch.arange(n) % len(
            SWIGLU_EDGE_G)].float()
    return g.to(_BF), u.to(_BF), dout.to(_BF)


def swiglu_exp2_overflows(g: torch.Tensor) -> torch.Tensor:
    """Where the kernels' exp2 argument reaches 128 (the result is inf)."""
    return torch.tensor(-LOG2E_F32, dtype=_F32) * g.float() >= 128.0


def _sig32(g32: torch.Tensor) -> torch.Tensor:
    e = torch.exp2(torch.tensor(-LOG2E_F32, dtype=_F32) * g32)
    return 1.0 / (1.0 + e)


def emulate_swiglu(g, u, fault: Optional[str] = None) -> torch.Tensor:
    """fp32 emulation of the SwiGLU forward kernels on flat tensors -> bf16.
    ``fault``: "tail_sentinel" (the last n % 8 elements are never written
    and hold SWIGLU_SENTINEL)."""
    gf, uf = g.float(), u.float()
    out = (gf * _sig32(gf) * uf).to(_BF)
    if fault == "tail_sentinel":
        n8 = g.numel() // 8 * 8
        out.view(-1)[n8:] = SWIGLU_SENTINEL
    return out


def emulate_swiglu_bwd(dout, g, u, fault: Optional[str] = None):
    """fp32 emulation of the SwiGLU backward kernels -> (dg, du) bf16.
    ``fault``: "tail_sentinel" as above, "dsilu_no_g_term" (dsilu = sig,
    the g (1 - sig) term left out)."""
    dof, gf, uf = dout.float(), g.float(), u.float()
    sig = _sig32(gf)
    dsilu = sig if fault == "dsilu_no_g_term" else (
        sig * (1.0 + gf * (1.0 - sig)))
    dg = (dof * uf * dsilu).to(_BF)
    du = (dof * (gf * sig)).to(_BF)
    if fault == "tail_sentinel":
        n8 = g.numel() // 8 * 8
        dg.view(-1)[n8:] = SWIGLU_SENTINEL
        du.view(-1)[n8:] = SWIGLU_SENTINEL
    return dg, du


# flat: below, at and above one vector, a tail behind a full block of 256
# vectors, and a grid of more than one block without a tail
SWIGLU_FLAT_N = (1, 7, 8, 9, 2048 + 3, 256 * 8 * 3 + 8)
# packed (rows, I): one vector; two x blocks (257 vectors) over 3 rows; 65
# rows of 9 vectors
SWIGLU_PACKED_CASES = [(1, 8), (3, 2056), (65, 72)]
# transposing (rows, I): one tile, plus the shapes of test_wgrad_tn.py
SWIGLU_BWD_T_CASES = [(64, 64), (192, 64), (64, 4096), (33 * 64, 128)]


# ---------------------------------------------------------------------------
# cross entropy
# ---------------------------------------------------------------------------


def ce_chain(V: int) -> int:
    """Longest chain of online-softmax updates a partial sum of
    ce_fwd_kernel passes through: 8 per 2048-column sweep and one per
    256-column tail sweep in its thread, 6 wave butterflies, 3 LDS
    combines."""
    v8 = V // 8 * 8
    return 8 * ((v8 + 2047) // 2048) + (V - v8 + 255) // 256 + 9


def _ce_exp_cover(arg: torch.Tensor) -> torch.Tensor:
    """Relative error of __expf at ``arg``: e32 for v_exp_f32, f |arg| for
    the rounding of the argument's subtraction and f |arg| for the product
    with log2(e) inside __expf."""
    return E32 + 2 * F * arg.abs()


def ce_ref_bound(logits: torch.Tensor, targets: torch.Tensor
                 ) -> Dict[str, torch.Tensor]:
    """logits [T, V] bf16, targets [T] int64 -> fp64 ``lse``, ``loss`` [T]
    and ``lse_bound``, ``loss_bound`` (absolute, as for attention).

    Every term exp(x - M) of the sum S is non-negative and is multiplied
    ``ce_chain(V)`` times at most by a rescale factor exp(m - M); each such
    update is one __expf (arguments beyond 88 give an exact 0, so the cover
    is taken at 88: e32 + 176 f), one product and one add.  log S = lse - M
    carries the __logf cover, M + log S one rounding:

      lse:  ce_chain(V) (e32 + 178 f) + e32 |lse64 - max| + f |lse64|
      loss: lse_bound + f (|lse64| + |x_t|)        one fp32 subtraction.

    A target outside [0, V) has no loss: the kernel returns NaN there, and
    so does this reference (``loss_bound`` 0; compare with ``ce_loss_ok``)."""
    x = logits.double()
    T, V = x.shape
    lse = torch.logsumexp(x, -1)
    mx = x.amax(-1)
    lse_bound = (ce_chain(V) * (E32 + 178 * F) + E32 * (lse - mx).abs()
                 + F * lse.abs())
    valid = (targets >= 0) & (targets < V)
    xt = x.gather(1, targets.clamp(0, V - 1)[:, None])[:, 0]
    nan = torch.full_like(lse, float("nan"))
    loss = torch.where(valid, lse - xt, nan)
    loss_bound = torch.where(valid, lse_bound + F * (lse.abs() + xt.abs()),
                             torch.zeros_like(lse))
    return {"lse": lse, "lse_bound": lse_bound, "loss": loss,
            "loss_bound": loss_bound}


def ce_loss_ok(got: torch.Tensor, ref: Dict[str, torch.Tensor]
               ) -> Tuple[float, bool]:
    """``bound_ratio`` for the loss, with the rows of an out-of-range target
    held to the pinned NaN."""
    want_nan = torch.isnan(ref["loss"])
    g = got.double()
    if not bool((torch.isnan(g) == want_nan).all()):
        return float("inf"), False
    keep = ~want_nan
    if not bool(keep.any()):
        return 0.0, True
    return bound_ratio(g[keep], ref["loss"][keep], ref["loss_bound"][keep])


def ce_bwd_ref_bound(logits: torch.Tensor, targets: torch.Tensor,
                     lse: torch.Tensor, gscale: torch.Tensor
                     ) -> Dict[str, torch.Tensor]:
    """fp64 ``dlogits`` = gscale (exp(x - lse) - 1[t]) of ce_bwd_kernel's own
    inputs (the fp32 ``lse`` of the forward kernel included) and its bound

      u |d64| + (1 + u) e (p + 1[t]) |gscale| + tiny |gscale|,
      e = e32 + 2 f |x - lse| + 2 f:

    __expf at x - lse with both argument roundings (``_ce_exp_cover``), one
    subtraction and one product; p below the fp32 normal range may be
    flushed (``tiny``)."""
    x = logits.double()
    T, V = x.shape
    arg = x - lse.double()[:, None]
    p = torch.exp(arg)
    onehot = torch.zeros_like(x)
    valid = (targets >= 0) & (targets < V)
    onehot[valid, targets[valid]] = 1.0
    gs = gscale.double()[:, None]
    d = gs * (p - onehot)
    e = _ce_exp_cover(arg) + 2 * F
    return {"dlogits": d,
            "dlogits_bound": U * d.abs() + (1 + U) * e * (p + onehot) * gs.abs()
            + TINY * gs.abs()}


def ce_inputs(family: str, T: int, V: int, seed: int):
    """(logits bf16 [T, V], targets int64 [T], gscale f32 [T]).  ``edges``
    gives row i, by i % 5: the maximum (12) in the vector tail (column V8,
    or V - 1 where V % 8 == 0); in the last column; in column 0; all logits
    equal; logits of +-3e4.  The target is the argmax where there is one."""
    assert family in FAMILIES, family
    g = _gen(seed)
    x = torch.randn(T, V, generator=g)
    t = torch.randint(0, V, (T,), generator=g)
    gs = torch.randn(T, generator=g)
    if family == "edges":
        v8 = V // 8 * 8
        for i in range(T):
            k = i % 5
            if k <= 2:
                col = (v8 if v8 < V else V - 1, V - 1, 0)[k]
                x[i, col] = 12.0
                t[i] = col
            elif k == 3:
                x[i] = 0.75
            else:
                x[i] = torch.where(x[i] < 0, -3e4, 3e4)
    return x.to(_BF), t, gs


def ce_row_max_in_tail(logits: torch.Tensor) -> torch.Tensor:
    """bool [T]: the row's argmax lies in the scalar tail V8 .. V."""
    V = logits.shape[1]
    return logits.float().argmax(-1) >= V // 8 * 8


def _ce_combine(m, s, m2, s2):
    M = torch.maximum(m, m2)
    return M, s * torch.exp(m - M) + s2 * torch.exp(m2 - M)


def emulate_ce_fwd(logits, targets, fault: Optional[str] = None):
    """fp32 emulation of ce_fwd_kernel with its thread structure: 256
    threads, 8-column vectors in 2048-column sweeps, the scalar tail, the
    xor-butterfly wave reduction and the 4-way combine -> (loss, lse) f32.
    ``fault``: "lse_no_tail" (columns V8 .. V missing from the sum),
    "empty_s1" (a thread that saw no column enters the reduction as if it
    had seen one logit of 0: m = 0, s = 1 instead of m = -3.4e38, s = 0),
    "empty_s1_neg" (s = 1 at the kernel's m = -3.4e38: harmless, because
    exp(-3.4e38 - M) = 0)."""
    x = logits.float()
    T, V = x.shape
    v8 = V // 8 * 8
    tid = torch.arange(256)
    cols = []
    for base in range(0, v8, 2048):
        for j in range(8):
            cols.append(base + tid * 8 + j)
            cols[-1] = torch.where(cols[-1] < v8, cols[-1], -1)
    if fault != "lse_no_tail":
        for base in range(v8, V, 256):
            c = base + tid
            cols.append(torch.where(c < V, c, -1))
    m = torch.full((T, 256), CE_NEG, dtype=_F32)
    s = torch.zeros(T, 256, dtype=_F32)
    seen = torch.zeros(256, dtype=torch.bool)
    for c in cols:
        act = c >= 0
        f = x[:, c.clamp(min=0)]
        M = torch.maximum(m, f)
        s2 = s * torch.exp(m - M) + torch.exp(f - M)
        s = torch.where(act, s2, s)
        m = torch.where(act, M, m)
        seen |= act
    if fault == "empty_s1":
        m = torch.where(seen, m, torch.zeros_like(m))
        s = torch.where(seen, s, torch.ones_like(s))
    elif fault == "empty_s1_neg":
        s = torch.where(seen, s, torch.ones_like(s))
    m, s = m.view(T, 4, 64), s.view(T, 4, 64)
    lane = torch.arange(64)
    off = 32
    while off > 0:
        m, s = _ce_combine(m, s, m[..., lane ^ off], s[..., lane ^ off])
        off >>= 1
    M, S = m[:, 0, 0], s[:, 0, 0]
    for i in range(1, 4):
        M, S = _ce_combine(M, S, m[:, i, 0], s[:, i, 0])
    lse = M + torch.log(S)
    valid = (targets >= 0) & (targets < V)
    xt = x.gather(1, targets.clamp(0, V - 1)[:, None])[:, 0]
    loss = torch.where(valid, lse - xt, torch.full_like(lse, float("nan")))
    return loss, lse


def emulate_ce_bwd(logits, targets, lse, gscale,
                   fault: Optional[str] = None) -> torch.Tensor:
    """fp32 emulation of ce_bwd_kernel -> dlogits bf16.  ``fault``:
    "onehot_plus1" (the 1 subtracted at column target + 1)."""
    x = logits.float()
    T, V = x.shape
    p = torch.exp(x - lse.float()[:, None])
    t = targets + 1 if fault == "onehot_plus1" else targets
    valid = (t >= 0) & (t < V)
    p[valid, t[valid]] -= 1.0
    return (p * gscale.float()[:, None]).to(_BF)


# (T, V): one column; a row that is all tail; one vector; an odd row pitch
# (the 16-byte loads of odd rows start at 2-byte alignment) with a tail;
# exactly one sweep; a second sweep in which most threads see nothing, plus
# a tail
CE_CASES = [(1, 1), (3, 7), (2, 8), (5, 1003), (4, 2048), (3, 4099)]


# ---------------------------------------------------------------------------
# AdamW
# ---------------------------------------------------------------------------


def _adamw_consts(lr, beta1, beta2, eps, wd, step: int, fault=None):
    """The fp32 values adamw_kernel holds, as python floats: the casts of the
    binding, 1.f - beta in the kernel, bc = 1 - powf(beta, step) in fp32 and
    the launcher's 1 / bc1, 1 / sqrtf(bc2); plus ``cover``, the relative
    error this side's powf may have against the host's (one ulp, 2 f, of
    the power, relative to bc: 2 f pow / bc; halved by the square root)."""
    t = lambda v: torch.tensor(v, dtype=_F32)    # noqa: E731
    one = t(1.0)
    b1, b2 = t(beta1), t(beta2)
    p1, p2 = torch.pow(b1, t(float(step))), torch.pow(b2, t(float(step)))
    bc1, bc2 = one - p1, one - p2
    ibc1, isbc2 = one / bc1, one / torch.sqrt(bc2)
    if fault == "no_bias_correction":
        ibc1, isbc2 = one, one
    cover = 2 * F * (p1 / bc1).item() + F * (p2 / bc2).item()
    c = {"lr": t(lr), "b1": b1, "b2": b2, "omb1": one - b1, "omb2": one - b2,
         "eps": t(eps), "wd": t(wd), "ibc1": ibc1, "isbc2": isbc2}
    return {k: v.item() for k, v in c.items()}, cover


def adamw_ref_bound(p32, g, m, v, lr: float, beta1: float, beta2: float,
                    eps: float, wd: float, step: int
                    ) -> Dict[str, torch.Tensor]:
    """One step of adamw_kernel in fp64 from the fp32 values the kernel
    holds (``_adamw_consts``) -> ``m``, ``v``, ``p32`` and their bounds.

      m' = fma(b1, m, omb1 g):            2 f (|b1 m| + |omb1 g|)
      v' = fma(b2, v, (omb2 g) g):        3 f (b2 v + omb2 g^2)
      mhat = m' ibc1, denom = sqrtf(v') isbc2 + eps (all terms >= 0:
             1.5 f from v', sqrtf, product, add: rel(denom) <= 4.5 f + cover)
      upd = mhat / denom:                 err(m') ibc1 / denom
                                          + |upd| (8 f + cover)
      p' = p - lr (upd + wd p):           the sum, the product with lr and
             the product wd p add 3 f (|upd| + |wd p|), the subtraction
             f |p'|.

      p32_bound = f |p'| + |lr| (err(m') ibc1 / denom + |upd| (11 f + cover)
                                 + 3 f |wd p|).

    ``cover`` is the powf term, relative to the update.  p16 has no bound:
    it must equal ``p32.bfloat16()`` of the kernel's own p32."""
    c, cover = _adamw_consts(lr, beta1, beta2, eps, wd, step)
    pf, gf, mf, vf = p32.double(), g.double(), m.double(), v.double()
    tm = (c["b1"] * mf).abs() + (c["omb1"] * gf).abs()
    m1 = c["b1"] * mf + c["omb1"] * gf
    v1 = c["b2"] * vf + c["omb2"] * gf * gf
    em = 2 * F * tm
    denom = v1.sqrt() * c["isbc2"] + c["eps"]
    upd = m1 * c["ibc1"] / denom
    p1 = pf - c["lr"] * (upd + c["wd"] * pf)
    p_bound = F * p1.abs() + abs(c["lr"]) * (
        em * c["ibc1"] / denom + upd.abs() * (11 * F + cover)
        + 3 * F * (c["wd"] * pf).abs())
    return {"m": m1, "m_bound": em, "v": v1, "v_bound": 3 * F * v1.abs(),
            "p32": p1, "p32_bound": p_bound}


def emulate_adamw(p32, g, m, v, lr, beta1, beta2, eps, wd, step: int,
                  fault: Optional[str] = None):
    """fp32 emulation of one adamw_kernel step -> (p32, p16, m, v), new
    tensors.  ``fault``: "no_bias_correction", "wd_after_update" (weight
    decay applied to the updated p), "eps_in_sqrt" (eps added under the
    square root)."""
    c, _ = _adamw_consts(lr, beta1, beta2, eps, wd, step, fault)
    t = lambda k: torch.tensor(c[k], dtype=_F32)    # noqa: E731
    gf = g.float()
    m1 = _fma32(t("b1").expand_as(m), m, t("omb1") * gf)
    v1 = _fma32(t("b2").expand_as(v), v, t("omb2") * gf * gf)
    mhat = m1 * t("ibc1")
    if fault == "eps_in_sqrt":
        denom = torch.sqrt(v1 * t("isbc2") * t("isbc2") + t("eps"))
    else:
        denom = torch.sqrt(v1) * t("isbc2") + t("eps")
    if fault == "wd_after_update":
        p1 = p32 - t("lr") * (mhat / denom)
        p1 = p1 - t("lr") * (t("wd") * p1)
    else:
        p1 = p32 - t("lr") * (mhat / denom + t("wd") * p32)
    return p1, p1.to(_BF), m1, v1


def adamw_inputs(family: str, n: int, seed: int):
    """(p32 f32, g bf16, m f32, v f32 >= 0).  ``flat``: randn parameters and
    gradients with nonzero starting moments.  ``edges`` gives element i, by
    i % 4: g = m = v = 0 (update 0 / eps); sqrt(v') far below eps (g 1e-12,
    v 1e-26) under a live m; large gradient (1e3) on small moments; randn
    with nonzero moments."""
    assert family in FAMILIES, family
    gen = _gen(seed)
    p = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen)
    m = 0.1 * torch.randn(n, generator=gen)
    v = (0.1 * torch.randn(n, generator=gen)) ** 2
    if family == "edges":
        k = torch.arange(n) % 4
        g = torch.where(k == 0, 0.0, g)
        m = torch.where(k == 0, 0.0, m)
        v = torch.where(k == 0, 0.0, v)
        g = torch.where(k == 1, 1e-12, g)
        m = torch.where(k == 1, 1e-10 * m, m)
        v = torch.where(k == 1, 1e-26, v)
        g = torch.where(k == 2, 1e3 * g, g)
    return p, g.to(_BF), m, v


ADAMW_N = (4, 1020, 3076)       # one vector; a partial block; four blocks
# (lr, beta1, beta2, eps, wd, step), every one run at every n and family
ADAMW_CONFIGS = [(1e-3, 0.9, 0.95, 1e-8, 0.1, 1),
                 (1e-3, 0.9, 0.95, 1e-8, 0.0, 2),
                 (3e-4, 0.9, 0.999, 1e-8, 0.1, 1000)]


# ---------------------------------------------------------------------------
# fp8 cast + transpose (exact) and the bf16 transpose
# ---------------------------------------------------------------------------


def fp8_format(e5m2: bool):
    """(torch dtype, fmax, mantissa bits, exponent of the smallest normal)."""
    return ((torch.float8_e5m2, 57344.0, 2, -14) if e5m2
            else (torch.float8_e4m3fn, 448.0, 3, -6))


def _fp8_scaled(x: torch.Tensor, scale: float) -> torch.Tensor:
    """fp32(x) * inv with inv = fp32(1) / fp32(scale), as the kernel forms
    it (one correctly rounded division, one product)."""
    inv = torch.tensor(1.0, dtype=_F32) / torch.tensor(scale, dtype=_F32)
    return x.float().cpu() * inv


def fp8_cast_ref(x: torch.Tensor, scale: float, e5m2: bool
                 ) -> Dict[str, torch.Tensor]:
    """x bf16 [R, C] -> the exact ``out`` [R, C], ``out_t`` [C, R] (float8)
    and ``amax`` (f32 [1]) of fp8_cast_transpose_kernel:
    clamp(fp32(x) * inv, +-fmax) cast round-to-nearest-even, its transpose,
    and max |x|.  Computed on the CPU."""
    dt, fmax, _, _ = fp8_format(e5m2)
    out = _fp8_scaled(x, scale).clamp(-fmax, fmax).to(dt)
    return {"out": out, "out_t": out.t().contiguous(),
            "amax": x.float().cpu().abs().max().reshape(1)}


def fp8_bits(t: torch.Tensor) -> torch.Tensor:
    """The bytes of a float8 tensor (torch.equal on them tells -0 from 0)."""
    return t.contiguous().view(torch.uint8).cpu()


def _fp8_grid(y: torch.Tensor, e5m2: bool):
    """y fp32 -> (y / q in fp64, q) with q the spacing of the format at
    |y| (exact: powers of two)."""
    _, _, mbits, emin = fp8_format(e5m2)
    yd = y.double()
    _, e = torch.frexp(yd.abs())
    ex = (e - 1).clamp(min=emin)
    q = torch.pow(torch.tensor(2.0, dtype=_F64), (ex - mbits).double())
    return yd / q, q


def emulate_fp8_cast(x, scale: float, e5m2: bool,
                     fault: Optional[str] = None):
    """The cast by explicit rounding on the format's grid -> (out, out_t,
    amax) as ``fp8_cast_ref``.  ``fault``: "truncate" (round toward zero
    instead of to nearest even), "no_clamp" (values beyond fmax become
    NaN), "edge_tile_neighbour" (where R > 64 is no multiple of 64, the
    out_t columns of the last row tile are taken from the rows of the tile
    before)."""
    dt, fmax, _, _ = fp8_format(e5m2)
    y = _fp8_scaled(x, scale)
    if fault != "no_clamp":
        y = y.clamp(-fmax, fmax)
    v, q = _fp8_grid(y, e5m2)
    r = (torch.trunc(v) if fault == "truncate" else torch.round(v)) * q
    r = torch.where(r.abs() > fmax, torch.full_like(r, float("nan")), r)
    out = r.float().to(dt)
    out_t = out.t().contiguous()
    R = x.shape[0]
    if fault == "edge_tile_neighbour" and R % 64 and R > 64:
        r0 = R // 64 * 64
        out_t[:, r0:] = out[r0 - 64:R - 64].t()
    return out, out_t, x.float().cpu().abs().max().reshape(1)


def _fp8_edge_targets(e5m2: bool):
    """Values of y = x / scale that the ``edges`` family aims at: exact
    ties of the format (normal range, next to fmax, subnormal range), other
    subnormals, +-0 and values beyond fmax."""
    _, fmax, mbits, emin = fp8_format(e5m2)
    sp = 2.0 ** (emin - mbits)               # subnormal spacing
    h = 2.0 ** -(mbits + 1)                  # half a spacing in [1, 2)
    top = 2.0 ** math.floor(math.log2(fmax))
    t = [1 + h, 1 + 3 * h, 16 * (1 + h), 16 * (1 + 3 * h),
         fmax - top * h, fmax - 3 * top * h,
         0.5 * sp, 1.5 * sp, 2.5 * sp,
         sp, 3 * sp, 0.25 * sp, 0.75 * sp, 5 * sp,
         0.0, fmax, fmax + top * h, 2 * fmax, 25 * fmax]
    return t + [-a for a in t]


def fp8_inputs(family: str, R: int, C: int, e5m2: bool, scale: float,
               seed: int) -> torch.Tensor:
    """x bf16 [R, C].  ``flat``: randn scaled so that y = x / scale covers
    the normal range (std 8).  ``edges``: x = bf16(t * scale) for the
    targets t of ``_fp8_edge_targets`` (exact for the power-of-two scales;
    for other scales the x of ``fp8_exact_tie_inputs`` are added), repeated
    over the matrix in an order shuffled by the seed."""
    assert family in FAMILIES, family
    g = _gen(seed)
    if family == "flat":
        return (torch.randn(R, C, generator=g) * (8.0 * scale)).to(_BF)
    t = (torch.tensor(_fp8_edge_targets(e5m2), dtype=_F64) * scale).to(_BF)
    if math.frexp(scale)[0] != 0.5:
        t = torch.cat([t, fp8_exact_tie_inputs(scale, e5m2)])
    idx = torch.randperm(R * C, generator=g) % t.numel()
    return t[idx].view(R, C)


def fp8_exact_tie_inputs(scale: float, e5m2: bool) -> torch.Tensor:
    """Every bf16 x whose y = fp32(x) * inv is an exact tie of the format,
    by search over all bf16 values.  For a scale that is no power of two
    these are the rare x at which the fp32 product happens to round onto a
    tie (none at all for e5m2 and 0.37): there the result depends on inv
    being the correctly rounded quotient."""
    _, fmax, _, _ = fp8_format(e5m2)
    every = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(_BF)
    every = every[torch.isfinite(every.float())]
    y = _fp8_scaled(every, scale)
    v, _ = _fp8_grid(y, e5m2)
    return every[((v.abs() - torch.floor(v.abs())) == 0.5) & (y.abs() <= fmax)]


def fp8_edge_coverage(x: torch.Tensor, scale: float, e5m2: bool
                      ) -> Dict[str, int]:
    """What y = fp32(x) * inv holds: the number of exact ties of the format
    (``tie``), of ties in the sense that x is the bf16 value nearest to
    scale times a tie (``near_tie``: the fp32 product decides the result),
    of nonzero values in the subnormal range and of values beyond fmax."""
    _, fmax, _, emin = fp8_format(e5m2)
    y = _fp8_scaled(x, scale)
    inr = y.abs() <= fmax
    v, _ = _fp8_grid(y, e5m2)
    frac = (v.abs() - torch.floor(v.abs()))
    return {"tie": int(((frac == 0.5) & inr).sum()),
            "near_tie": int((((frac - 0.5).abs() <= 2.0 ** -5) & inr).sum()),
            "subnormal": int(((y != 0) & (y.abs() < 2.0 ** emin)).sum()),
            "saturating": int((y.abs() > fmax).sum())}


# (R, C): the smallest the binding takes (one partial tile); one full tile;
# partial tiles in both directions over several tiles; a partial row tile;
# a partial column tile; 4 x 3 full tiles
FP8_CASES = [(8, 8), (64, 64), (72, 200), (136, 64), (64, 136), (256, 192)]
FP8_SCALES = (1.0, 2.0 ** -3, 2.0 ** 4, 0.37)

# (R, C): one tile; 33 row tiles, one full group of 32 and a group of one
TRANSPOSE_CASES = [(64, 64), (33 * 64, 128)]
