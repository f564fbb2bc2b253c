"""The kernels of the training step (RMSNorm, RoPE, SwiGLU, cross entropy,
AdamW, fp8 cast+transpose, bf16 transpose) against fp64 references under
the derived per-element bounds of torchx_amd.ops.bounds_train, at the
smallest shapes at which each code path exists: vector tails, partial tiles,
threads without work, the four RMSNorm instances, and per op an ``edges``
input family that reaches the places the arithmetic can go wrong.

Each test asserts err <= bound elementwise and prints max err / bound (the
fp8 cast and the transposes: bit equality); tests/test_train_bounds_cpu.py
shows without a GPU that emulations of the kernels' arithmetic stay within
the same bounds on the same cases and that injected faults do not.  Inputs
are drawn on the CPU from a fixed seed per case, references are computed
there in fp64.  The second half holds the input guards of the bindings and
the defined results for inputs the kernels used to mishandle.
"""

import pytest
import torch

from torchx_amd.ops import bounds_train as bt

pytestmark = pytest.mark.gpu

EPS = bt.RMSNORM_EPS
BF = torch.bfloat16


def _ops():
    from torchx_amd import ops

    assert ops.extension_available(), "HIP extension must be built in-tree"
    return ops


def _hip():
    return _ops().hip_ops(required=True)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _seed(*parts):
    return bt.case_seed("-".join(str(p) for p in parts))


def _check(label, got, ref, names=None):
    """got: {name: tensor}; ref holds name and name_bound.  Print max
    err/bound per tensor, then assert err <= bound elementwise."""
    res = {n: bt.bound_ratio(g.cpu(), ref[names[n] if names else n],
                             ref[(names[n] if names else n) + "_bound"])
           for n, g in got.items()}
    print(f"{label} max err/bound: " +
          " ".join(f"{n} {r[0]:.3g}" for n, r in res.items()))
    for n, r in res.items():
        assert r[1], f"{label}: {n} max err/bound = {r[0]:.4g}"


def _to(dev, *ts):
    return tuple(t.to(dev) for t in ts)


# ---------------------------------------------------------------------------
# RMSNorm
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("case", bt.RMSNORM_CASES,
                         ids=[c[0] for c in bt.RMSNORM_CASES])
def test_rmsnorm(dev, case):
    hip = _hip()
    cid, rows, H = case
    for family in bt.FAMILIES:
        x, w, dy, other = bt.rmsnorm_inputs(family, rows, H, _seed("rms", cid))
        xd, wd, dyd, od = _to(dev, x, w, dy, other)
        y, inv = hip.rmsnorm_fwd(xd, wd, EPS)
        _check(f"rmsnorm {cid} {family}", {"y": y, "invrms": inv},
               bt.rmsnorm_fwd_ref_bound(x, w, EPS))

        # the residual forms: s = bf16(x + delta) exactly, then the norm of s
        s, ys, invs = hip.add_rmsnorm_fwd(xd, od, wd, EPS)
        s_ref = (x.float() + other.float()).to(BF)
        assert torch.equal(s.cpu(), s_ref)
        _check(f"add_rmsnorm {cid} {family}", {"y": ys, "invrms": invs},
               bt.rmsnorm_fwd_ref_bound(s_ref, w, EPS))
        s2, y2 = hip.rmsnorm_res(xd, od, wd, EPS)
        assert torch.equal(s2, s) and torch.equal(y2, ys)

        # backward, from the kernel's own invrms
        dx, dw = hip.rmsnorm_bwd(dyd, xd, wd, inv, None)
        dxr, dwr = hip.rmsnorm_bwd(dyd, xd, wd, inv, od)
        got = {"dx": dx, "dw": dw}
        ref = dict(bt.rmsnorm_dx_ref_bound(dy, x, w, inv.cpu()))
        ref.update(bt.rmsnorm_dw_ref_bound(dy, x, inv.cpu()))
        _check(f"rmsnorm_bwd {cid} {family}", got, ref)
        _check(f"rmsnorm_bwd+dres {cid} {family}", {"dx": dxr},
               bt.rmsnorm_dx_ref_bound(dy, x, w, inv.cpu(), other))
        # two roundings: the bits of the dx kernel followed by a bf16 add
        assert torch.equal(dxr, (dx.float() + od.float()).to(BF))
        assert torch.equal(dwr, dw)


def test_rmsnorm_autograd(dev):
    ops = _ops()
    cid, rows, H = bt.RMSNORM_CASES[4]           # r3-H4096
    x, w, dy, other = bt.rmsnorm_inputs("flat", rows, H, _seed("rms", cid))
    xd, wd, od = (t.to(dev).requires_grad_(True) for t in (x, w, other))
    y = ops.rmsnorm(xd, wd, EPS)
    _check("ops.rmsnorm", {"y": y.detach()},
           bt.rmsnorm_fwd_ref_bound(x, w, EPS))
    y.backward(dy.to(dev))
    inv = _hip().rmsnorm_fwd(x.to(dev), w.to(dev), EPS)[1].cpu()
    _check("ops.rmsnorm bwd", {"dx": xd.grad},
           bt.rmsnorm_dx_ref_bound(dy, x, w, inv))
    dw = bt.rmsnorm_dw_ref_bound(dy, x, inv)
    # the wrapper rounds the fp32 dw to the weight's bf16
    assert bt.bound_ratio(wd.grad.cpu(), dw["dw"],
                          dw["dw_bound"] + bt.U * dw["dw"].abs())[1]

    xd.grad = None
    s, y = ops.add_rmsnorm(xd, od, wd, EPS)
    s_ref = (x.float() + other.float()).to(BF)
    assert torch.equal(s.detach().cpu(), s_ref)
    _check("ops.add_rmsnorm", {"y": y.detach()},
           bt.rmsnorm_fwd_ref_bound(s_ref, w, EPS))
    (y * dy.to(dev)).sum().backward()
    assert torch.equal(xd.grad, od.grad)
    inv = _hip().rmsnorm_fwd(s_ref.to(dev), w.to(dev), EPS)[1].cpu()
    _check("ops.add_rmsnorm bwd", {"dx": xd.grad},
           bt.rmsnorm_dx_ref_bound(dy, s_ref, w, inv))


# ---------------------------------------------------------------------------
# RoPE
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("case", bt.ROPE_CASES,
                         ids=[c[0] for c in bt.ROPE_CASES])
def test_rope(dev, case):
    """Both directions through the kernel entry point (tables of exactly S
    rows) and through ops.rope with its autograd backward (any table of at
    least S rows: the 16-row table must give the ``cos[:S]`` reference)."""
    ops = _ops()
    cid, B, S, H, D, rows = case
    x, cos, sin = bt.rope_inputs(B, S, H, D, rows, _seed("rope", cid))
    xd, cd, sd = _to(dev, x, cos, sin)
    fwd = bt.rope_ref_bound(x, cos, sin, 1.0)
    bwd = bt.rope_ref_bound(x, cos, sin, -1.0)
    if rows == S:
        hip = ops.hip_ops()
        _check(f"rope {cid}", {"y": hip.rope(xd, cd, sd, H, 1.0)}, fwd)
        _check(f"rope {cid} inverse", {"y": hip.rope(xd, cd, sd, H, -1.0)},
               bwd)
    xg = xd.clone().requires_grad_(True)
    y = ops.rope(xg, cd, sd)
    _check(f"ops.rope {cid}", {"y": y.detach()}, fwd)
    y.backward(xd)                       # dy = x: the inverse rotation of x
    _check(f"ops.rope {cid} bwd", {"y": xg.grad}, bwd)


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("case", bt.ROPE_QKV_CASES,
                         ids=[c[0] for c in bt.ROPE_QKV_CASES])
def test_rope_qkv(dev, case, sign, inplace):
    hip = _hip()
    cid, B, S, Hq, Hkv = case
    x, cos, sin = bt.rope_inputs(B, S, Hq + 2 * Hkv, 128, S + 3,
                                 _seed("ropeqkv", cid))
    qkv = x.reshape(B, S, -1)
    qd, cd, sd = _to(dev, qkv.clone(), cos, sin)
    y = hip.rope_qkv(qd, cd, sd, Hq, Hkv, sign, inplace)
    assert (y.data_ptr() == qd.data_ptr()) == inplace
    _check(f"rope_qkv {cid} sign {sign:+.0f} inplace {inplace}", {"y": y},
           bt.rope_qkv_ref_bound(qkv, cos, sin, Hq, Hkv, sign))
    v0 = (Hq + Hkv) * 128
    assert torch.equal(y[..., v0:].cpu(), qkv[..., v0:])


# ---------------------------------------------------------------------------
# SwiGLU
# ---------------------------------------------------------------------------


def _soil(dev, n, count):
    """Leave ``count`` freed blocks of n bf16 sentinels for the allocator to
    hand to the next empty_like, and run the op's forward once on sentinels
    for the same reason."""
    junk = [torch.full((n,), bt.SWIGLU_SENTINEL, device=dev, dtype=BF)
            for _ in range(count)]
    junk.append(_hip().swiglu_fwd(junk[0], junk[0]))
    torch.cuda.synchronize()
    del junk


@pytest.mark.parametrize("n", bt.SWIGLU_FLAT_N)
def test_swiglu_flat(dev, n):
    """Every element against the bound, the n % 8 tail included, with the
    output allocations' likely contents set to a sentinel first."""
    hip = _hip()
    for family in bt.FAMILIES:
        g, u, dout = bt.swiglu_inputs(family, n, _seed("swiglu", n))
        gd, ud, dd = _to(dev, g, u, dout)
        _soil(dev, n, 2)
        out = hip.swiglu_fwd(gd, ud)
        _soil(dev, n, 3)
        dg, du = hip.swiglu_bwd(dd, gd, ud)
        assert out.shape == dg.shape == du.shape == (n,)
        _check(f"swiglu n={n} {family}", {"out": out},
               bt.swiglu_ref_bound(g, u))
        _check(f"swiglu_bwd n={n} {family}", {"dg": dg, "du": du},
               bt.swiglu_bwd_ref_bound(dout, g, u))


def test_swiglu_autograd_any_shape(dev):
    """ops.swiglu takes any shape on the GPU as it does on the CPU: [3, 5]
    is 15 elements, one vector and a tail of 7."""
    ops = _ops()
    g, u, dout = bt.swiglu_inputs("flat", 15, 15)
    gd, ud = (t.view(3, 5).to(dev).requires_grad_(True) for t in (g, u))
    _soil(dev, 15, 2)
    out = ops.swiglu(gd, ud)
    assert out.shape == (3, 5)
    _check("ops.swiglu", {"out": out.detach().reshape(-1)},
           bt.swiglu_ref_bound(g, u))
    _soil(dev, 15, 3)
    out.backward(dout.view(3, 5).to(dev))
    _check("ops.swiglu bwd", {"dg": gd.grad.reshape(-1),
                              "du": ud.grad.reshape(-1)},
           bt.swiglu_bwd_ref_bound(dout, g, u))


def _packed(family, rows, inter):
    g, u, dout = bt.swiglu_inputs(family, rows * inter,
                                  _seed("swiglu-gu", rows, inter))
    g, u, dout = (t.view(rows, inter) for t in (g, u, dout))
    return g, u, dout, torch.cat([g, u], -1).contiguous()


def _packed_ref(dout, g, u):
    r = bt.swiglu_bwd_ref_bound(dout, g, u)
    return {"dgu": torch.cat([r["dg"], r["du"]], -1),
            "dgu_bound": torch.cat([r["dg_bound"], r["du_bound"]], -1)}


@pytest.mark.parametrize("case", bt.SWIGLU_PACKED_CASES,
                         ids=lambda c: "%dx%d" % c)
def test_swiglu_packed(dev, case):
    ops = _ops()
    hip = ops.hip_ops()
    rows, inter = case
    for family in bt.FAMILIES:
        g, u, dout, gu = _packed(family, rows, inter)
        gud, dd = _to(dev, gu, dout)
        _check(f"swiglu_gu {rows}x{inter} {family}",
               {"out": hip.swiglu_gu_fwd(gud)}, bt.swiglu_ref_bound(g, u))
        _check(f"swiglu_gu_bwd {rows}x{inter} {family}",
               {"dgu": hip.swiglu_gu_bwd(dd, gud)}, _packed_ref(dout, g, u))
    gug = gud.clone().requires_grad_(True)
    out = ops.swiglu_packed(gug)
    assert torch.equal(out.detach(), hip.swiglu_gu_fwd(gud))
    out.backward(dd)
    assert torch.equal(gug.grad, hip.swiglu_gu_bwd(dd, gud))


@pytest.mark.parametrize("case", bt.SWIGLU_BWD_T_CASES,
                         ids=lambda c: "%dx%d" % c)
def test_swiglu_gu_bwd_t(dev, case):
    hip = _hip()
    rows, inter = case
    for family in bt.FAMILIES:
        g, u, dout, gu = _packed(family, rows, inter)
        gud, dd = _to(dev, gu, dout)
        dgu, dgut = hip.swiglu_gu_bwd_t(dd, gud)
        _check(f"swiglu_gu_bwd_t {rows}x{inter} {family}", {"dgu": dgu},
               _packed_ref(dout, g, u))
        assert dgut.shape == (2 * inter, rows) and dgut.is_contiguous()
        assert torch.equal(dgut, dgu.t())


# ---------------------------------------------------------------------------
# cross entropy
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("case", bt.CE_CASES, ids=lambda c: "%dx%d" % c)
def test_cross_entropy(dev, case):
    hip = _hip()
    T, V = case
    for family in bt.FAMILIES:
        x, t, gs = bt.ce_inputs(family, T, V, _seed("ce", T, V))
        xd, td, gd = _to(dev, x, t, gs)
        loss, lse = hip.ce_fwd(xd, td)
        _check(f"ce {T}x{V} {family}", {"lse": lse, "loss": loss},
               bt.ce_ref_bound(x, t))
        d = hip.ce_bwd(xd, td, lse, gd)
        _check(f"ce_bwd {T}x{V} {family}", {"dlogits": d},
               bt.ce_bwd_ref_bound(x, t, lse.cpu(), gs))


def test_cross_entropy_autograd(dev):
    ops = _ops()
    T, V = 5, 1003
    x, t, _ = bt.ce_inputs("flat", T, V, _seed("ce", T, V))
    xd = x.to(dev).requires_grad_(True)
    loss = ops.cross_entropy(xd, t.to(dev))
    ref = bt.ce_ref_bound(x, t)
    # the mean of T fp32 losses: their bounds, plus T roundings of the sum
    bound = ref["loss_bound"].mean() + T * bt.F * ref["loss"].abs().mean()
    assert abs(loss.item() - ref["loss"].mean().item()) <= bound.item()
    (loss * 3.0).backward()
    lse = ops.hip_ops().ce_fwd(x.to(dev), t.to(dev))[1].cpu()
    gs = torch.full((T,), 3.0) / T
    _check("ops.cross_entropy bwd", {"dlogits": xd.grad},
           bt.ce_bwd_ref_bound(x, t, lse, gs))


def test_cross_entropy_target_out_of_range(dev):
    """A target outside [0, V) (torch's ignore_index -100 included) has no
    loss on the GPU path: NaN for that row, deterministically; lse and the
    other rows are unaffected, and the backward's row is the plain softmax."""
    hip = _hip()
    T, V = 5, 1003
    x, t, gs = bt.ce_inputs("flat", T, V, _seed("ce", T, V))
    t[0], t[2], t[4] = -100, V, -1
    xd, td, gd = _to(dev, x, t, gs)
    ref = bt.ce_ref_bound(x, t)
    for _ in range(2):
        loss, lse = hip.ce_fwd(xd, td)
        assert torch.isnan(loss.cpu()).tolist() == [True, False, True, False,
                                                    True]
        ratio, ok = bt.ce_loss_ok(loss.cpu(), ref)
        assert ok, ratio
        _check("ce out-of-range targets", {"lse": lse}, ref)
    d = hip.ce_bwd(xd, td, lse, gd)
    _check("ce_bwd out-of-range targets", {"dlogits": d},
           bt.ce_bwd_ref_bound(x, t, lse.cpu(), gs))
    assert torch.isnan(_ops().cross_entropy(xd, td)).item()


# ---------------------------------------------------------------------------
# AdamW
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("n", bt.ADAMW_N)
def test_adamw(dev, n):
    hip = _hip()
    for family in bt.FAMILIES:
        for i, cfg in enumerate(bt.ADAMW_CONFIGS):
            p, g, m, v = bt.adamw_inputs(family, n, _seed("adamw", n, i))
            ref = bt.adamw_ref_bound(p, g, m, v, *cfg)
            pd, gd, md, vd = _to(dev, p.clone(), g, m.clone(), v.clone())
            p16 = torch.full((n,), bt.SWIGLU_SENTINEL, device=dev, dtype=BF)
            hip.adamw_step(pd, p16, gd, md, vd, *cfg)
            _check(f"adamw n={n} {family} step={cfg[5]} wd={cfg[4]}",
                   {"p32": pd, "m": md, "v": vd}, ref)
            assert torch.equal(p16, pd.bfloat16())
            assert torch.equal(gd.cpu(), g)


def test_adamw_wrapper(dev):
    ops = _ops()
    n, cfg = 1020, bt.ADAMW_CONFIGS[0]
    p, g, m, v = bt.adamw_inputs("flat", n, _seed("adamw", n, 0))
    ref = bt.adamw_ref_bound(p, g, m, v, *cfg)
    pd, gd, md, vd = _to(dev, p.clone(), g, m.clone(), v.clone())
    p16 = torch.zeros(n, device=dev, dtype=BF)
    ops.adamw_step(pd, p16, gd, md, vd, lr=cfg[0], beta1=cfg[1],
                   beta2=cfg[2], eps=cfg[3], weight_decay=cfg[4], step=cfg[5])
    _check("ops.adamw_step", {"p32": pd, "m": md, "v": vd}, ref)
    assert torch.equal(p16, pd.bfloat16())


# ---------------------------------------------------------------------------
# fp8 cast + transpose, bf16 transpose: exact
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("e5m2", [False, True], ids=["e4m3", "e5m2"])
@pytest.mark.parametrize("case", bt.FP8_CASES, ids=lambda c: "%dx%d" % c)
def test_fp8_cast_transpose_exact(dev, case, e5m2):
    """out, out_t and amax bit for bit (bytes compared, so -0 is told from
    0), at every scale and family; out_t == out.t() regardless of the
    reference.  Scale 0.37 holds the kernel's 1.0f / scale to the correctly
    rounded quotient: its edges include every x whose fp32 product lands on
    an exact tie."""
    hip = _hip()
    R, C = case
    for scale in bt.FP8_SCALES:
        for family in bt.FAMILIES:
            x = bt.fp8_inputs(family, R, C, e5m2, scale,
                              _seed("fp8", R, C, e5m2, scale))
            ref = bt.fp8_cast_ref(x, scale, e5m2)
            sc = torch.tensor([scale], dtype=torch.float32, device=dev)
            out, out_t, amax = hip.fp8_cast_transpose(x.to(dev), sc, e5m2)
            label = f"fp8 {R}x{C} e5m2={e5m2} scale={scale} {family}"
            assert out.dtype == ref["out"].dtype and out.shape == (R, C)
            assert out_t.shape == (C, R)
            assert torch.equal(bt.fp8_bits(out_t),
                               bt.fp8_bits(out).t().contiguous()), label
            bad = (bt.fp8_bits(out) != bt.fp8_bits(ref["out"]))
            assert not bad.any(), (
                label, int(bad.sum()), x[bad][:4].tolist(),
                out.cpu().float()[bad][:4].tolist(),
                ref["out"].float()[bad][:4].tolist())
            assert torch.equal(bt.fp8_bits(out_t), bt.fp8_bits(ref["out_t"]))
            assert torch.equal(amax.cpu(), ref["amax"]), label


@pytest.mark.parametrize("case", bt.TRANSPOSE_CASES,
                         ids=lambda c: "%dx%d" % c)
def test_transpose_bf16_exact(dev, case):
    R, C = case
    x = torch.randn(R, C, generator=torch.Generator().manual_seed(R + C)
                    ).to(BF).to(dev)
    t = _hip().transpose_bf16(x)
    assert t.shape == (C, R) and t.is_contiguous()
    assert torch.equal(t, x.t())


# ---------------------------------------------------------------------------
# input guards: each of these used to launch on buffers it had not checked
# ---------------------------------------------------------------------------


def _raises(fn, *args):
    with pytest.raises(RuntimeError):
        fn(*args)


def test_rope_guards_and_long_table(dev):
    """The kernel takes a row's position modulo the table length: the
    binding refuses an x that is no whole number of [S, heads, D] blocks of
    its table (so a longer table cannot rotate b >= 1 by wrong positions),
    a head_dim off the 4-pair vector, and a sin unlike cos; ops.rope hands
    the kernel the S rows it needs and refuses a table shorter than S."""
    ops = _ops()
    hip = ops.hip_ops()
    cid, B, S, H, D, rows = bt.ROPE_CASES[3]     # 16-row table
    x, cos, sin = bt.rope_inputs(B, S, H, D, rows, _seed("rope", cid))
    xd, cd, sd = _to(dev, x, cos, sin)
    _raises(hip.rope, xd, cd, sd, H, 1.0)
    assert torch.equal(ops.rope(xd, cd, sd), hip.rope(xd, cd[:S], sd[:S], H,
                                                      1.0))
    _raises(hip.rope, xd, cd[:S], sd[:S - 1], H, 1.0)
    _raises(hip.rope, xd, cd[:S], sd[:S, :D // 4].contiguous(), H, 1.0)
    with pytest.raises(ValueError):
        ops.rope(xd, cd[:S - 1], sd[:S - 1])
    x4 = torch.zeros(1, 1, 1, 4, device=dev, dtype=BF)
    t4 = torch.zeros(1, 2, device=dev)
    _raises(hip.rope, x4, t4, t4, 1, 1.0)


def test_rope_qkv_guards(dev):
    hip = _hip()
    B, S, Hq, Hkv = 2, 5, 4, 2
    qkv = torch.zeros(B, S, (Hq + 2 * Hkv) * 128, device=dev, dtype=BF)
    ok = torch.zeros(S, 64, device=dev)
    hip.rope_qkv(qkv, ok, ok, Hq, Hkv, 1.0, False)
    short = torch.zeros(S - 1, 64, device=dev)
    narrow = torch.zeros(S, 32, device=dev)
    _raises(hip.rope_qkv, qkv, short, short, Hq, Hkv, 1.0, False)
    _raises(hip.rope_qkv, qkv, narrow, narrow, Hq, Hkv, 1.0, False)
    _raises(hip.rope_qkv, qkv, ok, short, Hq, Hkv, 1.0, False)
    _raises(hip.rope_qkv, qkv, ok, ok.double(), Hq, Hkv, 1.0, False)


def test_swiglu_guards(dev):
    hip = _hip()
    a = torch.zeros(16, device=dev, dtype=BF)
    b = torch.zeros(8, device=dev, dtype=BF)
    f = torch.zeros(16, device=dev)
    _raises(hip.swiglu_fwd, a, b)
    _raises(hip.swiglu_bwd, a, f, a)
    _raises(hip.swiglu_bwd, a, a, f)
    _raises(hip.swiglu_bwd, a, b, a)
    _raises(hip.swiglu_bwd, a, a, b)
    _raises(hip.swiglu_bwd, a, a.cpu(), a)
    _raises(hip.swiglu_bwd, a, a.view(4, 4).t(), a)
    gu = torch.zeros(2, 32, device=dev, dtype=BF)
    dout = torch.zeros(2, 16, device=dev, dtype=BF)
    hip.swiglu_gu_bwd(dout, gu)
    _raises(hip.swiglu_gu_bwd, dout, gu.float())
    _raises(hip.swiglu_gu_bwd, dout, gu.cpu())
    _raises(hip.swiglu_gu_bwd, dout[:1], gu)
    _raises(hip.swiglu_gu_bwd, torch.zeros(2, 12, device=dev, dtype=BF),
            torch.zeros(2, 24, device=dev, dtype=BF))
    _raises(hip.swiglu_gu_bwd, dout.view(4, 8), gu)


def test_ce_guards(dev):
    hip = _hip()
    x = torch.zeros(3, 16, device=dev, dtype=BF)
    t = torch.zeros(3, device=dev, dtype=torch.long)
    loss, lse = hip.ce_fwd(x, t)
    gs = torch.ones(3, device=dev)
    for fn, rest in ((hip.ce_fwd, ()), (hip.ce_bwd, (lse, gs))):
        _raises(fn, x, t.cpu(), *rest)
        _raises(fn, x, t.int(), *rest)
        _raises(fn, x, t[:2], *rest)
        _raises(fn, x, torch.zeros(6, device=dev, dtype=torch.long)[::2],
                *rest)
    _raises(hip.ce_bwd, x, t, lse[:2], gs)
    _raises(hip.ce_bwd, x, t, lse, gs[:2])


def test_adamw_guards(dev):
    hip = _hip()
    n = 8
    p = torch.zeros(n, device=dev)
    p16 = torch.zeros(n, device=dev, dtype=BF)
    g = torch.zeros(n, device=dev, dtype=BF)
    cfg = bt.ADAMW_CONFIGS[0]
    hip.adamw_step(p, p16, g, p.clone(), p.clone(), *cfg)
    half = torch.zeros(n // 2, device=dev)
    _raises(hip.adamw_step, p, p16, g, half, p.clone(), *cfg)
    _raises(hip.adamw_step, p, p16, g, p.clone(), half, *cfg)
    _raises(hip.adamw_step, p, p16, g, p.double(), p.clone(), *cfg)
    _raises(hip.adamw_step, p, p16, g, p.clone(), p.bfloat16(), *cfg)
    _raises(hip.adamw_step, p, p16, g, p.cpu(), p.clone(), *cfg)
    _raises(hip.adamw_step, p, p16, g, p.clone(),
            torch.zeros(2 * n, device=dev)[::2], *cfg)
    _raises(hip.adamw_step, p, p16[:4], g, p.clone(), p.clone(), *cfg)
    _raises(hip.adamw_step, p, p16, g[:4], p.clone(), p.clone(), *cfg)


def test_rmsnorm_weight_length_guard(dev):
    hip = _hip()
    x = torch.zeros(2, 4096, device=dev, dtype=BF)
    _raises(hip.rmsnorm_fwd, x, torch.zeros(2048, device=dev, dtype=BF), EPS)
