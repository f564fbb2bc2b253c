"""The training-kernel error bounds of torchx_amd.ops.bounds_train, checked
without a GPU against plain torch emulations that round where the kernels
round.

  reference alone  the clean emulation stays within every bound at every
                   case and family tests/test_train_bounds.py runs (the fp8
                   cast: equals the exact reference), max err / bound printed
                   per op;
  sensitivity      every injected fault pushes the emulation over a bound at
                   some listed case (fp8 cast: breaks equality), and what the
                   older metric of tests/test_ops_gpu.py, max|err| / max|ref|
                   under its limit, says at those very cases is asserted;
  coverage         properties of the inputs: the SwiGLU edges reach the exp2
                   overflow, the CE cases put a row maximum in the scalar
                   tail, the fp8 edges hold ties, subnormals and saturating
                   values for every format and scale.

Faults the older metric lets through, i.e. passes at a place where the bound
catches them (OLD_METRIC_PASSES below): rmsnorm "mean_2048" (on invrms) and
"kk_r2", swiglu "dsilu_no_g_term", CE "lse_no_tail" and "empty_s1", AdamW
"wd_after_update" and "eps_in_sqrt".  It catches the others, which put an
error of the size of the largest element somewhere: rmsnorm "no_eps" (NaN),
both rope faults, the SwiGLU sentinel tail (because the sentinel is large:
what empty_like returns need not be), CE "onehot_plus1", AdamW
"no_bias_correction", and all three fp8 faults on the edges family.
Two faults cannot exceed a bound at all and are held otherwise:
"dres_before_round" rounds once where the kernel rounds twice, which is the
*more* accurate result, so it is held by the bit equality the kernel
promises (fused == bf16(plain dx) + dres); the CE fault "empty_s1_neg"
(s = 1 at the kernel's own m = -3.4e38) is shown to change nothing, which
is why "empty_s1" is injected at m = 0.
"""

import functools

import pytest
import torch

from torchx_amd.ops import bounds_train as bt

EPS = bt.RMSNORM_EPS


def _seed(*parts):
    return bt.case_seed("-".join(str(p) for p in parts))


def _entry(got, ref, name):
    return (got, ref[name], ref[name + "_bound"])


# ---------------------------------------------------------------------------
# one evaluation per op: (case, family, fault) -> {tensor: (got, ref, bound)}
# ---------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _rms_base(case, family):
    cid, rows, H = case
    x, w, dy, other = bt.rmsnorm_inputs(family, rows, H, _seed("rms", cid))
    s = (x.float() + other.float()).to(torch.bfloat16)
    _, r = bt.emulate_rmsnorm_fwd(x, w, EPS)
    return (x, w, dy, other, s, r,
            bt.rmsnorm_fwd_ref_bound(x, w, EPS),
            bt.rmsnorm_fwd_ref_bound(s, w, EPS),
            bt.rmsnorm_dx_ref_bound(dy, x, w, r),
            bt.rmsnorm_dx_ref_bound(dy, x, w, r, other),
            bt.rmsnorm_dw_ref_bound(dy, x, r))


def eval_rmsnorm(case, family, fault=None):
    x, w, dy, other, s, r, fwd, fwd_s, dx, dx_res, dw = _rms_base(case,
                                                                  family)
    f_fwd = fault if fault in ("no_eps", "mean_2048") else None
    f_dx = fault if fault in ("kk_r2",) else None
    y, inv = bt.emulate_rmsnorm_fwd(x, w, EPS, f_fwd)
    ys, invs = bt.emulate_rmsnorm_fwd(s, w, EPS, f_fwd)
    return {
        "y": _entry(y, fwd, "y"), "invrms": _entry(inv, fwd, "invrms"),
        "y_add": _entry(ys, fwd_s, "y"),
        "invrms_add": _entry(invs, fwd_s, "invrms"),
        "dx": _entry(bt.emulate_rmsnorm_dx(dy, x, w, r, None, f_dx), dx,
                     "dx"),
        "dx_res": _entry(bt.emulate_rmsnorm_dx(dy, x, w, r, other, f_dx),
                         dx_res, "dx"),
        "dw": _entry(bt.emulate_rmsnorm_dw(dy, x, r), dw, "dw"),
    }


def eval_rope(case, family, fault=None):
    cid, B, S, H, D, rows = case
    x, cos, sin = bt.rope_inputs(B, S, H, D, rows, _seed("rope", cid))
    out = {}
    for sign in (1.0, -1.0):
        ref = bt.rope_ref_bound(x, cos, sin, sign)
        out["y_fwd" if sign > 0 else "y_bwd"] = _entry(
            bt.emulate_rope(x, cos, sin, sign, fault), ref, "y")
    return out


def eval_rope_qkv(case, family, fault=None):
    cid, B, S, Hq, Hkv = case
    nh = Hq + Hkv
    x, cos, sin = bt.rope_inputs(B, S, Hq + 2 * Hkv, 128, S + 3,
                                 _seed("ropeqkv", cid))
    qkv = x.reshape(B, S, -1)
    out = {}
    for sign in (1.0, -1.0):
        ref = bt.rope_qkv_ref_bound(qkv, cos, sin, Hq, Hkv, sign)
        y = bt.emulate_rope(x[:, :, :nh], cos, sin, sign, fault)
        got = torch.cat([y.reshape(B, S, -1), qkv[..., nh * 128:]], -1)
        out["y_fwd" if sign > 0 else "y_bwd"] = _entry(got, ref, "y")
    return out


def _swiglu_eval(g, u, dout, fault):
    fwd = bt.swiglu_ref_bound(g, u)
    bwd = bt.swiglu_bwd_ref_bound(dout, g, u)
    f_fwd = fault if fault == "tail_sentinel" else None
    dg, du = bt.emulate_swiglu_bwd(dout, g, u, fault)
    return {"out": _entry(bt.emulate_swiglu(g, u, f_fwd), fwd, "out"),
            "dg": _entry(dg, bwd, "dg"), "du": _entry(du, bwd, "du")}


def eval_swiglu(n, family, fault=None):
    g, u, dout = bt.swiglu_inputs(family, n, _seed("swiglu", n))
    return _swiglu_eval(g, u, dout, fault)


def eval_swiglu_packed(case, family, fault=None):
    """The packed and transposing kernels: the same arithmetic per element
    on g = gu[:, :I], u = gu[:, I:]."""
    rows, inter = case
    g, u, dout = bt.swiglu_inputs(family, rows * inter,
                                  _seed("swiglu-gu", rows, inter))
    return _swiglu_eval(g, u, dout, None if fault == "tail_sentinel"
                        else fault)


def eval_ce(case, family, fault=None):
    T, V = case
    x, t, gs = bt.ce_inputs(family, T, V, _seed("ce", T, V))
    ref = bt.ce_ref_bound(x, t)
    f_fwd = fault if fault in ("lse_no_tail", "empty_s1",
                               "empty_s1_neg") else None
    _, lse_clean = bt.emulate_ce_fwd(x, t)
    loss, lse = bt.emulate_ce_fwd(x, t, f_fwd)
    bwd = bt.ce_bwd_ref_bound(x, t, lse_clean, gs)
    d = bt.emulate_ce_bwd(x, t, lse_clean, gs,
                          fault if fault == "onehot_plus1" else None)
    return {"lse": _entry(lse, ref, "lse"), "loss": _entry(loss, ref, "loss"),
            "dlogits": _entry(d, bwd, "dlogits")}


def eval_adamw(n, family, fault=None):
    out = {}
    for i, cfg in enumerate(bt.ADAMW_CONFIGS):
        p, g, m, v = bt.adamw_inputs(family, n, _seed("adamw", n, i))
        ref = bt.adamw_ref_bound(p, g, m, v, *cfg)
        p1, p16, m1, v1 = bt.emulate_adamw(p, g, m, v, *cfg, fault=fault)
        assert torch.equal(p16, p1.bfloat16())
        for name, got in (("p32", p1), ("m", m1), ("v", v1)):
            out["%s-step%d" % (name, cfg[5])] = _entry(got, ref, name)
    return out


OPS = {
    # op: (evaluate, cases, old limit, faults)
    "rmsnorm": (eval_rmsnorm, bt.RMSNORM_CASES, 3e-2,
                ("no_eps", "mean_2048", "kk_r2")),
    "rope": (eval_rope, bt.ROPE_CASES, 2e-2,
             ("pos_mod_table", "sin_sign_second_half")),
    "rope_qkv": (eval_rope_qkv, bt.ROPE_QKV_CASES, 2e-2,
                 ("sin_sign_second_half",)),
    "swiglu": (eval_swiglu, bt.SWIGLU_FLAT_N, 2e-2,
               ("tail_sentinel", "dsilu_no_g_term")),
    "swiglu_packed": (eval_swiglu_packed,
                      bt.SWIGLU_PACKED_CASES + bt.SWIGLU_BWD_T_CASES, 2e-2,
                      ("dsilu_no_g_term",)),
    "ce": (eval_ce, bt.CE_CASES, 3e-2,
           ("lse_no_tail", "onehot_plus1", "empty_s1")),
    "adamw": (eval_adamw, bt.ADAMW_N, 1e-4,
              ("no_bias_correction", "wd_after_update", "eps_in_sqrt")),
}
# rmsnorm's forward is held to 2e-2 by the old test and its backward to 3e-2:
# the laxer one is used for all its tensors here

# (op, fault) -> whether the old metric passes at the first case where the
# bound catches the fault: True = the old test would have let it through
OLD_METRIC_PASSES = {
    ("rmsnorm", "no_eps"): False,
    ("rmsnorm", "mean_2048"): True,
    ("rmsnorm", "kk_r2"): True,
    ("rope", "pos_mod_table"): False,
    ("rope", "sin_sign_second_half"): False,
    ("rope_qkv", "sin_sign_second_half"): False,
    ("swiglu", "tail_sentinel"): False,
    ("swiglu", "dsilu_no_g_term"): True,
    ("swiglu_packed", "dsilu_no_g_term"): False,
    ("ce", "lse_no_tail"): True,
    ("ce", "onehot_plus1"): False,
    ("ce", "empty_s1"): True,
    ("adamw", "no_bias_correction"): False,
    ("adamw", "wd_after_update"): True,
    ("adamw", "eps_in_sqrt"): True,
}


def _ratio(entry):
    got, ref, bound = entry
    if got.dtype == torch.float32 and torch.isnan(ref).any():
        # pinned NaN rows (no such input in the listed families)
        return bt.ce_loss_ok(got, {"loss": ref, "loss_bound": bound})
    return bt.bound_ratio(got, ref, bound)


# ---------------------------------------------------------------------------
# reference alone
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("family", bt.FAMILIES)
@pytest.mark.parametrize("op", sorted(OPS))
def test_clean_emulation_within_bounds(op, family):
    evaluate, cases, _, _ = OPS[op]
    worst = {}
    for case in cases:
        for name, entry in evaluate(case, family).items():
            ratio, ok = _ratio(entry)
            assert ok, f"{op} {case} {family} {name}: err/bound {ratio:.4g}"
            key = name.split("-")[0]
            worst[key] = max(worst.get(key, 0.0), ratio)
    print(f"{op} {family} max err/bound: " +
          " ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())))


@pytest.mark.parametrize("family", bt.FAMILIES)
@pytest.mark.parametrize("e5m2", [False, True], ids=["e4m3", "e5m2"])
def test_clean_fp8_emulation_is_exact(e5m2, family):
    for R, C in bt.FP8_CASES:
        for scale in bt.FP8_SCALES:
            x = bt.fp8_inputs(family, R, C, e5m2, scale,
                              _seed("fp8", R, C, e5m2, scale))
            ref = bt.fp8_cast_ref(x, scale, e5m2)
            out, out_t, amax = bt.emulate_fp8_cast(x, scale, e5m2)
            label = (R, C, e5m2, scale, family)
            assert torch.equal(bt.fp8_bits(out), bt.fp8_bits(ref["out"])), label
            assert torch.equal(bt.fp8_bits(out_t),
                               bt.fp8_bits(ref["out_t"])), label
            assert torch.equal(amax, ref["amax"]), label
            assert not torch.isnan(ref["out"].float()).any(), label


def test_pinned_rows_of_the_references():
    """Inputs whose fp64 value is not what the kernel is held to are pinned,
    not dropped: the 2^60 row of the rmsnorm edges (fp32 overflow: r = 0,
    y = 0 exactly) and an out-of-range CE target (NaN loss, finite lse)."""
    x, w, _, _ = bt.rmsnorm_inputs("edges", 3, 2048, 1)
    ref = bt.rmsnorm_fwd_ref_bound(x, w, EPS)
    y, r = bt.emulate_rmsnorm_fwd(x, w, EPS)
    assert ref["invrms"][1] == 0 and r[1] == 0
    assert (ref["y"][1] == 0).all() and (y[1].float() == 0).all()
    assert ref["invrms"][0] == pytest.approx(EPS ** -0.5, rel=1e-6)
    assert torch.isfinite(ref["y"]).all() and torch.isfinite(ref["invrms"]).all()

    logits, t, _ = bt.ce_inputs("flat", 3, 7, 2)
    t[0], t[2] = -100, 7
    ref = bt.ce_ref_bound(logits, t)
    loss, lse = bt.emulate_ce_fwd(logits, t)
    assert torch.isnan(ref["loss"]).tolist() == [True, False, True]
    assert bt.ce_loss_ok(loss, ref)[1]
    assert bt.bound_ratio(lse, ref["lse"], ref["lse_bound"])[1]
    assert not bt.ce_loss_ok(torch.zeros(3), ref)[1]


# ---------------------------------------------------------------------------
# sensitivity
# ---------------------------------------------------------------------------


def _catches(op, fault):
    """Every (case, family, tensor) at which the fault exceeds its bound,
    with err / bound and whether the old metric of that tensor passes
    there."""
    evaluate, cases, limit, _ = OPS[op]
    out = []
    for case in cases:
        for family in bt.FAMILIES:
            for name, entry in evaluate(case, family, fault).items():
                ratio, ok = _ratio(entry)
                if ok:
                    continue
                got, ref, _ = entry
                if op == "ce" and name in ("loss", "lse"):
                    # the old test compares the mean loss, absolutely
                    old = abs(got.double().mean().item() - ref.mean().item())
                    old_ok = old < 2e-2
                else:
                    old = bt.global_rel_err(got, ref)
                    old_ok = old < limit        # NaN: fails
                out.append((case, family, name, ratio, old, old_ok))
    return out


@pytest.mark.parametrize("op,fault", sorted(OLD_METRIC_PASSES))
def test_fault_exceeds_bound(op, fault):
    """The fault is over its bound somewhere; the old metric "lets it
    through" if it passes at one of the very places the bound catches it."""
    assert fault in OPS[op][3]
    hits = _catches(op, fault)
    assert hits, f"{op} {fault}: within every bound"
    through = [h for h in hits if h[5]]
    case, family, name, ratio, old, _ = (through or hits)[0]
    print(f"{op} {fault}: over the bound at {len(hits)} (case, family, "
          f"tensor); the old metric passes at {len(through)} of them, e.g. "
          f"{case} {family} {name}: err/bound {ratio:.3g}, old {old:.3g}")
    assert bool(through) == OLD_METRIC_PASSES[(op, fault)]


def test_every_listed_fault_is_exercised():
    for op, (_, _, _, faults) in OPS.items():
        for fault in faults:
            assert (op, fault) in OLD_METRIC_PASSES


def test_dres_before_round_breaks_bit_equality():
    """One rounding instead of two is the more accurate result and cannot
    exceed a bound centred on the exact value; the kernel is held to
    fused == bf16(bf16(dx) + dres) bit for bit instead, which this fault
    breaks at every listed case with more than a handful of elements."""
    for case in bt.RMSNORM_CASES:
        x, w, dy, other, _, r = _rms_base(case, "flat")[:6]
        plain = bt.emulate_rmsnorm_dx(dy, x, w, r)
        want = (plain.float() + other.float()).to(torch.bfloat16)
        assert torch.equal(bt.emulate_rmsnorm_dx(dy, x, w, r, other), want)
        bad = bt.emulate_rmsnorm_dx(dy, x, w, r, other, "dres_before_round")
        assert not torch.equal(bad, want), case
        ref = bt.rmsnorm_dx_ref_bound(dy, x, w, r, other)
        assert bt.bound_ratio(bad, ref["dx"], ref["dx_bound"])[1]


def test_empty_thread_sum_cannot_matter_at_the_kernels_max():
    """s = 1 in a CE thread that saw no column is multiplied by
    exp(-3.4e38 - M) = 0 in every combine: same bits as the clean run."""
    for T, V in bt.CE_CASES:
        x, t, _ = bt.ce_inputs("edges", T, V, _seed("ce", T, V))
        a = bt.emulate_ce_fwd(x, t)
        b = bt.emulate_ce_fwd(x, t, "empty_s1_neg")
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


FP8_OLD_METRIC_PASSES = {"truncate": False, "no_clamp": False,
                         "edge_tile_neighbour": False}


@pytest.mark.parametrize("fault", sorted(FP8_OLD_METRIC_PASSES))
def test_fp8_fault_breaks_equality(fault):
    """Every fp8 fault changes a byte at some listed case.  The old check,
    test_fp8_linear_numerics' 8e-2 on max|err| / max|ref|, applied to the
    dequantised cast itself: truncation passes it."""
    broken, old = [], 0.0
    nan_to_inf = lambda t: torch.nan_to_num(t.float(), nan=1e30)  # noqa: E731
    for e5m2 in (False, True):
        for R, C in bt.FP8_CASES:
            for scale in bt.FP8_SCALES:
                x = bt.fp8_inputs("edges", R, C, e5m2, scale,
                                  _seed("fp8", R, C, e5m2, scale))
                ref = bt.fp8_cast_ref(x, scale, e5m2)
                out, out_t, _ = bt.emulate_fp8_cast(x, scale, e5m2, fault)
                if not (torch.equal(bt.fp8_bits(out), bt.fp8_bits(ref["out"]))
                        and torch.equal(bt.fp8_bits(out_t),
                                        bt.fp8_bits(ref["out_t"]))):
                    broken.append((R, C, e5m2, scale))
                    old = max(old, bt.global_rel_err(
                        nan_to_inf(out_t), ref["out_t"].float()))
    assert broken, fault
    print(f"fp8 {fault}: {len(broken)} cases differ; old metric {old:.3g}")
    if fault == "edge_tile_neighbour":
        assert {(R, C) for R, C, _, _ in broken} == {(72, 200), (136, 64)}
    assert (old < 8e-2) == FP8_OLD_METRIC_PASSES[fault]


# ---------------------------------------------------------------------------
# coverage: properties of the inputs
# ---------------------------------------------------------------------------


def test_swiglu_edges_reach_exp2_overflow():
    for n in bt.SWIGLU_FLAT_N:
        g, _, _ = bt.swiglu_inputs("edges", n, _seed("swiglu", n))
        over = bt.swiglu_exp2_overflows(g)
        assert bool(over.any()) == (n >= len(bt.SWIGLU_EDGE_G)), n
        if n >= len(bt.SWIGLU_EDGE_G):
            assert set(g.float().unique().tolist()) == {
                torch.tensor(v).bfloat16().item() for v in bt.SWIGLU_EDGE_G}
    # -88 is the last finite one: only -100 overflows
    g = torch.tensor(bt.SWIGLU_EDGE_G).bfloat16()
    assert g[bt.swiglu_exp2_overflows(g)].tolist() == [-100.0]
    # the tail of the odd sizes holds edge values too
    assert bt.SWIGLU_FLAT_N[4] % 8 == 3


def test_ce_cases_put_a_row_maximum_in_the_tail():
    tails = 0
    for T, V in bt.CE_CASES:
        x, t, _ = bt.ce_inputs("edges", T, V, _seed("ce", T, V))
        in_tail = bt.ce_row_max_in_tail(x)
        if V % 8:
            assert in_tail[0], (T, V)
            assert t[0] == x[0].float().argmax()
            tails += 1
        else:
            assert not in_tail.any()
        assert ((t >= 0) & (t < V)).all()
    assert tails >= 3
    # V < 2048: threads without a column; V = 4099: a second, sparse sweep
    assert any(V < 2048 for _, V in bt.CE_CASES)
    assert bt.ce_chain(4099) == 8 * 2 + 1 + 9 and bt.ce_chain(1) == 0 + 1 + 9


@pytest.mark.parametrize("e5m2", [False, True], ids=["e4m3", "e5m2"])
@pytest.mark.parametrize("scale", bt.FP8_SCALES)
def test_fp8_edges_hold_ties_subnormals_and_saturation(scale, e5m2):
    """Exact ties need y = fp32(x) * inv to have at most 5 significant
    bits.  For the power-of-two scales the edges family constructs them.
    For 0.37 the family holds every bf16 x whose fp32 product happens to
    round onto a tie, found by search (30 for e4m3, none at all for e5m2),
    and the bf16 value next to scale times each tie, where the fp32
    product decides the result."""
    R, C = bt.FP8_CASES[1]
    x = bt.fp8_inputs("edges", R, C, e5m2, scale,
                      _seed("fp8", R, C, e5m2, scale))
    cov = bt.fp8_edge_coverage(x, scale, e5m2)
    print(f"scale {scale} e5m2 {e5m2}: {cov}")
    assert cov["subnormal"] >= 1 and cov["saturating"] >= 1, cov
    assert (x.float() == 0).any()
    assert cov["near_tie"] >= 1, cov
    if scale != 0.37 or not e5m2:
        assert cov["tie"] >= 1, cov
    else:
        assert bt.fp8_exact_tie_inputs(scale, e5m2).numel() == 0


def test_transpose_cases_cover_the_short_block_group():
    assert [(R // 64) % 32 for R, _ in bt.TRANSPOSE_CASES] == [1, 1]
    assert bt.TRANSPOSE_CASES[1][0] // 64 == 33
