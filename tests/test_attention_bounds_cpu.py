"""The attention error bounds of torchx_amd.ops.bounds, checked without a
GPU against a plain torch emulation of the kernels' arithmetic (same wave /
tile structure, same defer-max decision, bf16 rounding at the same points).

  reference alone  the emulation stays within every bound at every (shape,
                   family, mask) the GPU tests use: the cap err/bound <= 1
                   is not a property of one lucky input;
  sensitivity      each injected kernel fault pushes the emulation over the
                   bound, and the faults the older metric
                   (max|err| / max|ref| under 3e-2 forward, 4e-2 backward)
                   lets through are shown to pass it;
  coverage         the stepped family reaches both sides of the rescale
                   decision with a live accumulator at every shape used.
"""

import functools

import pytest
import torch

from torchx_amd.ops import bounds as bd

OLD_FWD_LIMIT = 3e-2     # test_ops_gpu.py::test_attention_fwd
OLD_BWD_LIMIT = 4e-2     # test_ops_gpu.py::test_attention_bwd
GRADS = ("dq", "dk", "dv")


def _ids(cases):
    return [c[0] for c in cases]


@functools.lru_cache(maxsize=None)
def _train(cid, B, S, Hq, Hkv, causal, scale, family):
    """Inputs, fp64 references and the clean emulation of one training case;
    computed once, shared and never modified."""
    q, k, v, do = bd.attention_inputs(family, B, S, Hq, Hkv,
                                      seed=bd.case_seed(cid))
    fwd = bd.attention_fwd_ref_bound(q, k, v, scale, causal)
    o, lse = bd.emulate_attention_fwd(q, k, v, scale, causal)
    return q, k, v, do, fwd, o, lse


def _ratios(got, ref, names):
    return {n: bd.bound_ratio(g, ref[n], ref[n + "_bound"])[0]
            for g, n in zip(got, names)}


# ---------------------------------------------------------------------------
# reference alone
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("family", bd.FAMILIES)
@pytest.mark.parametrize("case", bd.FWD_CASES, ids=_ids(bd.FWD_CASES))
def test_emulated_fwd_within_bounds(case, family):
    q, k, v, do, fwd, o, lse = _train(*case, family)
    r = _ratios((o, lse), fwd, ("o", "lse"))
    print(f"{case[0]} {family} max err/bound: o {r['o']:.3g} "
          f"lse {r['lse']:.3g}")
    assert r["o"] <= 1 and r["lse"] <= 1, r


@pytest.mark.parametrize("family", bd.FAMILIES)
@pytest.mark.parametrize("case", bd.BWD_CASES, ids=_ids(bd.BWD_CASES))
def test_emulated_bwd_within_bounds(case, family):
    q, k, v, do, fwd, o, lse = _train(*case, family)
    scale, causal = case[6], case[5]
    ref = bd.attention_bwd_ref_bound(q, k, v, o, do, lse, scale, causal)
    got = bd.emulate_attention_bwd(q, k, v, o, do, lse, scale, causal)
    r = _ratios(got, ref, GRADS)
    print(f"{case[0]} {family} max err/bound: " +
          " ".join(f"{n} {r[n]:.3g}" for n in GRADS))
    assert max(r.values()) <= 1, r


def _paged_inputs(case, family):
    cid, B, S, Hq, Hkv, P, ctx = case
    q, k, v, _ = bd.attention_inputs(family, B, S, Hq, Hkv, T=max(ctx) + S,
                                     seed=bd.case_seed(cid))
    return q, k, v


@pytest.mark.parametrize("family", bd.FAMILIES)
@pytest.mark.parametrize("case", bd.PAGED_CASES, ids=_ids(bd.PAGED_CASES))
def test_emulated_paged_prefill_within_bounds(case, family):
    ctx = case[6]
    q, k, v = _paged_inputs(case, family)
    ref = bd.attention_fwd_ref_bound(q, k, v, bd.SCALE, True, ctx=ctx)
    o, _ = bd.emulate_attention_fwd(q, k, v, bd.SCALE, True, ctx=ctx)
    ratio, ok = bd.bound_ratio(o, ref["o"], ref["o_bound"])
    print(f"{case[0]} {family} max err/bound: o {ratio:.3g}")
    assert ok, ratio


@pytest.mark.parametrize("family", bd.FAMILIES)
@pytest.mark.parametrize("case", bd.DECODE_CASES, ids=_ids(bd.DECODE_CASES))
def test_emulated_decode_within_bounds(case, family):
    cid, B, Hq, Hkv, L = case
    q, kc, vc = bd.decode_inputs(family, B, Hq, Hkv, bd.DECODE_T,
                                 seed=bd.case_seed(cid))
    ref = bd.decode_ref_bound(q, kc, vc, [L] * B, bd.SCALE)
    o = bd.emulate_decode(q, kc, vc, [L] * B, bd.SCALE)
    ratio, ok = bd.bound_ratio(o, ref["o"], ref["o_bound"])
    print(f"{cid} {family} max err/bound: o {ratio:.3g}")
    assert ok, ratio


def test_references_agree_with_fp32_reference():
    """The fp64 forward reference is the operation the fp32 reference of the
    older tests computes, and the fp64 backward is its autograd gradient."""
    from torchx_amd.ops import reference

    cid, B, S, Hq, Hkv, causal, scale = bd.FWD_CASES[2]
    q, k, v, do, fwd, _, _ = _train(*bd.FWD_CASES[2], "flat")
    o32 = reference.attention(q, k, v, causal=causal, scale=scale)
    assert bd.global_rel_err(o32, fwd["o"]) < 1e-2
    lse32 = reference.attention_lse(q, k, v, causal=causal, scale=scale)
    assert (lse32.double() - fwd["lse"]).abs().max() < 1e-4
    leaves = [x.double().requires_grad_(True) for x in (q, k, v)]
    G = Hq // Hkv
    qf = leaves[0].permute(0, 2, 1, 3)
    kf = leaves[1].permute(0, 2, 1, 3).repeat_interleave(G, dim=1)
    vf = leaves[2].permute(0, 2, 1, 3).repeat_interleave(G, dim=1)
    s = (qf @ kf.transpose(-1, -2)) * scale
    s = s.masked_fill(torch.ones(S, S, dtype=torch.bool).triu(1),
                      float("-inf"))
    o64 = (torch.softmax(s, -1) @ vf).permute(0, 2, 1, 3)
    assert torch.allclose(o64, fwd["o"], rtol=1e-12, atol=1e-14)
    o64.backward(do.double())
    ref = bd.attention_bwd_ref_bound(q, k, v, o64.detach(), do, fwd["lse"],
                                     scale, causal)
    for leaf, n in zip(leaves, GRADS):
        assert torch.allclose(leaf.grad, ref[n], rtol=1e-9, atol=1e-12), n


# ---------------------------------------------------------------------------
# coverage of the rescale decision
# ---------------------------------------------------------------------------


def _assert_coverage(cov, S, ctx=None):
    assert cov["rescale"] >= 1, cov
    assert cov["deferred"] >= 1, cov
    assert cov["undecided"] == 0, cov
    if bd.every_tile_full(S, ctx):
        assert cov["ambiguous"] == 0, cov


@pytest.mark.parametrize("case", bd.FWD_CASES, ids=_ids(bd.FWD_CASES))
def test_stepped_reaches_both_sides_of_rescale(case):
    q, k = _train(*case, "stepped")[:2]
    cov = bd.rescale_coverage(q, k, case[6], case[5])
    print(case[0], cov)
    _assert_coverage(cov, case[2])


@pytest.mark.parametrize("case", bd.PAGED_CASES, ids=_ids(bd.PAGED_CASES))
def test_stepped_reaches_both_sides_of_rescale_paged(case):
    q, k, _ = _paged_inputs(case, "stepped")
    cov = bd.rescale_coverage(q, k, bd.SCALE, True, ctx=case[6])
    print(case[0], cov)
    _assert_coverage(cov, case[2], case[6])


def test_flat_never_rescales_a_live_accumulator():
    """Why the stepped family exists: on randn inputs the rescale branch is
    taken on tile 0 only."""
    for case in bd.FWD_CASES[:4]:
        q, k = _train(*case, "flat")[:2]
        _, _, logs = bd._run_fwd_tiled(q, k, torch.zeros_like(k), case[6],
                                       case[5], None, torch.float64, None)
        assert not any(rs.any() for log in logs for _, t, _, rs in log
                       if t > 0)


# ---------------------------------------------------------------------------
# sensitivity: injected faults exceed the bound
# ---------------------------------------------------------------------------

S320 = bd.FWD_CASES[0]


def _fwd_fault(case, family, fault):
    q, k, v, do, fwd, _, _ = _train(*case, family)
    o, lse = bd.emulate_attention_fwd(q, k, v, case[6], case[5], fault=fault)
    return _ratios((o, lse), fwd, ("o", "lse"))


def _bwd_fault(case, family, fault, lse_shift=0.0):
    q, k, v, do, fwd, o, lse = _train(*case, family)
    ref = bd.attention_bwd_ref_bound(q, k, v, o, do, lse, case[6], case[5])
    got = bd.emulate_attention_bwd(q, k, v, o, do, lse + lse_shift, case[6],
                                   case[5], fault=fault)
    return _ratios(got, ref, GRADS)


def test_fault_skip_rescale():
    r = _fwd_fault(S320, "stepped", "skip_rescale")
    print("skip acc_o *= alpha, stepped: o err/bound", r["o"])
    assert r["o"] > 1
    # randn inputs do not see it at all: the very bits of the correct kernel
    q, k, v, do, fwd, o, lse = _train(*S320, "flat")
    o_f, lse_f = bd.emulate_attention_fwd(q, k, v, S320[6], True,
                                          fault="skip_rescale")
    assert torch.equal(o_f, o) and torch.equal(lse_f, lse)
    assert bd.global_rel_err(o_f, fwd["o"]) < OLD_FWD_LIMIT


def test_fault_drop_tile():
    r = _fwd_fault(S320, "flat", "drop_tile")
    print("drop a kv tile for the last wave, flat: o err/bound", r["o"])
    assert r["o"] > 1
    # under stepped the early tiles carry no mass: correctly within the bound
    assert _fwd_fault(S320, "stepped", "drop_tile")["o"] <= 1


def test_fault_skip_subtile():
    r = _bwd_fault(S320, "flat", "skip_subtile")
    print("skip a 32-q sub-tile in dK/dV, flat: err/bound", r)
    assert r["dk"] > 1 and r["dv"] > 1
    assert r["dq"] <= 1                   # dQ does not take that path


def test_fault_delta_neighbour():
    for family in bd.FAMILIES:
        r = _bwd_fault(S320, family, "delta_neighbour")
        print(f"neighbour's delta, {family}: err/bound", r)
        assert r["dq"] > 1 and r["dk"] > 1
        assert r["dv"] <= 1               # dV does not read delta


def test_fault_lse_shift():
    for family in bd.FAMILIES:
        q, k, v, do, fwd, o, lse = _train(*S320, family)
        ratio, ok = bd.bound_ratio(lse + 0.01, fwd["lse"], fwd["lse_bound"])
        print(f"lse + 0.01, {family}: lse err/bound {ratio:.3g}")
        assert not ok and ratio > 10
        # and a backward that reads such an lse
        r = _bwd_fault(S320, family, None, lse_shift=0.01)
        print(f"backward on lse + 0.01, {family}: err/bound", r)
        assert min(r.values()) > 1
        # the older lse check allowed 2e-2 of max|lse|, ten times this shift
        assert 2e-2 * fwd["lse"].abs().max() > 0.1


def test_fault_mask_off_by_one():
    for family in bd.FAMILIES:
        r = _fwd_fault(S320, family, "mask_off_by_one")
        print(f"causal mask off by one, {family}: err/bound", r)
        assert r["o"] > 1 and r["lse"] > 1


# ---------------------------------------------------------------------------
# what the older metric lets through.  max|ref| of a causal output is set by
# the first rows (row 0 is v[0] itself) while the rows a fault hits average
# hundreds of values, so the fault's error has to reach 3-4 % of the largest
# element of the tensor to be seen.  One head pair at S = 512; the scores of
# the first case are flattened (scale / 4) so that no single key dominates
# a row.
# ---------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _blind(scale):
    q, k, v, do = bd.attention_inputs("flat", 1, 512, 2, 1, seed=512)
    fwd = bd.attention_fwd_ref_bound(q, k, v, scale, True)
    o, lse = bd.emulate_attention_fwd(q, k, v, scale, True)
    bwd = bd.attention_bwd_ref_bound(q, k, v, o, do, lse, scale, True)
    return q, k, v, do, fwd, o, lse, bwd


def test_old_metric_passes_dropped_tile():
    scale = bd.SCALE / 4
    q, k, v, do, fwd, o, lse, bwd = _blind(scale)
    o_f, _ = bd.emulate_attention_fwd(q, k, v, scale, True,
                                      fault="drop_tile")
    old = bd.global_rel_err(o_f, fwd["o"])
    new = bd.bound_ratio(o_f, fwd["o"], fwd["o_bound"])[0]
    print(f"dropped tile: old rel_err {old:.3g}, err/bound {new:.3g}")
    assert old < OLD_FWD_LIMIT and new > 1


def test_old_metric_passes_skipped_subtile():
    scale = bd.SCALE / 4
    q, k, v, do, fwd, o, lse, bwd = _blind(scale)
    got = bd.emulate_attention_bwd(q, k, v, o, do, lse, scale, True,
                                   fault="skip_subtile")
    old = {n: bd.global_rel_err(g, bwd[n]) for g, n in zip(got, GRADS)}
    new = _ratios(got, bwd, GRADS)
    print(f"skipped sub-tile: old rel_err {old}, err/bound {new}")
    assert max(old.values()) < OLD_BWD_LIMIT
    assert new["dk"] > 1 and new["dv"] > 1


def test_old_metric_passes_neighbour_delta():
    q, k, v, do, fwd, o, lse, bwd = _blind(bd.SCALE)
    got = bd.emulate_attention_bwd(q, k, v, o, do, lse, bd.SCALE, True,
                                   fault="delta_neighbour")
    old = {n: bd.global_rel_err(g, bwd[n]) for g, n in zip(got, GRADS)}
    new = _ratios(got, bwd, GRADS)
    print(f"neighbour's delta: old rel_err {old}, err/bound {new}")
    assert max(old.values()) < OLD_BWD_LIMIT
    assert new["dq"] > 1
