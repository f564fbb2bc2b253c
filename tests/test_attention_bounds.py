"""Every attention kernel against an fp64 reference under a derived
per-element bound (torchx_amd.ops.bounds): training forward + lse, the
backward trio, paged prefill and decode, each on two input families.

``flat`` (randn) spreads the softmax mass over all tiles, so a dropped or
duplicated tile or sub-tile shows; ``stepped`` makes the running max climb
from tile to tile, so the O-wide rescale and the deferred side of the
defer-max decision both run with a live accumulator — which randn inputs
never reach after tile 0.  For ``stepped`` the coverage of that decision is
asserted on the very inputs, by an fp64 replay, before the kernel runs.

Each test asserts err <= bound elementwise and prints max err/bound;
tests/test_attention_bounds_cpu.py shows without a GPU that an emulation of
the kernels' arithmetic stays within the same bounds on the same cases and
that injected faults do not.  The other forms of each kernel (split dK/dV,
recompute dQ, the forward block maps, packed qkv, ragged prefill, paged
decode) are tied to the ones tested here by torch.equal elsewhere.
"""

import pytest
import torch

from torchx_amd.ops import bounds as bd

pytestmark = pytest.mark.gpu

D = 128
GRADS = ("dq", "dk", "dv")


def _ids(cases):
    return [c[0] for c in cases]


def _ops():
    from torchx_amd import ops

    assert ops.extension_available(), "HIP extension must be built in-tree"
    return ops


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _check(label, got, ref, names):
    """Print max err/bound per tensor, then assert err <= bound elementwise."""
    res = {n: bd.bound_ratio(g, ref[n], ref[n + "_bound"])
           for g, n in zip(got, names)}
    print(f"{label} max err/bound: " +
          " ".join(f"{n} {res[n][0]:.3g}" for n in names))
    for n in names:
        assert res[n][1], f"{label}: {n} max err/bound = {res[n][0]:.4g}"


def _assert_coverage(label, q, k, scale, causal, S, ctx=None):
    """stepped inputs only: both sides of the rescale decision are reached
    with a live accumulator, and fp32 cannot decide otherwise than the fp64
    replay.  Where every wave and tile is full, no decision is within 1 of
    the threshold either (bounds.every_tile_full says why not elsewhere)."""
    cov = bd.rescale_coverage(q, k, scale, causal, ctx=ctx)
    print(f"{label} rescale coverage: {cov}")
    assert cov["rescale"] >= 1, cov
    assert cov["deferred"] >= 1, cov
    assert cov["undecided"] == 0, cov
    if bd.every_tile_full(S, ctx):
        assert cov["ambiguous"] == 0, cov


_FWD_RUNS = {}


def _fwd_run(case, family, dev):
    """Inputs and the kernel forward of one training case, computed once
    and shared by the forward and the backward test; never modified."""
    key = (case[0], family)
    if key not in _FWD_RUNS:
        cid, B, S, Hq, Hkv, causal, scale = case
        q, k, v, do = bd.attention_inputs(family, B, S, Hq, Hkv,
                                          seed=bd.case_seed(cid), device=dev)
        o, lse = _ops().hip_ops(required=True).attn_fwd(q, k, v, scale,
                                                        causal)
        _FWD_RUNS[key] = (q, k, v, do, o, lse)
    return _FWD_RUNS[key]


@pytest.mark.parametrize("family", bd.FAMILIES)
@pytest.mark.parametrize("case", bd.FWD_CASES, ids=_ids(bd.FWD_CASES))
def test_attn_fwd_bounds(dev, case, family):
    cid, B, S, Hq, Hkv, causal, scale = case
    q, k, v, do, o, lse = _fwd_run(case, family, dev)
    if family == "stepped":
        _assert_coverage(f"{cid} {family}", q, k, scale, causal, S)
    assert o.shape == q.shape and o.dtype == torch.bfloat16
    assert lse.shape == (B, Hq, S) and lse.dtype == torch.float32
    ref = bd.attention_fwd_ref_bound(q, k, v, scale, causal)
    _check(f"attn_fwd {cid} {family}", (o, lse), ref, ("o", "lse"))


@pytest.mark.parametrize("family", bd.FAMILIES)
@pytest.mark.parametrize("case", bd.BWD_CASES, ids=_ids(bd.BWD_CASES))
def test_attn_bwd_bounds(dev, case, family):
    """The default backward (merged dK/dV kernel, streamed dQ) on the o and
    lse of the kernel forward; the reference takes the same o and lse."""
    cid, B, S, Hq, Hkv, causal, scale = case
    ops = _ops()
    q, k, v, do, o, lse = _fwd_run(case, family, dev)
    impl, mode = ops.get_attn_bwd_dkv_impl(), ops.get_attn_bwd_dq_mode()
    try:
        ops.set_attn_bwd_dkv_impl("merged")
        ops.set_attn_bwd_dq_mode("stream")
        got = ops.hip_ops().attn_bwd(q, k, v, o, do, lse, scale, causal)
    finally:
        ops.set_attn_bwd_dkv_impl(impl)
        ops.set_attn_bwd_dq_mode(mode)
    for g, like in zip(got, (q, k, v)):
        assert g.shape == like.shape and g.dtype == torch.bfloat16
    ref = bd.attention_bwd_ref_bound(q, k, v, o, do, lse, scale, causal)
    _check(f"attn_bwd {cid} {family}", got, ref, GRADS)


def _scatter_to_pools(k, v, P, lengths, seed, dev):
    """Pools [num_pages, P, Hkv, D] and an int32 table [B, M] holding the
    logical caches k, v [B, T, Hkv, D]: sequence b's pages are distinct
    physical pages of a seeded permutation of 1 .. num_pages - 1, the rows
    past lengths[b] and the pages no table names hold other randn values,
    unused table entries stay 0."""
    B, T, Hkv, _ = k.shape
    n = [-(-L // P) for L in lengths]
    num_pages = sum(n) + 4
    g = torch.Generator().manual_seed(seed)
    perm = (torch.randperm(num_pages - 1, generator=g) + 1).tolist()
    kpool = torch.randn(num_pages, P, Hkv, D, generator=g).bfloat16().to(dev)
    vpool = torch.randn(num_pages, P, Hkv, D, generator=g).bfloat16().to(dev)
    bt = torch.zeros(B, max(n) + 2, dtype=torch.int32)
    at = 0
    for b in range(B):
        for j in range(n[b]):
            page = perm[at]
            at += 1
            bt[b, j] = page
            rows = min(P, lengths[b] - j * P)
            kpool[page, :rows] = k[b, j * P:j * P + rows]
            vpool[page, :rows] = v[b, j * P:j * P + rows]
    return kpool, vpool, bt.to(dev)


@pytest.mark.parametrize("family", bd.FAMILIES)
@pytest.mark.parametrize("case", bd.PAGED_CASES, ids=_ids(bd.PAGED_CASES))
def test_paged_prefill_bounds(dev, case, family):
    """ctx % 128 != 0: the waves group other rows than the dense kernel's,
    so nothing ties these outputs to attn_fwd."""
    cid, B, S, Hq, Hkv, P, ctx = case
    ops = _ops()
    q, k, v, _ = bd.attention_inputs(family, B, S, Hq, Hkv, T=max(ctx) + S,
                                     seed=bd.case_seed(cid), device=dev)
    if family == "stepped":
        _assert_coverage(f"{cid} {family}", q, k, bd.SCALE, True, S, ctx)
    lengths = [c + S for c in ctx]
    kpool, vpool, bt = _scatter_to_pools(k, v, P, lengths,
                                         bd.case_seed(cid) + 1, dev)
    ctx_t = torch.tensor(ctx, dtype=torch.int32, device=dev)
    o = ops.paged_prefill_attention(q, kpool, vpool, bt, ctx_t, bd.SCALE)
    assert o.shape == q.shape and o.dtype == torch.bfloat16
    ref = bd.attention_fwd_ref_bound(q, k, v, bd.SCALE, True, ctx=ctx)
    _check(f"paged_prefill {cid} {family}", (o,), ref, ("o",))


@pytest.mark.parametrize("family", bd.FAMILIES)
@pytest.mark.parametrize("case", bd.DECODE_CASES, ids=_ids(bd.DECODE_CASES))
def test_decode_bounds(dev, case, family):
    """decode_attention (host length) and decode_attention_dev (device
    positions, one per row) on the split and the single-pass path."""
    cid, B, Hq, Hkv, L = case
    ops = _ops()
    q, kc, vc = bd.decode_inputs(family, B, Hq, Hkv, bd.DECODE_T,
                                 seed=bd.case_seed(cid), device=dev)
    assert (bd.decode_split(B, Hq) > 1) == cid.startswith("split")
    ref = bd.decode_ref_bound(q, kc, vc, [L] * B, bd.SCALE)
    o = ops.decode_attention(q, kc, vc, L, bd.SCALE)
    pos = torch.full((B,), L - 1, dtype=torch.int32, device=dev)
    o_dev = ops.decode_attention_dev(q, kc, vc, pos, bd.SCALE)
    for name, got in (("decode_attention", o),
                      ("decode_attention_dev", o_dev)):
        assert got.shape == q.shape and got.dtype == torch.bfloat16
        _check(f"{name} {cid} {family}", (got,), ref, ("o",))
